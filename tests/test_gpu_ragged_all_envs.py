"""MI355X: the multi-class (ragged) engine for every env id -- the CPU matrix of tests/test_ragged_all_envs.py on the device, and a
full-size size curriculum per env id admitted to the multi-class engine by this test's feature."""
import pytest
import torch

from ragged_all_check import check_equals_uniform, check_full_size, check_ragged_all, full_size_sizes
from test_ragged_all_envs import CASES, EQUIV, _id

import graphenvs_amd as ge

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return "cuda:0"


@pytest.mark.parametrize("prefetch", [0, 2])
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_gpu_ragged_every_env_matches_oracle(device, case, prefetch):
    import oracle
    eid, sizes, common, steps = case
    check_ragged_all(ge, oracle, eid, sizes, common, device=device, steps=steps, prefetch=prefetch)


@pytest.mark.parametrize("eid,sizes,common", EQUIV, ids=[e[0].split("-")[0] + str(i) for i, e in enumerate(EQUIV)])
def test_gpu_ragged_equals_uniform_engines(device, eid, sizes, common):
    check_equals_uniform(ge, eid, sizes, common, device=device, steps=12)


FULL = [
    ("LongestPath-v0", dict(parenting=2), {}),
    ("SteinerTree-v0", dict(n_dests=3), {}),
    ("SteinerTree-v0", {}, dict(mst=True)),
    ("TSP-v0", dict(parenting=1), {}),
    ("MulticastRouting-v0", dict(parenting=4), {}),
    ("DistributionCenter-v0", dict(parenting=2), {}),
    ("PerishableProductDelivery-v0", dict(parenting=1, n_products=1), {}),  # (three products: hardly an episode ends in 40 random steps)
]


@pytest.mark.parametrize("eid,common,opt", FULL, ids=["LongestPath", "SteinerTree", "MST", "TSP", "MulticastRouting", "DistributionCenter",
                                                       "PerishableProductDelivery"])
def test_gpu_ragged_full_size_curriculum(device, eid, common, opt):
    import oracle
    if opt.get("mst"):
        sizes = [(b, n, m, dict(n_dests=n - 1)) for b, n, m in full_size_sizes(eid, lo=32, hi=128)]
    else:
        sizes = full_size_sizes(eid)
    assert sum(s[0] for s in sizes) == 16384 and len(sizes) >= 64
    if eid == "SteinerTree-v0" and not opt:
        # n = 256, m = 1 024 is the widest class: its mask rows (32 words) still fit the LDS stage of the quad-per-slot kernel
        sizes[-1] = (sizes[-1][0], 256, 1024)
    check_full_size(ge, oracle, eid, sizes, common, device)
