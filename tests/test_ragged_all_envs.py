"""CPU: the multi-class (ragged) engine for every env id, through the kernels' CPU harness (tests/emu): every slot replayed on the
oracle through autoresets, the equivalence with one uniform engine per class, and the host-side refusals."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402
from ragged_all_check import check_equals_uniform, check_ragged_all  # noqa: E402

import graphenvs_amd as ge  # noqa: E402
from graphenvs_amd import _lib  # noqa: E402

GE_E_BADARG, GE_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def emu():
    return build_emu.load()


@pytest.fixture(scope="module")
def stress():
    """the stress build of tests/test_emu_kernels.py (same flags, same file): residual-graph walks in memory above 64 nodes
    (-DGE_MAXW=1), PerishableProductDelivery's wide placement above 6 nodes (-DGE_PPD_WIDE_ABOVE=6), and the other large-graph paths"""
    return build_emu.load(extra=["-DGE_F64_LV=3", "-DGE_NP_EARLY_MAX=8", "-DGE_MAXW=1", "-DGE_PPD_WIDE_ABOVE=6", "-DGE_BCW_REG_W=1", "-DGE_BW_TWO_ABOVE=64", "-DGE_BW_U=2"],
                          out=os.path.join(os.path.dirname(build_emu.OUT), "libgraphenvs_emu_stress.so"))


# (env id, sizes, kwargs common to the classes, steps): 3-5 classes, 1-3 slots each, sizes on both sides of 64 / 65
CASES = [
    ("LongestPath-v0", [(2, 12, 24), (1, 64, 160), (2, 65, 160)], dict(parenting=0), 12),
    ("LongestPath-v0", [(2, 12, 24), (1, 64, 160), (2, 65, 160)], dict(parenting=1), 12),
    ("LongestPath-v0", [(2, 12, 24), (1, 64, 160), (2, 65, 160)], dict(parenting=2), 12),
    ("LongestPath-v0", [(2, 12, 24), (1, 64, 160), (2, 65, 160)], dict(parenting=3), 12),
    ("SteinerTree-v0", [(2, 12, 30), (1, 64, 192), (2, 65, 195)], dict(n_dests=3), 16),
    ("SteinerTree-v0", [(2, 8, 14, dict(n_dests=7)), (1, 12, 30, dict(n_dests=11)), (1, 64, 192, dict(n_dests=63)), (2, 65, 195, dict(n_dests=64))], {}, 16),  # MST
    ("TSP-v0", [(2, 10, 20), (1, 64, 200), (2, 65, 200)], dict(parenting=1), 16),
    ("TSP-v0", [(2, 10, 20), (1, 64, 200), (2, 65, 200)], dict(parenting=2), 16),
    ("TSP-v0", [(2, 12, 30), (1, 20, 190), (2, 65, 200)], dict(parenting=2, spatial=True, is_eval_env=True), 16),  # (20, 190): complete
    ("TSP-v0", [(2, 10, 20), (1, 8, 28), (1, 66, 200)], dict(parenting=1, is_eval_env=True), 16),
    ("MulticastRouting-v0", [(2, 10, 20), (1, 64, 192), (2, 65, 195)], dict(parenting=1, is_eval_env=True), 12),
    ("MulticastRouting-v0", [(2, 10, 20), (1, 64, 192), (2, 65, 195)], dict(parenting=2), 12),
    ("MulticastRouting-v0", [(2, 10, 20, dict(n_dests=2)), (1, 64, 192), (2, 65, 195, dict(n_dests=4))], dict(parenting=3), 12),
    ("MulticastRouting-v0", [(2, 10, 20), (1, 8, 28), (2, 65, 195)], dict(parenting=4, is_eval_env=True), 12),
    ("DistributionCenter-v0", [(2, 12, 25, dict(target_count=4)), (1, 64, 192), (2, 65, 195)], dict(parenting=1, max_distance=1.5), 12),
    ("DistributionCenter-v0", [(2, 12, 25), (1, 64, 192, dict(max_distance=0.7)), (2, 65, 195)], dict(parenting=2), 12),
    ("PerishableProductDelivery-v0", [(2, 8, 12, dict(n_products=1)), (1, 64, 192), (2, 65, 195, dict(n_products=2))], dict(parenting=1), 16),
    ("MaxIndependentSet-v0", [(2, 8, 12), (1, 64, 192), (2, 65, 195)], dict(weighted=False, is_eval_env=True), 12),
    # the second class's mask rows (13 bytes each) start at byte 15 of the mask slab: single bytes, one 8-byte store, single bytes
    ("MaxIndependentSet-v0", [(3, 5, 7), (3, 13, 20)], dict(weighted=False, is_eval_env=True), 16),
]


def _id(case):
    eid, sizes, common, _ = case
    return eid.split("-")[0] + "-" + "-".join(f"{k}{v}" for k, v in common.items()) + f"-{len(sizes)}cls"


@pytest.mark.parametrize("prefetch", [0, 2])
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_emulated_ragged_every_env_matches_oracle(emu, case, prefetch):
    import oracle
    eid, sizes, common, steps = case
    check_ragged_all(ge, oracle, eid, sizes, common, library=emu, steps=steps, prefetch=prefetch)


@pytest.mark.parametrize("prefetch", [0, 2])
@pytest.mark.parametrize("eid,sizes,common", [
    ("LongestPath-v0", [(1, 12, 24), (2, 65, 160), (1, 70, 180)], dict(parenting=2)),   # PRUNE 2 for every class (one above 64 nodes)
    ("TSP-v0", [(2, 10, 20), (1, 66, 200)], dict(parenting=2)),
    ("PerishableProductDelivery-v0", [(2, 6, 8), (2, 12, 25)], dict(parenting=1, n_products=1)),  # n > 6: the wide placement
])
def test_emulated_ragged_stress_paths_match_oracle(stress, eid, sizes, common, prefetch):
    import oracle
    check_ragged_all(ge, oracle, eid, sizes, common, library=stress, steps=24, prefetch=prefetch)


EQUIV = [
    ("LongestPath-v0", [(2, 12, 24), (1, 65, 160)], dict(parenting=3)),
    ("TSP-v0", [(2, 10, 20), (1, 8, 28), (1, 65, 200)], dict(parenting=2, is_eval_env=True)),
    ("SteinerTree-v0", [(2, 8, 14, dict(n_dests=7)), (1, 65, 195, dict(n_dests=3))], dict(is_eval_env=True)),
    ("MulticastRouting-v0", [(2, 10, 20), (1, 65, 195)], dict(parenting=4)),
    # the widest mask row (2 m = 2 200 edges: 35 words) is beyond the quad kernel's LDS stage: the whole engine takes the
    # thread-per-slot kernel, while the uniform engine of the small class takes the quad kernel
    ("SteinerTree-v0", [(2, 10, 20), (1, 70, 1100)], dict(n_dests=3)),
    ("DistributionCenter-v0", [(2, 12, 25), (1, 65, 195)], dict(parenting=2)),
    ("PerishableProductDelivery-v0", [(2, 8, 12), (1, 65, 195)], dict(parenting=1)),
]


@pytest.mark.parametrize("eid,sizes,common", EQUIV, ids=[e[0].split("-")[0] + str(i) for i, e in enumerate(EQUIV)])
def test_emulated_ragged_equals_uniform_engines(emu, eid, sizes, common):
    check_equals_uniform(ge, eid, sizes, common, library=emu, steps=12)


def test_emulated_ragged_stress_equals_uniform_engines(stress):
    check_equals_uniform(ge, "LongestPath-v0", [(2, 12, 24), (1, 70, 180)], dict(parenting=2), library=stress, steps=12)


def test_ragged_per_class_kwargs_are_checked_before_any_device_call(emu):
    with pytest.raises(TypeError):
        ge.RaggedVectorEnv("LongestPath-v0", [(1, 10, 20), (1, 12, 24, dict(parenting=2))], device="cpu", _library=emu, parenting=1)
    with pytest.raises(TypeError):
        ge.RaggedVectorEnv("SteinerTree-v0", [(1, 10, 20, dict(weighted=False))], device="cpu", _library=emu)
    # the reference's defaults per class: DistributionCenter target_count = n // 5, n_edges = -1 where the reference allows it
    env = ge.RaggedVectorEnv("DistributionCenter-v0", [(1, 20, 40), (1, 40, 80)], device="cpu", _library=emu, parenting=2, prefetch=0)
    assert [c.cfg.n_dests for c in env.classes] == [4, 8]
    env.close()
    env = ge.RaggedVectorEnv("MulticastRouting-v0", [(1, 10, -1), (1, 12, -1)], device="cpu", _library=emu, prefetch=0)
    assert env.sizes == [(1, 10, 13), (1, 12, 19)] and env.mask_flat.numel() == 2 * 13 + 2 * 19
    env.close()


def _deferred(emu, parenting, b, n, m, base):
    return ge.VectorGraphEnv("LongestPath-v0", b, n, m, device="cpu", _library=emu, parenting=parenting, env_index_base=base,
                             _defer_create=True)


def test_ragged_create_refuses_classes_that_differ_in_parenting(emu):
    a, b = _deferred(emu, 1, 2, 12, 24, 0), _deferred(emu, 2, 2, 14, 28, 2)
    cfgs = (_lib.GeConfig * 2)(a.cfg, b.cfg)
    bufs = (_lib.GeBuffers * 2)(a.bufs, b.bufs)
    table = torch.zeros(int(emu.ge_ragged_table_bytes(2)), dtype=torch.uint8)
    sc, cs = torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    h = C.c_void_p()
    rc = emu.ge_create_ragged(cfgs, bufs, 2, table.data_ptr(), sc.data_ptr(), cs.data_ptr(), C.byref(h))
    assert rc == GE_E_BADARG and b"parenting" in emu.ge_last_error()


def test_ragged_inject_state_and_unseeded_reset_stay_unsupported(emu):
    env = ge.RaggedVectorEnv("TSP-v0", [(1, 10, 20), (1, 12, 30)], device="cpu", _library=emu, parenting=1, prefetch=0)
    env.reset(seed=1)
    links = torch.zeros(2 * 20 * 2, dtype=torch.int64)
    wcode = torch.zeros(2 * 20, dtype=torch.uint8)
    x = torch.zeros(10 * 16, dtype=torch.float32)
    assert emu.ge_inject_state(env._h, links.data_ptr(), wcode.data_ptr(), x.data_ptr(), None, None, None) == GE_E_UNSUPPORTED
    assert emu.ge_reset_continue(env._h, None) == GE_E_UNSUPPORTED
    env.close()
