"""CPU: the C-ABI library loads and exports every symbol include/graphenvs.h declares (no compute
calls without a GPU), config validation mirrors the reference constructors, the codec round-trips."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import graphenvs_amd as ge
from graphenvs_amd import _lib, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    _lib.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "graphenvs.h")).read()
    declared = set(re.findall(r"\b(ge_[a-z_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s
    assert lib.ge_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define GE_ABI_VERSION (\d+)", header).group(1))


def test_binary_carries_the_hash_of_its_sources(tmp_path):
    """the .so embeds the hash of csrc/* + the header; build() reuses a binary only when that hash equals
    the sources on disk, and load() refuses / rebuilds a stale one instead of mapping whatever file is there."""
    _lib.build()
    want = _lib.source_hash()
    assert _lib.built_hash() == want and _lib.load().ge_source_hash().decode() == want
    _lib.build()
    assert _lib.last_build == "reused"
    stale = tmp_path / "libstale.so"
    data = open(_lib.LIB_PATH, "rb").read()
    stale.write_bytes(data.replace(b"GE_SOURCE_HASH=" + want.encode(), b"GE_SOURCE_HASH=" + b"0" * 32))
    assert _lib.built_hash(str(stale)) == "0" * 32 != want


def test_struct_sizes_match_header_field_counts():
    header = open(os.path.join(ROOT, "include", "graphenvs.h")).read()
    body = header[header.index("typedef struct {\n  /* --- observation"):header.index("} ge_buffers;")]
    fields = re.findall(r"\*\s*([a-z_0-9]+);", body)
    assert fields == _lib.BUFFER_FIELDS


def test_layout_and_validation_without_gpu():
    lib = _lib.load()
    lay = _lib.GeLayout()
    cfg = _lib.GeConfig(0, 8, 64, 192, 1, -1, 0, 0, 0, 1, -1.0, 0, 8)
    assert lib.ge_get_layout(C.byref(cfg), C.byref(lay)) == 0
    assert (lay.F, lay.Fe, lay.A, lay.W, lay.E, lay.obs_len) == (7, 1, 64, 1, 384, 1600)  # 7n+6m
    cfg = _lib.GeConfig(2, 8, 256, 1024, 1, -1, 8, 0, 0, 1, -1.0, 0, 8)
    assert lib.ge_get_layout(C.byref(cfg), C.byref(lay)) == 0
    assert (lay.F, lay.Fe, lay.A, lay.obs_len) == (7, 2, 2048, 7 * 256 + 8 * 1024)
    cfg = _lib.GeConfig(3, 8, 10, 20, 1, 1, 0, 0, 0, 1, -1.0, 0, 8)
    assert lib.ge_get_layout(C.byref(cfg), C.byref(lay)) == 0 and lay.obs_len == 9 * 10 + 6 * 20  # tsp quirk, SURVEY 9.3
    # the reference's constructor asserts
    bad = [(_lib.GeConfig(0, 8, 10, 20, 1, 1, 0, 0, 0, 1, -1.0, 0, 8), b"shortest"),
           (_lib.GeConfig(3, 8, 10, 20, 1, -1, 0, 0, 0, 1, -1.0, 0, 8), b"1 or 2"),
           (_lib.GeConfig(4, 8, 10, 20, 1, 1, 0, 0, 0, 1, -1.0, 0, 8), b"Weighted"),
           (_lib.GeConfig(0, 8, 10, 5, 1, -1, 0, 0, 0, 1, -1.0, 0, 8), b"connected")]
    for cfg, msg in bad:
        assert lib.ge_get_layout(C.byref(cfg), C.byref(lay)) == -1
        assert msg.lower() in lib.ge_last_error().lower()


def test_host_asserts_match_reference_constructors():
    with pytest.raises(AssertionError, match="Parenting is not available"):
        ge.vector_env.normalize_kwargs("ShortestPath-v0", 10, 20, parenting=1)
    with pytest.raises(AssertionError, match="either 1 or 2"):
        ge.vector_env.normalize_kwargs("TSP-v0", 10, 20)
    with pytest.raises(AssertionError, match="Weighted graphs"):
        ge.vector_env.normalize_kwargs("DensestSubgraph-v0", 10, 20, parenting=1, weighted=True)
    kw = ge.vector_env.normalize_kwargs("DensestSubgraph-v0", 10, -1, parenting=1)
    assert kw["n_edges"] == int((10 * 9 // 2) * 0.30) and kw["n_choices"] == 3.0
    # the three remaining envs (multicast_routing.py:31-35,53-54; distribution_center.py:29-45; perishable_product_delivery.py:27-61)
    with pytest.raises(ValueError, match="Invalid parenting type"):
        ge.vector_env.normalize_kwargs("MulticastRouting-v0", 10, 20, parenting=5)
    kw = ge.vector_env.normalize_kwargs("MulticastRouting-v0", 12)
    assert kw["n_edges"] == 19 and kw["parenting"] == 4 and kw["n_dests"] == 3
    with pytest.raises(AssertionError):
        ge.vector_env.normalize_kwargs("DistributionCenter-v0", 10, 20, parenting=3)
    assert ge.vector_env.normalize_kwargs("DistributionCenter-v0", 23, 60)["target_count"] == 4
    with pytest.raises(AssertionError, match="Parenting must be 1"):
        ge.vector_env.normalize_kwargs("PerishableProductDelivery-v0", 10, 20)
    with pytest.raises(AssertionError, match="Max 5 products"):
        ge.vector_env.normalize_kwargs("PerishableProductDelivery-v0", 10, 20, parenting=1, n_products=6)
    kw = ge.vector_env.normalize_kwargs("PerishableProductDelivery-v0", 64, 192, parenting=1)
    avg = np.log(64) / np.log(6.0) * (0.3 + 1.0) / 2.0
    assert kw["_dt_window"] == (float(avg * 0.6), float(avg * 1.4))
    assert utils.get_env_info("MulticastRouting-v0") == (9, 2, "edge") and utils.get_env_info("PerishableProductDelivery-v0") == (21, 1, "node")


def _recorded_constructors():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "constructor_refusals.json")) as f:
        return [(c["env_id"], c["kwargs"], c["raised"], c["error"]) for c in json.load(f)["cases"]]


@pytest.fixture(scope="module")
def emu():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    return build_emu.load()


@pytest.mark.parametrize("env_id,kwargs,raised,error", _recorded_constructors(),
                         ids=[f"{e.split('-')[0]}-{'-'.join(f'{k}={v}' for k, v in kw.items() if k not in ('n_nodes', 'n_edges')) or 'defaults'}"
                              for e, kw, _, _ in _recorded_constructors()])
def test_constructors_refuse_exactly_what_the_reference_refuses(emu, env_id, kwargs, raised, error):
    """tests/golden/constructor_refusals.json: constructor calls and whether the reference's constructor raised (recorded once by
    oracle/gen_golden.py --constructors).  ge.make and ge.make_vec raise the same exception type for the refused ones and build an
    engine for the rest; derive() in ge_api.hip, asked directly past the host's asserts, answers GE_E_BADARG for the same set."""
    makers = [lambda: ge.make(env_id, device="cpu", _library=emu, **kwargs),
              lambda: ge.make_vec(env_id, 3, device="cpu", _library=emu, **kwargs)]
    for make in makers:
        if raised:
            with pytest.raises({"AssertionError": AssertionError, "ValueError": ValueError, "TypeError": TypeError}[error]):
                make()
        else:
            env = make()
            env.close() if hasattr(env, "close") else None
    if error == "TypeError":  # a kwarg the env does not take: nothing to put into a ge_config
        return
    kw = dict(ge.vector_env._DEFAULTS[env_id], **kwargs)
    if env_id == "DistributionCenter-v0":
        kw["target_count"] = kw["n_nodes"] // 5
    if env_id == "PerishableProductDelivery-v0":
        kw["_dt_window"] = (0.5, 1.5)
    cfg = ge.vector_env.make_config(env_id, 3, kw)
    rc = emu.ge_get_layout(C.byref(cfg), C.byref(_lib.GeLayout()))
    assert rc == (-1 if raised else 0), (rc, emu.ge_last_error())
    assert not raised or emu.ge_last_error()


# refusals of the engine's own ("Deliberate differences"): calls the reference's constructor accepts and then cannot
# serve -- its reset would not return, or raises later.  (kwargs, what the host raises, the engine's return code in the message)
OWN_REFUSALS = [
    ("ShortestPath-v0", dict(n_nodes=140, n_edges=147), RuntimeError, r"code -2\).*probability"),       # too disconnected to sample
    ("TSP-v0", dict(n_nodes=200, n_edges=380, parenting=1), RuntimeError, r"code -2\).*degree-1"),
    ("ShortestPath-v0", dict(n_nodes=12, n_edges=10), RuntimeError, r"code -1\).*no connected graph"),
    ("SteinerTree-v0", dict(n_nodes=12, n_edges=30, n_dests=0), RuntimeError, r"code -1\).*n_dests"),
    ("SteinerTree-v0", dict(n_nodes=12, n_edges=30, n_dests=12), RuntimeError, r"code -1\).*n_dests"),
    ("MulticastRouting-v0", dict(n_nodes=12, n_edges=30, n_dests=12), RuntimeError, r"code -1\).*n_dests"),
    ("PerishableProductDelivery-v0", dict(n_nodes=8, n_edges=12, n_products=5, parenting=1), RuntimeError, r"code -1\).*2 \* n_products"),
    ("PerishableProductDelivery-v0", dict(n_nodes=12, n_edges=30, parenting=1, delivery_time=2.0), AssertionError, "delivery_time"),
]


@pytest.mark.parametrize("env_id,kwargs,exc,match", OWN_REFUSALS)
def test_refusals_of_the_engine_alone_carry_their_code(emu, env_id, kwargs, exc, match):
    for make in (lambda: ge.make(env_id, device="cpu", _library=emu, **kwargs),
                 lambda: ge.make_vec(env_id, 3, device="cpu", _library=emu, **kwargs)):
        with pytest.raises(exc, match=match):
            make()


def test_product_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="GPU"):
        ge.make("ShortestPath-v0", n_nodes=10, n_edges=20)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ge.make("ShortestPath-v0", n_nodes=10, n_edges=20, device="cpu")


def test_codec_roundtrip_and_env_info():
    assert utils.get_env_info("ShortestPath-v0") == (7, 1, "node")
    assert utils.get_env_info("SteinerTree-v0") == (7, 2, "edge")
    assert utils.get_env_info("TSP-v0") == (9, 1, "node")
    assert utils.get_env_info("DensestSubgraph-v0") == (6, 1, "node")
    rng = np.random.default_rng(0)
    n, m, bs = 6, 8, 3
    nodes = rng.random((bs, n, 7), dtype=np.float32)
    edges = rng.random((bs, 2 * m, 1), dtype=np.float32)
    links = rng.integers(0, n, (bs, 2 * m, 2))
    from types import SimpleNamespace
    vec = np.stack([utils.vectorize_graph(SimpleNamespace(nodes=nodes[i], edges=edges[i], edge_links=links[i])) for i in range(bs)])
    x, ef, ei = utils.devectorize_graph(torch.from_numpy(vec), "ShortestPath-v0", n_nodes=n, n_edges=m)
    assert torch.equal(x, torch.from_numpy(nodes)) and torch.equal(ef, torch.from_numpy(edges))
    assert torch.equal(ei, torch.from_numpy(links))
    g = utils.to_pyg_graph(x, ef, ei)
    assert g.x.shape == (bs * n, 7) and g.edge_index.shape == (2, bs * 2 * m)
    assert torch.equal(g.edge_index[:, 2 * m:4 * m], torch.from_numpy(links[1]).T + n)  # utils.py:27 offset by i*n
    assert torch.equal(g.ptr, torch.arange(bs + 1) * n)


def test_hopeless_rejection_sampling_is_refused_without_a_gpu():
    """a G(n, m) that is connected with probability < 1e-7 would spin the reset kernel for ever (the reference too)"""
    L = _lib.load()
    cfg = _lib.GeConfig(0, 4, 140, 147, 1, -1, 0, 0, 0, 1, -1.0, 0, 4, 0, 0, 0.0, 0.0, 0.0)
    lay = _lib.GeLayout()
    assert L.ge_get_layout(C.byref(cfg), C.byref(lay)) == -2 and b"probability" in L.ge_last_error()
    cfg = _lib.GeConfig(0, 4, 64, 70, 1, -1, 0, 0, 0, 1, -1.0, 0, 4, 0, 0, 0.0, 0.0, 0.0)  # ~1 400 attempts on average: fine
    assert L.ge_get_layout(C.byref(cfg), C.byref(lay)) == 0


_STANDINS = {
    "gymnasium/__init__.py": """
from . import spaces, vector
from .envs.registration import register, registry
def make(id, **kw):
    return registry[id](**kw)
""",
    "gymnasium/spaces.py": """
class Discrete:
    def __init__(self, n): self.n = n
class MultiDiscrete:
    def __init__(self, nvec): self.nvec = list(nvec)
class Box:
    def __init__(self, low, high, shape, dtype): self.shape, self.dtype = tuple(shape), dtype
""",
    "gymnasium/vector/__init__.py": """
class VectorEnv:
    metadata = {}
""",
    "gymnasium/envs/__init__.py": "",
    "gymnasium/envs/registration.py": """
registry = {}
def register(id, entry_point, **kw):
    registry[id] = entry_point
""",
    "torch_geometric/__init__.py": "",
    "torch_geometric/data.py": """
class Data:
    def __init__(self, **kw): self.__dict__.update(kw)
class Batch(Data):
    pass
""",
}


def test_gymnasium_and_pyg_integration_with_stand_in_packages(tmp_path):
    """SURVEY 8f-4 / VERDICT r1 item 7: gymnasium and torch_geometric are not in the image, so the branches that use them run here
    against minimal stand-in packages (what refshim.py does for the reference): VectorGraphEnv subclasses gymnasium.vector.VectorEnv,
    the nine ids register and gymnasium.make() builds the facade, GraphBatch.to_pyg() yields a torch_geometric Batch."""
    import subprocess, sys, textwrap
    for rel, body in _STANDINS.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(body))
    code = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{str(tmp_path)!r}, {ROOT!r}, {os.path.join(ROOT, 'tests', 'emu')!r}]
        import gymnasium, torch_geometric.data
        import graphenvs_amd as ge, build_emu
        emu = build_emu.load()
        assert issubclass(ge.VectorGraphEnv, gymnasium.vector.VectorEnv)
        ge.register_with_gymnasium()
        assert sorted(gymnasium.registry) == sorted(ge.ENV_IDS) and len(ge.ENV_IDS) == 9
        env = gymnasium.make("ShortestPath-v0", n_nodes=8, n_edges=14, device="cpu", _library=emu)
        obs, info = env.reset(seed=3)
        assert obs.shape == (7 * 8 + 6 * 14,) and info["mask"].dtype == bool
        v = ge.VectorGraphEnv("SteinerTree-v0", 3, 8, 14, n_dests=2, device="cpu", _library=emu)
        assert isinstance(v, gymnasium.vector.VectorEnv) and v.num_envs == 3
        assert v.single_action_space.n == 14 and v.observation_space.shape == (3, v.obs_len) and v.metadata["autoreset_mode"] == "same_step"
        g, info = v.reset(seed=1)
        b = g.to_pyg()
        assert isinstance(b, torch_geometric.data.Batch) and b.x.shape == (24, 7) and b.edge_index.shape == (2, 84) and b._num_graphs == 3
        assert int(b.ptr[-1]) == 24 and int(b.batch[-1]) == 2
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
