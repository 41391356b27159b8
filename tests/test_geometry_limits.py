"""The largest graphs the engine admits, and the first ones it refuses.

For every env id and density rule the edge n_max of ge_get_layout is FOUND by bisection (limits_check.find_n_max), never assumed;
the tests assert what must hold around it: admitted up to n_max and refused with GE_E_TOOBIG and a message beyond it, ge_create and
ge_create_ragged admit what the layout query admits (the host sizes every slab from the layout answer), the host raises before it
allocates for the first size beyond, and at n_max the engine still equals the CPU oracle bit for bit.

CPU: the checks that need no kernel run on the sanitizer harness library (the same ge_api.hip), and so does one rollout at n_max.
A reset of one 794-node slot takes the harness about 80 s (the rollout test: 82 s; the slowest other harness test,
test_emulated_late_numpy_draws_of_large_graphs, took 111 s in the same session), so the rollouts of all nine env ids and the
multi-class engines at n_max, a dozen such resets and more, run on the device only.
DESIGN.md, "Graph limits", records the edges measured by this module."""
import os
import sys

import pytest

import limits_check as lc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402

import graphenvs_amd as ge  # noqa: E402

# TSP on the complete graph without is_eval_env: the engine whose ge_inject_state carve (with the {neighbour, code} list) is larger
# than its reset carve (GeParams.nocolw)
COMPLETE_TSP = ("TSP-v0", dict(parenting=1), "complete")
GEOMETRIES = [(env_id, kw, density) for env_id, kw in lc.ENV_KWARGS.items() for density in ("dense", "sparse")] + [COMPLETE_TSP]
IDS = [f"{e.split('-')[0]}-{d}" for e, _, d in GEOMETRIES]
DENSE = [(env_id, kw) for env_id, kw in lc.ENV_KWARGS.items()]
SHORT_EPISODES = ("DistributionCenter-v0",)  # about six steps an episode: a rollout of a dozen steps sees autoresets


@pytest.fixture(scope="module")
def emu():
    return build_emu.load()


def _n_max(lib, env_id, kw, density):
    n_max = lc.find_n_max(lib, env_id, kw, density, lo=16 if density == "complete" else 64)
    print(f"n_max {env_id} {kw} {density}: n = {n_max}, m = {lc.n_edges_of(lib, env_id, kw, density, n_max)}")
    return n_max


def _ragged_sizes(lib, env_id, kw, n_max):
    return [(1, n_max, lc.n_edges_of(lib, env_id, kw, "dense", n_max)), (2, 40, 160), (2, 12, 36)]


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("env_id,kw,density", GEOMETRIES, ids=IDS)
def test_layout_edge_is_monotone(emu, env_id, kw, density):
    n_max = _n_max(emu, env_id, kw, density)
    if density != "complete":
        assert n_max > 600, "the admitted edge lies above the largest fixtures of the suite"
    lc.check_monotone_edge(emu, env_id, kw, density, n_max)


@pytest.mark.parametrize("env_id,kw,density", GEOMETRIES, ids=IDS)
def test_create_admits_what_the_layout_query_admits(emu, env_id, kw, density):
    lc.check_create_agrees(ge, emu, env_id, kw, density, _n_max(emu, env_id, kw, density), "cpu", emu)


@pytest.mark.parametrize("env_id,kw,density", GEOMETRIES, ids=IDS)
def test_host_refuses_the_first_size_beyond_the_edge_before_it_allocates(emu, env_id, kw, density):
    lc.check_refused_beyond(ge, emu, env_id, kw, density, _n_max(emu, env_id, kw, density), "cpu", emu)


def test_emulated_rollout_at_the_largest_admitted_graph(emu):
    """one slot of LongestPath with parenting 2 at n_max: the reset (adjacency rows of 13 words, the generic feature kernel at one
    wave), the walks in prune_scratch, and the whole observation after every step, under UBSan"""
    import oracle
    env_id, kw = "LongestPath-v0", lc.ENV_KWARGS["LongestPath-v0"]
    n_max = _n_max(emu, env_id, kw, "dense")
    lc.check_edge_rollout(ge, oracle, env_id, kw, n_max, lc.n_edges_of(emu, env_id, kw, "dense", n_max), "cpu", emu, B=1, K=3)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _hip():
    from graphenvs_amd import _lib
    return _lib.load()


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,kw,density", GEOMETRIES, ids=IDS)
def test_gpu_create_agrees_with_layout_and_refuses_beyond(env_id, kw, density):
    lib = _hip()
    n_max = _n_max(lib, env_id, kw, density)
    lc.check_monotone_edge(lib, env_id, kw, density, n_max)
    lc.check_create_agrees(ge, lib, env_id, kw, density, n_max, "cuda", below=(0, 1))
    lc.check_refused_beyond(ge, lib, env_id, kw, density, n_max, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,kw", DENSE, ids=[e for e, _ in DENSE])
def test_gpu_rollout_at_the_largest_admitted_graph(env_id, kw):
    import oracle
    lib = _hip()
    n_max = _n_max(lib, env_id, kw, "dense")
    short = env_id in SHORT_EPISODES
    lc.check_edge_rollout(ge, oracle, env_id, kw, n_max, lc.n_edges_of(lib, env_id, kw, "dense", n_max), "cuda", B=3,
                          K=24 if short else 12, want_episodes=1 if short else 0)


@pytest.mark.gpu
def test_gpu_complete_tsp_at_the_largest_admitted_graph_resets_steps_and_takes_an_injected_state():
    """the nocolw engine at its edge: the reset on the short carve against the oracle, then ge_inject_state on the full one"""
    import oracle
    from inject_check import check_inject
    env_id, kw, density = COMPLETE_TSP
    lib = _hip()
    n_max = _n_max(lib, env_id, kw, density)
    m = lc.n_edges_of(lib, env_id, kw, density, n_max)
    lc.check_edge_rollout(ge, oracle, env_id, kw, n_max, m, "cuda", B=2, K=6)
    check_inject(ge, oracle, "cuda", env_id, dict(n_nodes=n_max, n_edges=m, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,kw", DENSE, ids=[e for e, _ in DENSE])
def test_gpu_ragged_engine_with_a_class_at_the_largest_admitted_graph(env_id, kw):
    import oracle
    from ragged_all_check import check_ragged_all, make_ragged
    lib = _hip()
    sizes = _ragged_sizes(lib, env_id, kw, _n_max(lib, env_id, kw, "dense"))
    if env_id in ("LongestPath-v0", "TSP-v0"):  # parenting 2 with a class above 512 nodes: every class walks in prune_scratch
        env = make_ragged(ge, env_id, sizes, kw, "cuda")
        assert all(c.t["prune_scratch"] is not None and c.t["prune_scratch"].numel() == c.num_envs * 4 * c.W for c in env.classes)
        env.close()
    check_ragged_all(ge, oracle, env_id, sizes, kw, device="cuda", steps=24 if env_id == "PerishableProductDelivery-v0" else 12,
                     want_episodes=0 if env_id == "PerishableProductDelivery-v0" else 1)


@pytest.mark.gpu
def test_gpu_ragged_engine_at_the_edge_equals_uniform_engines():
    from ragged_all_check import check_equals_uniform
    env_id, kw = "LongestPath-v0", lc.ENV_KWARGS["LongestPath-v0"]
    lib = _hip()
    check_equals_uniform(ge, env_id, _ragged_sizes(lib, env_id, kw, _n_max(lib, env_id, kw, "dense")), kw, device="cuda", steps=12)
