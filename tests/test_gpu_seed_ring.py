"""GPU (MI355X): the generator-state ring against CPython's and numpy's own seeders, and the split seeding (GE_SEED_SPLIT: pass 1
of random.seed in the graph launch, pass 2 at the head of ge_k_features64's launch) against a -DGE_SEED_SPLIT=0 build of the same
sources, slab by slab after every step.  Bodies and shapes: tests/seed_ring_check.py (tests/test_emu_seed_ring.py runs the small
ones on the CPU harness)."""
import ctypes
import os
import subprocess

import pytest

import seed_ring_check as rc

pytestmark = pytest.mark.gpu


def _ge():
    import graphenvs_amd as ge
    return ge


@pytest.fixture(scope="module")
def unsplit():
    """the library of the same sources built with -DGE_SEED_SPLIT=0, beside the product; compiled when there is none of these sources"""
    from graphenvs_amd import _lib
    out = os.path.join(os.path.dirname(_lib.LIB_PATH), "libgraphenvs_hip_unsplit.so")
    if _lib.built_hash(out) != _lib.source_hash():
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.check_call(_lib.compile_command(tmp, ["-DGE_SEED_SPLIT=0"]), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(tmp, out)
    return _lib.bind(ctypes.CDLL(out))


@pytest.fixture(scope="module")
def libs(unsplit):
    return dict(split=None, unsplit=unsplit)  # None: the product (GE_SEED_SPLIT defaults to 1)


@pytest.mark.parametrize("build", ["split", "unsplit"])
@pytest.mark.parametrize("env_id,kw,B,expect", rc.RING_CASES, ids=rc.RING_IDS)
def test_ring_entries_equal_cpython_and_numpy_states(libs, build, env_id, kw, B, expect):
    print(rc.check_ring(_ge(), "cuda", libs[build], env_id, kw, B, expect))


@pytest.mark.parametrize("env_id,kw,B,expect", rc.RING_CASES[:4], ids=rc.RING_IDS[:4])
def test_split_build_leaves_the_slabs_of_the_unsplit_build(unsplit, env_id, kw, B, expect):
    queues = rc.check_same_rollout(rc.uniform(_ge(), "cuda", env_id, kw, B), None, unsplit, 25, min_episodes=B)
    assert any(q % 64 for q in queues), queues


@pytest.mark.parametrize("B", [3200, 4200])
def test_split_build_leaves_the_slabs_of_the_unsplit_build_when_the_queue_exceeds_a_trip(unsplit, B):
    """MaxIndependentSet n = 6 m = 8: every slot finishes in the same step, the sixth of its episode.  At B = 3 200 the seeding
    workgroups of both launches cover the whole queue in ONE trip of their stride loops -- the plan sizes them for the resident
    grid, which is one workgroup per slot up to 4 096 slots at this carve --, so the batch of 4 200 is run beside it: its queue
    of 4 200 exceeds the trips of 4 096 and both loops run twice, the second time over 104 items."""
    ge = _ge()
    probe = ge.VectorGraphEnv(rc.MIS, B, device="cuda", prefetch=0, n_nodes=6, n_edges=8)
    trips = rc.seeding_trips(probe)
    probe.close()
    queues = rc.check_same_rollout(rc.uniform(ge, "cuda", rc.MIS, dict(n_nodes=6, n_edges=8), B), None, unsplit, 13, min_episodes=2 * B)
    print(trips, queues)
    assert max(queues) == B and min(queues) == 0, queues
    if B > 4096:
        assert max(queues) > max(trips), (queues, trips)


def test_engine_with_spares_is_unchanged_by_the_split(unsplit):
    make = rc.uniform(_ge(), "cuda", rc.SP, dict(n_nodes=10, n_edges=20), 200, prefetch=2)
    rc.check_same_rollout(make, None, unsplit, 25, min_episodes=200)


def test_two_class_engine_is_unchanged_by_the_split(unsplit):
    make = rc.ragged(_ge(), "cuda", rc.SP, [(120, 6, 9), (80, 10, 20)], {})
    rc.check_same_rollout(make, None, unsplit, 25, min_episodes=200)


def test_split_build_matches_the_oracle():
    print(rc.check_split_vs_oracle(_ge(), "cuda", None, dict(n_nodes=10, n_edges=20), 200, 40))


def test_split_build_matches_the_oracle_with_a_non_empty_fallback_list():
    """the deep geometry of test_gpu_priority_roles: the slots the walk items hand to the list launch are advanced exactly once"""
    from test_gpu_priority_roles import DEEP
    st = rc.check_split_vs_oracle(_ge(), "cuda", None, DEEP, 200, 40)
    print(st)
    assert sum(1 for c in st["listed"] if c > 0) >= 10, st["listed"]
