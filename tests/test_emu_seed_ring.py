"""CPU harness (tests/emu): the generator-state ring against CPython's and numpy's own seeders, and the split seeding
(GE_SEED_SPLIT, ge_reset.h / ge_features.h) against a -DGE_SEED_SPLIT=0 build of the same sources, slab by slab.  The bodies
and the shapes are tests/seed_ring_check.py's; tests/test_gpu_seed_ring.py runs them on the MI355X."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402
import seed_ring_check as rc  # noqa: E402

import graphenvs_amd as ge  # noqa: E402

# the harness runs a slot's 1 869 seeding steps and its graph on one CPU thread: the batches of 70 here (a queue of 0 and of 70, one
# more than a wave of seeding items, in the MaxIndependentSet case), the batches of 200 on the GPU
SMALL = [c for c in rc.RING_CASES if c[2] == 70]
SMALL_IDS = [i for c, i in zip(rc.RING_CASES, rc.RING_IDS) if c[2] == 70]


@pytest.fixture(scope="module")
def split():
    return build_emu.load()


@pytest.fixture(scope="module")
def unsplit():
    return build_emu.load(extra=["-DGE_SEED_SPLIT=0"], out=os.path.join(os.path.dirname(build_emu.OUT), "libgraphenvs_emu_unsplit.so"))


@pytest.fixture(scope="module")
def libs(split, unsplit):
    return dict(split=split, unsplit=unsplit)


@pytest.mark.parametrize("build", ["split", "unsplit"])
@pytest.mark.parametrize("env_id,kw,B,expect", SMALL, ids=SMALL_IDS)
def test_emulated_ring_entries_equal_cpython_and_numpy_states(libs, build, env_id, kw, B, expect):
    print(rc.check_ring(ge, "cpu", libs[build], env_id, kw, B, expect))


@pytest.mark.parametrize("env_id,kw,B,expect", SMALL[:2], ids=SMALL_IDS[:2])
def test_emulated_split_build_leaves_the_slabs_of_the_unsplit_build(split, unsplit, env_id, kw, B, expect):
    queues = rc.check_same_rollout(rc.uniform(ge, "cpu", env_id, kw, B), split, unsplit, 10, min_episodes=B)
    assert any(q % 64 for q in queues), queues


def test_emulated_engine_with_spares_is_unchanged_by_the_split(split, unsplit):
    make = rc.uniform(ge, "cpu", rc.SP, dict(n_nodes=10, n_edges=20), 70, prefetch=2)
    rc.check_same_rollout(make, split, unsplit, 10, min_episodes=70)


def test_emulated_two_class_engine_is_unchanged_by_the_split(split, unsplit):
    make = rc.ragged(ge, "cpu", rc.SP, [(40, 6, 9), (30, 10, 20)], {})
    rc.check_same_rollout(make, split, unsplit, 10, min_episodes=70)


def test_emulated_split_build_matches_the_oracle(split):
    print(rc.check_split_vs_oracle(ge, "cpu", split, dict(n_nodes=10, n_edges=20), 70, 12))


def test_emulated_split_build_matches_the_oracle_with_a_non_empty_fallback_list(split):
    """the deep geometry of test_gpu_priority_roles: the slots the walk items hand to the list launch are advanced exactly once"""
    st = rc.check_split_vs_oracle(ge, "cpu", split, dict(n_nodes=28, n_edges=32), 48, 16)
    print(st)
    assert sum(1 for c in st["listed"] if c > 0) >= 2, st["listed"]
