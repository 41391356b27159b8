"""GPU (MI355X): the kernels ge_random_rollout launches -- the device policy fused into the step kernel -- against the CPU oracle
and against an unfused twin engine (tests/fused_check.py).  bench.py times these kernels and random_rollout() users run them; every
other oracle comparison of the suite goes through sample_random_actions() + step(), i.e. the unfused instantiations.

The engine is driven only by random_rollout(1, policy_seed) with record_actions=True; seeds 2**32 - 40 + 11 + slot (they wrap inside
the batch), stride 7919, policy seed 77.  B = 300: two step workgroups, the second partial (44 slots).  The mask rows run from one
word (path64, node actions up to 64 nodes) over 2 / 4 / 5 / 9 / 10 words to 32 (the quad sampler's last chunk) and 33 (the first
row it refuses); every case must draw from every word of its rows."""
import pytest

import fused_check as fc

pytestmark = pytest.mark.gpu


def _ge():
    import graphenvs_amd as ge
    return ge


SP64 = ("ShortestPath-v0", dict(n_nodes=64, n_edges=192, is_eval_env=True))
MC100 = dict(n_nodes=100, n_edges=300, n_dests=6)

# (env id, kwargs, B, K, autoreset, prefetch, episodes required)
CASES = [
    pytest.param(*SP64, 300, 40, True, 0, 1, id="path64"),
    pytest.param(*SP64, 300, 40, True, 3, 1, id="path64-spares-headline"),
    pytest.param("LongestPath-v0", dict(n_nodes=20, n_edges=50, parenting=0), 300, 40, True, 0, 1, id="path64-open-mask"),
    # next-step autoreset: a swap is consumed at the start of the next step
    pytest.param("LongestPath-v0", dict(n_nodes=20, n_edges=50, parenting=1), 300, 40, "next_step", 2, 1, id="path64-next-step-spares"),
    # quad sampler: A = 200, AW = 4 -- one chunk, all four lanes, ragged last word
    pytest.param("SteinerTree-v0", dict(n_nodes=40, n_edges=100, n_dests=5), 300, 40, True, 0, 1, id="quad-aw4"),
    # A = 288, AW = 5: the second chunk holds one lane's word (few episodes end within 40 steps)
    pytest.param("SteinerTree-v0", dict(n_nodes=64, n_edges=144, n_dests=6), 300, 40, True, 0, 1, id="quad-aw5"),
    pytest.param("MulticastRouting-v0", dict(MC100, parenting=2), 300, 40, True, 0, 1, id="quad-aw10-w2"),
    pytest.param("MulticastRouting-v0", dict(MC100, parenting=4, is_eval_env=True), 300, 40, "next_step", 0, 1, id="quad-aw10-w2-next-step"),
    # BASELINE config 4's geometry, AW = 32: all eight chunks, jsel == 7 (no episode ends within 40 steps)
    pytest.param("SteinerTree-v0", dict(n_nodes=256, n_edges=1024, n_dests=8), 260, 40, True, 0, 0, id="quad-aw32-limit"),
    # AW = 33: the first row the quad kernel refuses -- ge_k_step<.., true, ..> and the AW > 8 loop of ge_policy_pick
    pytest.param("SteinerTree-v0", dict(n_nodes=260, n_edges=1040, n_dests=8), 260, 30, True, 0, 0, id="edge-aw33-thread-per-slot"),
    # thread-per-slot fused kernel, node actions
    pytest.param("TSP-v0", dict(n_nodes=20, n_edges=60, parenting=1), 300, 40, True, 0, 1, id="tsp-p1"),
    pytest.param("TSP-v0", dict(n_nodes=14, n_edges=40, parenting=2), 300, 40, True, 0, 1, id="tsp-p2-prune1"),
    pytest.param("LongestPath-v0", dict(n_nodes=100, n_edges=300, parenting=2), 300, 40, True, 0, 1, id="lp-p2-w2"),
    pytest.param("DensestSubgraph-v0", dict(n_nodes=64, n_edges=192, parenting=1), 300, 40, True, 0, 1, id="densest"),
    # (an episode of MaxIndependentSet lasts n steps whatever is drawn: 80 steps, so that every slot finishes once)
    pytest.param("MaxIndependentSet-v0", dict(n_nodes=70, n_edges=200), 300, 80, True, 0, 1, id="mis-w2"),
    pytest.param("PerishableProductDelivery-v0", dict(n_nodes=20, n_edges=50, parenting=1), 300, 120, True, 0, 1, id="perishable"),
    pytest.param("DistributionCenter-v0", dict(n_nodes=100, n_edges=260, weighted=False), 300, 40, True, 0, 1, id="dc-w2"),
    # above 512 nodes: PRUNE 2, node sets in prune_scratch (no walk over 560 nodes ends within 20 steps)
    pytest.param("LongestPath-v0", dict(n_nodes=560, n_edges=1500, parenting=2), 6, 20, True, 0, 0, id="lp-p2-prune2"),
    *fc.SMALL_CASES,
]


@pytest.mark.parametrize("env_id,kw,B,K,autoreset,prefetch,episodes", CASES)
def test_fused_rollout_matches_oracle_and_unfused_twin(env_id, kw, B, K, autoreset, prefetch, episodes):
    import oracle
    st = fc.check_fused_vs_oracle(_ge(), oracle, "cuda", None, env_id, kw, B, K, autoreset=autoreset, prefetch=prefetch, min_episodes=episodes)
    print(env_id, kw, st)
    if kw["n_nodes"] == 256:
        assert sum(st["word_draws"][28:]) > 0  # the quad sampler's last chunk


def test_rollout_without_a_fused_kernel_goes_through_the_actions_scratch():
    """DistributionCenter, n <= 64: policy kernel -> coverage range kernel -> step kernel; actions_out stays unset by design, the
    picks are in the actions scratch"""
    import oracle
    st = fc.check_fused_vs_oracle(_ge(), oracle, "cuda", None, "DistributionCenter-v0", dict(n_nodes=64, n_edges=192), 300, 40,
                                  scratch_actions=True)
    print(st)


@pytest.mark.parametrize("env_id,kw", [("ShortestPath-v0", dict(n_nodes=10, n_edges=20)),
                                       ("SteinerTree-v0", dict(n_nodes=40, n_edges=100, n_dests=5)),
                                       ("MaxIndependentSet-v0", dict(n_nodes=20, n_edges=40))])
def test_fused_rollout_records_minus_one_for_frozen_slots(env_id, kw):
    """autoreset off: until every slot has finished and two steps beyond; a finished slot records -1, returns reward 0 and
    terminated 0, and none of its slabs change"""
    import oracle
    st = fc.check_fused_vs_oracle(_ge(), oracle, "cuda", None, env_id, kw, 300, 4 * kw["n_nodes"], autoreset=False)
    print(env_id, kw, st)
    assert st["minus_ones"] >= 2 * 300 and st["episodes"] == 300


RAGGED = [
    # slots of three classes share a workgroup; n <= 64 and n > 64
    ("ShortestPath-v0", [(70, 12, 30), (130, 64, 192), (100, 100, 300)], {}),
    # the quad kernel stages rows of AW 1 / 5 / 10 with the widest stride; the last class is MST
    ("SteinerTree-v0", [(70, 12, 30, dict(n_dests=3)), (130, 64, 144, dict(n_dests=6)), (100, 100, 300, dict(n_dests=99))], {}),
    ("TSP-v0", [(150, 14, 40), (150, 20, 60)], dict(parenting=2)),
]


@pytest.mark.parametrize("prefetch", [0, 4])
@pytest.mark.parametrize("env_id,sizes,common", RAGGED)
def test_fused_rollout_of_the_multi_class_engine_matches_oracle_and_unfused_twin(env_id, sizes, common, prefetch):
    import oracle
    st = fc.check_fused_ragged_vs_oracle(_ge(), oracle, "cuda", None, env_id, sizes, common, 40, prefetch=prefetch)
    print(env_id, sizes, st)


@pytest.mark.parametrize("env_id,kw", [SP64[:1] + (dict(n_nodes=64, n_edges=192),),
                                       ("SteinerTree-v0", dict(n_nodes=40, n_edges=100))])
def test_timed_rollout_leaves_what_random_rollout_leaves(env_id, kw):
    fc.check_timed_rollout_equals_random_rollout(_ge(), "cuda", None, env_id, kw)


def test_sharded_timed_rollout_leaves_what_random_rollout_leaves():
    fc.check_sharded_timed_rollout_equals_random_rollout(_ge())
