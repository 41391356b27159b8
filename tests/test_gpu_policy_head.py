"""GPU (MI355X): the masked categorical policy head of libgraphenvs_hip.so -- ge_k_policy_head<RAGGED, MODE> behind
sample_actions / evaluate_actions / step_policy -- against the float64 reference and the exact anchors of tests/policy_head_check.py.
B = 300: the rows of two 256-thread workgroups and more, the last one partial; 260 (130) slots for the rows of 2 048 actions and up."""
import pytest

import policy_head_check as pc

pytestmark = pytest.mark.gpu


def _ge():
    import graphenvs_amd as ge
    return ge


@pytest.mark.parametrize("env_id,kw,B,B_cpu", pc.CASES)
def test_policy_head_rows(env_id, kw, B, B_cpu):
    pc.check_uniform(_ge(), "cuda", None, env_id, kw, B)


@pytest.mark.parametrize("env_id,sizes,prefetch", pc.RAGGED)
def test_policy_head_multi_class(env_id, sizes, prefetch):
    pc.check_ragged(_ge(), "cuda", None, env_id, sizes, prefetch)


def test_policy_head_frozen_slots():
    pc.check_frozen(_ge(), "cuda", None, B=300)


def test_step_policy_equals_sample_then_step_distribution_center():
    """DistributionCenter, n <= 64: the coverage-range kernel sits between the policy and the step"""
    ge = _ge()
    make = lambda: ge.VectorGraphEnv(pc._DC, 300, n_nodes=64, n_edges=192, seed_stride=pc.STRIDE, env_index_base=pc.BASE, device="cuda")
    pc.check_step_policy_equals_sample_then_step(ge, "cuda", None, make)


@pytest.mark.parametrize("prefetch", [0, 4])
def test_step_policy_equals_sample_then_step_multi_class(prefetch):
    ge = _ge()
    make = lambda: ge.RaggedVectorEnv(pc._SP, [(70, 12, 30), (130, 64, 192), (100, 100, 300)], seed_stride=pc.STRIDE, env_index_base=pc.BASE,
                                      prefetch=prefetch, device="cuda")
    pc.check_step_policy_equals_sample_then_step(ge, "cuda", None, make)


def test_two_shards_equal_one_engine():
    ge = _ge()
    kw = dict(n_nodes=64, n_edges=192, prefetch=0, device="cuda")
    one = ge.VectorGraphEnv(pc._SP, 300, **kw)
    two = ge.make_vec(pc._SP, 300, shards=2, **kw)
    assert isinstance(two, ge.ShardedVectorEnv) and len(two.members) == 2
    pc.check_shards_equal_one_engine(one, two, "cuda")


def test_policy_head_errors():
    pc.check_errors(_ge(), "cuda", None)
