"""GPU (MI355X): ge_k_policy_head / ge_k_policy_grad of libgraphenvs_hip.so instantiated for bfloat16 and float16 logits, with a
temperature -- the bodies of tests/policy_dtype_check.py (bit-for-bit identity with the float32 path on x.float() * scale, forward
and gradient) on the slot counts of tests/test_gpu_policy_head.py: 300 / 260 / 130."""
import pytest
import torch

import policy_dtype_check as dc
import policy_head_check as pc

pytestmark = pytest.mark.gpu


def _ge():
    import graphenvs_amd as ge
    return ge


@pytest.mark.parametrize("T", dc.TEMPERATURES)
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("env_id,kw,B,B_cpu", dc.CASES)
def test_policy_dtype_rows(env_id, kw, B, B_cpu, dtype, T):
    dc.check_uniform(_ge(), "cuda", None, env_id, kw, B, dtype, T)


@pytest.mark.parametrize("T", dc.TEMPERATURES)
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("env_id,sizes,prefetch", dc.RAGGED)
def test_policy_dtype_multi_class(env_id, sizes, prefetch, dtype, T):
    dc.check_ragged(_ge(), "cuda", None, env_id, sizes, prefetch, dtype, T)


def test_step_policy_16bit_distribution_center():
    """DistributionCenter, n <= 64: the coverage-range kernel sits between the policy and the step"""
    ge = _ge()
    make = lambda: ge.VectorGraphEnv(pc._DC, 300, n_nodes=64, n_edges=192, seed_stride=pc.STRIDE, env_index_base=pc.BASE, device="cuda")
    dc.check_step_policy(ge, "cuda", make, torch.bfloat16, 0.7)


def test_step_policy_16bit_multi_class():
    ge = _ge()
    make = lambda: ge.RaggedVectorEnv(pc._SP, [(70, 12, 30), (130, 64, 192), (100, 100, 300)], seed_stride=pc.STRIDE, env_index_base=pc.BASE,
                                      device="cuda")
    dc.check_step_policy(ge, "cuda", make, torch.float16, 3.0)


def test_two_shards_equal_one_engine_bf16():
    ge = _ge()
    kw = dict(n_nodes=64, n_edges=192, prefetch=0, device="cuda")
    one = ge.VectorGraphEnv(pc._SP, 300, **kw)
    two = ge.make_vec(pc._SP, 300, shards=2, **kw)
    assert isinstance(two, ge.ShardedVectorEnv) and len(two.members) == 2
    dc.check_halves_equal_one(one, two, "cuda", torch.bfloat16, 0.7)


def test_policy_dtype_errors():
    dc.check_errors(_ge(), "cuda", None)
