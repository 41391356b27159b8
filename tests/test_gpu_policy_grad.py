"""GPU (MI355X): ge_k_policy_grad<RAGGED> of libgraphenvs_hip.so -- the logits gradient of evaluate_actions -- against the float64
closed form, its band and the exact anchors of tests/policy_grad_check.py, on the cases and slot counts of
tests/test_gpu_policy_head.py."""
import pytest

import policy_grad_check as gc
import policy_head_check as pc

pytestmark = pytest.mark.gpu


def _ge():
    import graphenvs_amd as ge
    return ge


@pytest.mark.parametrize("env_id,kw,B,B_cpu", pc.CASES)
def test_policy_grad_rows(env_id, kw, B, B_cpu):
    gc.check_uniform(_ge(), "cuda", None, env_id, kw, B)


@pytest.mark.parametrize("env_id,sizes,prefetch", pc.RAGGED)
def test_policy_grad_multi_class(env_id, sizes, prefetch):
    gc.check_ragged(_ge(), "cuda", None, env_id, sizes, prefetch)


def test_two_shards_equal_one_engine():
    ge = _ge()
    kw = dict(n_nodes=64, n_edges=192, prefetch=0, device="cuda")
    one = ge.VectorGraphEnv(pc._SP, 300, **kw)
    two = ge.make_vec(pc._SP, 300, shards=2, **kw)
    assert isinstance(two, ge.ShardedVectorEnv) and len(two.members) == 2
    gc.check_shards_equal_one_engine(one, two, "cuda")


def test_policy_grad_host_behaviour():
    gc.check_host(_ge(), "cuda", None)


def test_policy_grad_end_to_end():
    gc.check_end_to_end(_ge(), "cuda", None)
