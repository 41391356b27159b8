"""CPU: the gradient of the masked categorical policy head (ge_k_policy_grad / ge_policy_backward behind the autograd path of
evaluate_actions) compiled for the sanitizer harness (tests/emu) -- the bodies of tests/policy_grad_check.py on the cases and slot
counts of tests/test_policy_head.py.  The GPU runs the same bodies in tests/test_gpu_policy_grad.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402
import policy_grad_check as gc  # noqa: E402
import policy_head_check as pc  # noqa: E402

import graphenvs_amd as ge  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return build_emu.load()


@pytest.mark.parametrize("A", gc.YARDSTICK_A)
def test_closed_form_equals_float64_autograd(A):
    gc.yardstick(A)


@pytest.mark.parametrize("env_id,kw,B_gpu,B", pc.CASES)
def test_policy_grad_rows(emu, env_id, kw, B_gpu, B):
    gc.check_uniform(ge, "cpu", emu, env_id, kw, B)


def _shrunk(sizes):
    """the multi-class cases with an eighth of the slots: 9 / 17 / 13 -- classes still share waves and workgroups"""
    return [((e[0] + 7) // 8,) + tuple(e[1:]) for e in sizes]


@pytest.mark.parametrize("env_id,sizes,prefetch", pc.RAGGED)
def test_policy_grad_multi_class(emu, env_id, sizes, prefetch):
    gc.check_ragged(ge, "cpu", emu, env_id, _shrunk(sizes), prefetch)


def test_two_engines_over_the_halves_equal_one(emu):
    B, kw = 70, dict(n_nodes=12, n_edges=30, device="cpu", _library=emu)
    one = ge.VectorGraphEnv(pc._SP, B, **kw)
    halves = [ge.VectorGraphEnv(pc._SP, B // 2, env_index_base=k * (B // 2), seed_stride=B, **kw) for k in range(2)]
    gc.check_shards_equal_one_engine(one, ge.MixedVectorEnv(halves), "cpu")


def test_policy_grad_host_behaviour(emu):
    gc.check_host(ge, "cpu", emu)


def test_policy_grad_end_to_end(emu):
    gc.check_end_to_end(ge, "cpu", emu)
