"""CPU: the masked categorical policy head (graphenvs_amd/csrc/ge_policy.h, ge_policy_sample / ge_policy_evaluate / ge_policy_step)
compiled for the sanitizer harness (tests/emu: UBSan, bounds of every LDS block, divergent-rendezvous detector) -- the cases of
tests/policy_head_check.py at the harness's batch sizes: 70 slots (two waves of rows and a partial one) for rows of up to 200
actions, 3 slots for the rows of 2 048 actions and more.  The GPU runs the same cases in tests/test_gpu_policy_head.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402
import policy_head_check as pc  # noqa: E402

import graphenvs_amd as ge  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return build_emu.load()


@pytest.mark.parametrize("env_id,kw,B_gpu,B", pc.CASES)
def test_policy_head_rows(emu, env_id, kw, B_gpu, B):
    pc.check_uniform(ge, "cpu", emu, env_id, kw, B)


def _shrunk(sizes):
    """the multi-class cases with an eighth of the slots: 9 / 17 / 13 -- classes still share waves and workgroups"""
    return [((e[0] + 7) // 8,) + tuple(e[1:]) for e in sizes]


@pytest.mark.parametrize("env_id,sizes,prefetch", pc.RAGGED)
def test_policy_head_multi_class(emu, env_id, sizes, prefetch):
    pc.check_ragged(ge, "cpu", emu, env_id, _shrunk(sizes), prefetch)


def test_policy_head_frozen_slots(emu):
    pc.check_frozen(ge, "cpu", emu)


def test_step_policy_equals_sample_then_step_distribution_center(emu):
    """DistributionCenter, n <= 64: the coverage-range kernel sits between the policy and the step"""
    make = lambda: ge.VectorGraphEnv(pc._DC, 20, n_nodes=64, n_edges=192, seed_stride=pc.STRIDE, env_index_base=pc.BASE, device="cpu", _library=emu)
    pc.check_step_policy_equals_sample_then_step(ge, "cpu", emu, make)


def test_step_policy_equals_sample_then_step_multi_class(emu):
    make = lambda: ge.RaggedVectorEnv(pc._SP, [(9, 12, 30), (17, 64, 192), (13, 70, 200)], seed_stride=pc.STRIDE, env_index_base=pc.BASE,
                                      device="cpu", _library=emu)
    pc.check_step_policy_equals_sample_then_step(ge, "cpu", emu, make)


def test_step_policy_strict_and_copy_outputs(emu):
    """step_policy goes through step()'s bookkeeping: copy_outputs clones info['action'] / ['logp'] / ['entropy'] too"""
    import torch
    env = ge.VectorGraphEnv(pc._SP, 6, n_nodes=10, n_edges=20, strict=True, copy_outputs=True, device="cpu", _library=emu)
    env.reset(seed=3)
    x = torch.zeros(6, 10)
    out = env.step_policy(x, 5)
    act = out[4]["action"]
    assert act.data_ptr() != env._policy["actions"].data_ptr() and torch.equal(act, env._policy["actions"])
    assert out[1].data_ptr() != env.t["reward"].data_ptr()
    env.close()


def test_two_engines_over_the_halves_equal_one(emu):
    """env_index_base 0 and B / 2: a row's arithmetic and its draw do not depend on the batch it sits in (the halves behind one
    MixedVectorEnv: its sample_actions / evaluate_actions / step_policy, one entry per member)"""
    B, kw = 70, dict(n_nodes=12, n_edges=30, device="cpu", _library=emu)
    one = ge.VectorGraphEnv(pc._SP, B, **kw)
    halves = [ge.VectorGraphEnv(pc._SP, B // 2, env_index_base=k * (B // 2), seed_stride=B, **kw) for k in range(2)]
    pc.check_shards_equal_one_engine(one, ge.MixedVectorEnv(halves), "cpu")


def test_policy_head_errors(emu):
    pc.check_errors(ge, "cpu", emu)
