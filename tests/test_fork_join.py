"""CPU: the fork/join of the member streams (graphenvs_amd.mixed.forked) joins on the error path too.  torch.cuda.current_stream and
torch.cuda.stream are replaced by recording stand-ins; a member that raises in the middle of a fan-out must leave the caller's stream
joined with every side stream -- launches queued on them before the raise are still in flight when the exception is handled."""
import contextlib

import pytest
import torch

from graphenvs_amd import mixed
from graphenvs_amd.sharded import ShardedVectorEnv


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def record_event(self):
        self.log.append(("record_event", self.name))
        return "fork"

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev))

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))


class _Member:
    num_envs, device = 4, "cuda"

    def __init__(self, k, log, bad):
        self.k, self.log, self.bad = k, log, bad

    def _do(self, what):
        self.log.append((what, self.k))
        if self.bad:
            self.log.append(("raise", self.k))
            raise RuntimeError(f"member {self.k}: launch failed")

    def step(self, a):
        self._do("step")

    def random_rollout(self, n_steps, policy_seed=0):
        self._do("random_rollout")

    def timed_rollout(self, n_steps, policy_seed=0):
        self._do("timed_rollout")
        return dict(step_ms=0.0, reset_ms=0.0, policy_ms=0.0)


@pytest.fixture
def fan(monkeypatch):
    """(log, make): make(cls) is a `cls` over three stub members, the second of which raises, fanned out over three fake streams"""
    log = []
    cur = _Stream("cur", log)
    monkeypatch.setattr(mixed.torch.cuda, "current_stream", lambda device=None: cur)
    monkeypatch.setattr(mixed.torch.cuda, "stream", lambda st: contextlib.nullcontext())

    def make(cls):
        env = cls.__new__(cls)
        mixed.MixedVectorEnv.__init__(env, [_Member(k, log, bad=(k == 1)) for k in range(3)], concurrent=False)
        env._cuda, env._streams, env.device = True, [_Stream(f"side{k}", log) for k in range(3)], "cuda"
        return env
    return log, make


def _joined_after_the_raise(log):
    assert log[0] == ("record_event", "cur")
    assert log[1:4] == [("wait_event", f"side{k}", "fork") for k in range(3)]
    after = log[log.index(("raise", 1)) + 1:]
    assert after == [("wait_stream", "cur", f"side{k}") for k in range(3)], log
    assert sum(e[0] == "wait_stream" for e in log) == 3


def test_step_joins_every_side_stream_when_a_member_raises(fan):
    log, make = fan
    env = make(mixed.MixedVectorEnv)
    with pytest.raises(RuntimeError, match="member 1"):
        env.step(["a0", "a1", "a2"])
    assert ("step", 0) in log and ("step", 2) not in log
    _joined_after_the_raise(log)


def test_random_rollout_joins_every_side_stream_when_a_member_raises(fan):
    log, make = fan
    with pytest.raises(RuntimeError, match="member 1"):
        make(mixed.MixedVectorEnv).random_rollout(8)
    _joined_after_the_raise(log)


def test_sharded_timed_rollout_joins_every_side_stream_when_a_member_raises(fan):
    log, make = fan
    with pytest.raises(RuntimeError, match="member 1"):
        make(ShardedVectorEnv).timed_rollout(8)
    assert ("timed_rollout", 0) not in log
    _joined_after_the_raise(log)


def test_a_fan_out_that_succeeds_joins_once(fan):
    log, make = fan
    env = make(mixed.MixedVectorEnv)
    for m in env.members:
        m.bad = False
    env.random_rollout(8)
    assert [e for e in log if e[0] == "random_rollout"] == [("random_rollout", k) for _ in range(2) for k in range(3)]  # GE_ROLLOUT_CHUNK = 4
    assert log[-3:] == [("wait_stream", "cur", f"side{k}") for k in range(3)] and sum(e[0] == "wait_stream" for e in log) == 3
    assert sum(e[0] == "record_event" for e in log) == 1
