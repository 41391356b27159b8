"""Independent engines in flight together on one GPU: the process-wide pool of HIP streams that run beside one another, the fork
and join of those streams around a call, and ``MixedVectorEnv`` -- several engines (other env ids, other geometries, or the shards
of one batch: graphenvs_amd.sharded) behind one reset / step / rollout, every member on a stream of its own."""
import contextlib
import os

import torch


@contextlib.contextmanager
def forked(device, streams):
    """Fork `streams` from the current stream of `device` and join them back: every side stream waits for what the current stream
    holds so far, the body queues its work on them, and on the way out the current stream waits for all of them -- also when the
    body raises, so that whoever handles the exception (a read, close()) is ordered behind launches already queued."""
    cur = torch.cuda.current_stream(device)
    fork = cur.record_event()
    for st in streams:
        st.wait_event(fork)
    try:
        yield cur
    finally:
        for st in streams:
            cur.wait_stream(st)


_STREAMS = {}


def _runs_beside(a, b, device):
    """do kernels on streams a and b overlap?  The runtime maps streams onto a handful of hardware queues, and two streams on one
    queue run one behind the other.  Probe: a spin kernel on each, timed together against one alone."""
    spin = getattr(torch.cuda, "_sleep", None)
    if spin is None:
        return True
    cycles = 400000  # ~0.2 ms
    def timed(streams):
        torch.cuda.synchronize(device)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(torch.cuda.current_stream(device))
        with forked(device, streams) as cur:
            for st in streams:
                with torch.cuda.stream(st):
                    spin(cycles)
        t1.record(cur)
        torch.cuda.synchronize(device)
        return t0.elapsed_time(t1)
    timed([a]); one = min(timed([a]) for _ in range(3)); both = min(timed([a, b]) for _ in range(3))
    return both < 1.5 * one


def _member_streams(device, want):
    """up to `want` streams of the process (cached: every MixedVectorEnv uses the same ones) that run BESIDE one another -- a fresh
    stream that shares a hardware queue with one already chosen is set aside and the next is tried; when eight in a row fail the
    device has no queue left and the list ends there (profiles/r04_shards.txt: two shards on one queue 212 M env-steps/s instead of
    353 M; five shards on a device with four queues 166 M)"""
    dev = torch.device(device)
    have = _STREAMS.setdefault(str(dev), [])
    aside = _STREAMS.setdefault(str(dev) + " aside", [])
    full = _STREAMS.setdefault(str(dev) + " full", [False])
    while len(have) < want and not full[0]:
        for _ in range(8):
            cand = torch.cuda.Stream(device=dev)
            if all(_runs_beside(e, cand, dev) for e in have):
                have.append(cand)
                break
            aside.append(cand)  # (kept alive: a freed stream's queue slot would be handed out again)
        else:
            full[0] = True
    return have[:want]


class MixedVectorEnv:
    """Several env ids side by side (each a RaggedVectorEnv or VectorGraphEnv); step takes one action tensor per
    member.  Observation widths differ between ids (utils.get_env_info), so each member keeps its own PyG view.

    The members are independent engines, so on the GPU every call fans out over one HIP stream per member and joins on the caller's
    stream before it returns (``concurrent=False``: one after the other on the caller's stream): the regeneration kernels of a
    member with large graphs hold a workgroup per CU for hundreds of microseconds, and the other members' launches fill the rest
    of the chip meanwhile.  Results do not depend on it -- nothing is shared between members."""

    def __init__(self, members, concurrent=True):
        self.members = list(members)
        self.num_envs = sum(m.num_envs for m in self.members)
        dev = getattr(self.members[0], "device", None)
        self._cuda = concurrent and dev is not None and torch.device(dev).type == "cuda" and len(self.members) > 1
        # member k on a stream of its own -- the same streams for every MixedVectorEnv of the process, chosen so that they run beside one
        # another (_member_streams); with fewer such streams than members, members share them round-robin
        if self._cuda:
            pool = _member_streams(self.members[0].device, len(self.members))
            self._streams = [pool[k % len(pool)] for k in range(len(self.members))]
            self.concurrent_streams = len(pool)
        else:
            self._streams, self.concurrent_streams = None, 1

    def _forked(self):
        """the members' streams between a fork from and a join on the current stream (the join also on an exception)"""
        return forked(self.members[0].device, self._streams)

    def _each(self, fn, args=None):
        """fn(member[, arg]) for every member: on the member's own stream between a fork from and a join on the current stream"""
        args = [None] * len(self.members) if args is None else list(args)
        call = lambda m, a: fn(m) if a is None else fn(m, a)
        if not self._cuda:
            return [call(m, a) for m, a in zip(self.members, args)]
        outs = []
        with self._forked() as cur:
            for m, a, st in zip(self.members, args, self._streams):
                with torch.cuda.stream(st):
                    outs.append(call(m, a))
        # tensors a member allocated inside its call (sampled actions, copy_outputs clones) belong to the side stream's pool: tell the
        # caching allocator that the caller's stream uses them too, or a free followed by a direct call on a member could reuse the
        # memory while the caller's stream still reads it
        def mark(v):
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(cur)
            elif isinstance(v, dict):
                for x in v.values():
                    mark(x)
            elif isinstance(v, (tuple, list)):
                for x in v:
                    mark(x)
            elif hasattr(v, "__dict__") and not callable(v):
                for x in vars(v).values():
                    mark(x)
        mark(outs)
        return outs

    def reset(self, seed=0):
        outs = self._each(lambda m: m.reset(seed=seed))
        return [o for o, _ in outs], [i for _, i in outs]

    def step(self, actions):
        outs = self._each(lambda m, a: m.step(a), actions)
        return tuple(list(col) for col in zip(*outs))

    def sample_random_actions(self, policy_seed=0):
        return self._each(lambda m: m.sample_random_actions(policy_seed))

    def sample_actions(self, logits, policy_seed=0, greedy=False, temperature=1.0):
        """EngineHandle.sample_actions of every member: one logits tensor (float32, bfloat16 or float16) per member in, one
        (actions, logp, entropy) per member out; one temperature for all"""
        return self._each(lambda m, x: m.sample_actions(x, policy_seed, greedy, temperature=temperature), logits)

    def evaluate_actions(self, logits, actions, mask, temperature=1.0):
        """EngineHandle.evaluate_actions of every member: one (logp, entropy) per member"""
        return self._each(lambda m, a: m.evaluate_actions(*a, temperature=temperature), list(zip(logits, actions, mask)))

    def step_policy(self, logits, policy_seed=0, greedy=False, temperature=1.0):
        """EngineHandle.step_policy of every member, returned like step(): one list per element of the step tuple"""
        outs = self._each(lambda m, x: m.step_policy(x, policy_seed, greedy, temperature=temperature), logits)
        return tuple(list(col) for col in zip(*outs))

    def random_rollout(self, n_steps, policy_seed=0):
        """n_steps fused (device policy + step + autoreset) vector steps of every member.  The members are independent engines and
        nothing is read in between, so the streams are forked ONCE, the launches of the members alternate step by step (the host
        enqueues far ahead of the GPU: a member enqueued whole would run alone until the next one's launches arrive) and the caller's
        stream joins ONCE at the end -- no event between streams per step, and no member waits for the regeneration round of another."""
        n_steps = int(n_steps)
        if not self._cuda:
            for m in self.members:
                m.random_rollout(n_steps, policy_seed)
            return
        chunk = max(1, int(os.environ.get("GE_ROLLOUT_CHUNK", "4")))  # steps a member enqueues before the next member's turn (1 .. 8 measured alike; fewer host calls)
        with self._forked():
            for s0 in range(0, n_steps, chunk):
                for m, st in zip(self.members, self._streams):
                    with torch.cuda.stream(st):
                        m.random_rollout(min(chunk, n_steps - s0), policy_seed)

    def close(self):
        for m in self.members:
            m.close()
