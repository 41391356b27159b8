"""Bodies shared by the CPU harness (tests/test_emu_seed_ring.py) and the GPU tests (tests/test_gpu_seed_ring.py): the ring of
pre-seeded MT19937 states (ge_buffers.mt_state, GE_SEED_DEPTH entries of {python, numpy} x 624 words per slot) against the real
seeders, and the split seeding (GE_SEED_SPLIT: random.seed's second pass at the head of the feature launch) against the unsplit
build slab by slab.

The ring (ge_reset.h): while a slot runs episode e, seeded s = seed[slot], entry (e + k) mod 3 holds the states of episode e + k,
k = 0, 1, 2 -- entry e was consumed by the regeneration that started the episode and is left as it was seeded; the reset path that
moves the slot to e + 1 refills it with episode e + 3.  So after reset(seed=...) and after every step every entry of every slot is
checked: python == random.Random(s_k).getstate()[1][:624], numpy == np.random.RandomState(s_k).get_state()[1],
s_k = (s + k * seed_stride) mod 2^32.  Seeds, stride and base are fused_check's, so the seeds wrap around 2^32 inside the batch."""
import random

import numpy as np
import torch

import fused_check as fc

DEPTH, MT_N = 3, 624  # GE_SEED_DEPTH, GE_MT_N
MIN_EPISODES = 2 * DEPTH + 1  # every slot goes round its ring twice and once more
SP, MIS = "ShortestPath-v0", "MaxIndependentSet-v0"

# (env id, kwargs, B, what the queue lengths of the run must have shown).  The ShortestPath shapes regenerate a quarter to a third
# of their slots in every step -- the CPU oracle gives, with fused_check's seeds and policy seed 77, queues of 14..32 (n = 6, B = 70),
# 40..87 (n = 6, B = 200), 6..25 (n = 10, B = 70) and 17..58 (n = 10, B = 200): an empty queue there is an event of probability
# ~0.8^70 that no choice of seed buys.  An episode of MaxIndependentSet n = 6 lasts exactly six steps for every slot, so its queue is
# 0 five steps out of six and the whole batch (70: one more than a wave of seeding items and no multiple of 64; 200: more than two
# waves) in the sixth: these two cases are added for the empty queue, the queue of 65 or more and the queue above 128.
RING_CASES = [
    (SP, dict(n_nodes=6, n_edges=9), 70, dict(odd=True)),
    (SP, dict(n_nodes=6, n_edges=9), 200, dict(ge65=True, odd=True)),
    (SP, dict(n_nodes=10, n_edges=20), 70, dict(odd=True)),
    (SP, dict(n_nodes=10, n_edges=20), 200, dict(odd=True)),
    (MIS, dict(n_nodes=6, n_edges=8), 70, dict(zero=True, ge65=True, odd=True)),
    (MIS, dict(n_nodes=6, n_edges=8), 200, dict(zero=True, ge65=True, odd=True, gt128=True)),
]
RING_IDS = ["%s-n%d-B%d" % ("sp" if e == SP else "mis", kw["n_nodes"], B) for e, kw, B, _ in RING_CASES]

_states = {}


def seeded_states(s):
    """[2, 624] uint32: what random.seed(s) and np.random.seed(s) leave, from CPython and numpy themselves"""
    if s not in _states:
        py = np.array(random.Random(s).getstate()[1][:MT_N], dtype=np.uint32)
        npy = np.asarray(np.random.RandomState(s).get_state()[1], dtype=np.uint32)
        assert py.shape == npy.shape == (MT_N,)
        _states[s] = np.stack([py, npy])
    return _states[s]


def _u32(t):
    return fc._np(t).view(np.uint32)


def _check_ring(env, want, first, where):
    """every entry of every slot; `want` [B, 3, 2, 624] is brought up to date for the slots whose episode moved (seeded_states)"""
    env._quiesce()
    B = env.num_envs
    episode, seed = fc._np(env.t["episode"]).astype(np.int64), _u32(env.t["seed"]).astype(np.int64)
    for i in range(B):
        assert seed[i] == (first[i] + episode[i] * fc.STRIDE) % 2**32, (where, i, "seed[] is not the episode's seed")
        for k in range(DEPTH):
            want[i, (episode[i] + k) % DEPTH] = seeded_states(int((seed[i] + k * fc.STRIDE) % 2**32))
    got = _u32(env.t["mt_state"]).reshape(B, DEPTH, 2, MT_N)
    if not np.array_equal(got, want):
        i, j, st, w = [int(v[0]) for v in np.nonzero(got != want)]
        raise AssertionError((where, "slot", i, "episode", int(episode[i]), "entry", j, ("python", "numpy")[st], "word", w,
                              hex(int(got[i, j, st, w])), hex(int(want[i, j, st, w])), "differing words", int((got != want).sum())))
    return episode


def check_ring(ge, device, lib, env_id, kw, B, expect, policy_seed=77, cap=200):
    """reset(seed=S0), then random_rollout(1) until every slot has passed MIN_EPISODES episodes: the ring after the reset and after
    every step.  Returns the queue length of every step (the slots whose episode moved)."""
    env = ge.VectorGraphEnv(env_id, B, seed_stride=fc.STRIDE, env_index_base=fc.BASE, prefetch=0, **fc._extra(device, lib), **kw)
    env.reset(seed=fc.S0)
    first = [(fc.S0 + fc.BASE + i) % 2**32 for i in range(B)]
    assert max(first) > 2**32 - 64 and min(first) < 64  # the seeds wrap inside the batch
    want = np.zeros((B, DEPTH, 2, MT_N), dtype=np.uint32)
    episode = _check_ring(env, want, first, "reset")
    assert not episode.any()
    queues = []
    while episode.min() < MIN_EPISODES:
        assert len(queues) < cap, "slots short of their episodes at the step cap"
        env.random_rollout(1, policy_seed=policy_seed)
        after = _check_ring(env, want, first, len(queues))
        assert ((after - episode) >= 0).all() and ((after - episode) <= 1).all()
        queues.append(int((after - episode).sum()))
        episode = after
    env.check_device_errors()
    env.close()
    seen = dict(zero=min(queues) == 0, ge65=max(queues) >= 65, odd=any(q % 64 for q in queues), gt128=max(queues) > 128)
    for key in expect:
        assert seen[key], (key, queues)
    return queues


# ---- split == unsplit

def seeding_trips(env):
    """(slots the seeding workgroups of the graph launch cover in one trip of their stride loop, the same for the pass-2 workgroups
    of the feature launch): the plan's arithmetic (ge_api.hip, finish_create: GePlan.nseed, nseed2) on the engine's layout"""
    lds = int(env.layout.reset_lds_bytes)
    per_cu = max(1, min(16, 160 * 1024 // lds))
    nseed = (min(256 * per_cu, env.num_envs) + 63) // 64
    return nseed * 64, (nseed * 64 + 255) // 256 * 256


def check_same_rollout(make, lib_a, lib_b, K, policy_seed=77, min_episodes=1):
    """make(lib) -> a fused_check engine (_Uniform / _Ragged); K steps of random_rollout(1) on one engine per library: after the
    reset and after every step EVERY slab is byte-identical (mt_state, seed and episode among them).  Returns the queue lengths."""
    a, b = make(lib_a), make(lib_b)
    fc._same_slabs(a.slabs(), b.slabs(), (), "reset")
    episode = lambda e: np.asarray(e.out("episode")).astype(np.int64)
    before, queues = episode(a), []
    for k in range(K):
        a.fused(policy_seed); b.fused(policy_seed)
        fc._same_slabs(a.slabs(), b.slabs(), (), k)
        after = episode(a)
        queues.append(int((after - before).sum()))
        before = after
    assert int(before.sum()) >= min_episodes, int(before.sum())
    a.close(); b.close()
    return queues


def uniform(ge, device, env_id, kw, B, prefetch=0):
    return lambda lib: fc._Uniform(ge, device, lib, env_id, kw, B, True, prefetch)


def ragged(ge, device, env_id, sizes, common, prefetch=0):
    return lambda lib: fc._Ragged(ge, device, lib, env_id, sizes, common, prefetch)


# ---- parity with the oracle

class _Listed(fc._Uniform):
    """a uniform engine that records the length of the feature fast path's fallback list after every step"""

    def fused(self, ps):
        super().fused(ps)
        self.listed = getattr(self, "listed", []) + [int(self.env.t["work_count"][0])]


def check_split_vs_oracle(ge, device, lib, kw, B, K):
    import oracle
    f, u = _Listed(ge, device, lib, SP, kw, B, True, 0), fc._Uniform(ge, device, lib, SP, kw, B, True, 0)
    st = fc._rollout(oracle, f, u, SP, K, True, 0, 77, B)
    return dict(st, listed=f.listed)
