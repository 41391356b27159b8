"""Bodies shared by the CPU harness (tests/test_emu_f64_shortcuts.py) and the GPU tests (tests/test_gpu_f64_shortcuts.py): the
shortcut of the n <= 64 feature kernel's forward Brandes pull (ge_features.h, ge_f64_walk_env) -- GE_F64_L2POP, the path counts of
level 2 as popcounts -- against a -DGE_F64_L2POP=0 build of the same sources.

The shortcut is exact, so nothing here has a tolerance: after reset(seed) and after each random_rollout(1) step with same-step
autoreset the x slab of every build has the BYTES of the baseline's, every other slab is equal, work_count is equal and work_list
is the same set (fused_check._same_slabs); and the whole observation of a sample of slots -- its five structural columns among it --
equals the C oracle's, which is stepped with the actions the engine recorded."""
import numpy as np
import torch

import fused_check as fc

SP = "ShortestPath-v0"
VARIANTS = dict(base=["-DGE_F64_L2POP=0"])  # product: no flag (the switch defaults to 1)

# (id, n, m, what the run must have shown).  `listed`: some slot went to the generic kernel's list (deeper than GE_F64_LV = 12
# levels: a connected graph of 28 nodes and 32 edges is a tree with five more edges); `unlisted`: some regeneration left the list empty,
# i.e. the pulls themselves produced what is compared.
SHAPES = [
    ("n64-m192", 64, 192, dict(unlisted=True)),   # the workload's own graph family
    ("n64-m100", 64, 100, dict(unlisted=True)),   # sparse at 64 nodes: both source rounds and both 32-bit halves of the sets on deep,
                                                  # tree-like searches that end at different depths inside a wave.  (m = 70 is not here: a
                                                  # G(64, 70) draw has no isolated node with probability exp(-64 exp(-140 / 64)) ~ 1e-3 and
                                                  # is connected far more rarely still -- the rejection loop of the generator, and of the
                                                  # oracle, does not end in any useful time; at m = 100 that bound is 6 %)
    ("n28-m32", 28, 32, dict(listed=True)),       # tree-like (the deep geometry of test_gpu_priority_roles): slots over GE_F64_LV, the list must match
    ("n64-m600", 64, 600, dict(unlisted=True)),   # level 2 is the last level: I(2) empty, level 1 all internal
    ("n8-m28", 8, 28, dict(unlisted=True)),       # complete: no level 2 at all
    ("n33-m70", 33, 70, dict(unlisted=True)),     # sources that do not exist in the last octets, n no multiple of 8
    ("n12-m13", 12, 13, dict(unlisted=True)),     # deep, small
    ("n5-m7", 5, 7, dict(unlisted=True)),         # the smallest graph the fixtures use
]


def _x_bytes(eng):
    """the bytes of every x slab of the engine (a uniform engine has one, a multi-class engine one per class)"""
    return [(label, v.contiguous().view(torch.uint8)) for label, key, v in eng.slabs() if key == "x" and v is not None]


def _listed(eng):
    return int(eng.out("work_count")[0])


def _compare(engines, where):
    base = engines["base"]
    bs, bx = base.slabs(), _x_bytes(base)
    assert bx, "no x slab"
    for name, e in engines.items():
        if name == "base":
            continue
        fc._same_slabs(e.slabs(), bs, (), (where, name))  # work_count equal, work_list equal as a set, every other slab equal
        for (label, a), (_, b) in zip(_x_bytes(e), bx):
            assert torch.equal(a, b), (where, name, label, "x bytes")
        assert _listed(e) == _listed(base), (where, name)


class _Sample:
    """the C oracle on a sample of slots of the product engine, stepped with the actions the engine recorded"""

    def __init__(self, eng, env_id, slots):
        import oracle
        kws = eng.oracle_kwargs()
        self.slots = slots
        self.seeds = [(fc.S0 + fc.BASE + i) % 2**32 for i in slots]
        self.refs = [oracle.OracleEnv(env_id, **kws[i]) for i in slots]
        for r, s in zip(self.refs, self.seeds):
            r.reset(seed=s)
        self.episodes = 0

    def step(self, actions):
        for j, (i, r) in enumerate(zip(self.slots, self.refs)):
            a = int(actions[i])
            if a < 0:
                continue
            _, _, done, _, _ = r.step(a)
            if done:  # same-step autoreset
                self.seeds[j] = (self.seeds[j] + fc.STRIDE) % 2**32
                r.reset(seed=self.seeds[j])
                self.episodes += 1

    def check(self, eng, where):
        obs = eng.obs()
        for i, r in zip(self.slots, self.refs):
            assert np.array_equal(obs[i], r.obs()), (where, "slot", i, "observation (structural columns) != oracle")


def check_shortcuts(make, libs, env_id, K, sample, policy_seed=77):
    """make(lib) -> a fused_check engine; libs: {"product", "base"} -> library handle (None: the product).
    Returns what the run showed: list lengths after the reset and every step, regenerated slots, oracle episodes of the sample."""
    engines = {name: make(lib) for name, lib in libs.items()}
    assert set(engines) == {"product", "base"}
    prod = engines["product"]
    ref = _Sample(prod, env_id, [i for i in sample if i < prod.B])
    _compare(engines, "reset")
    ref.check(prod, "reset")
    listed = [_listed(prod)]
    episode = lambda e: np.asarray(e.out("episode")).astype(np.int64)
    before, queues = episode(prod), []
    for k in range(K):
        for e in engines.values():
            e.fused(policy_seed)
        _compare(engines, k)
        ref.step(prod.actions())
        ref.check(prod, k)
        after = episode(prod)
        queues.append(int((after - before).sum()))
        before = after
        listed.append(_listed(prod))
    for e in engines.values():
        e.close()
    return dict(listed=listed, queues=queues, sample_episodes=ref.episodes)


def expect(st, want):
    """the case was not vacuous: slots regenerated during the rollout (regen=False: a batch too small to promise that in a few steps
    of 64-node episodes), and the list was (non-)empty where the shape says so"""
    if want.get("regen", True):
        assert sum(st["queues"]) > 0, st
    if want.get("listed"):
        assert max(st["listed"]) > 0, st
    if want.get("unlisted"):  # the reset's launch or a regenerating step whose slots all stayed on the fast path
        assert st["listed"][0] == 0 or any(q > 0 and c == 0 for q, c in zip(st["queues"], st["listed"][1:])), st
