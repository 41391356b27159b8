"""Bodies shared by the CPU harness (tests/test_emu_f64_planes.py) and the GPU tests (tests/test_gpu_f64_planes.py): the level-3
path counts of the n <= 64 feature kernel's forward Brandes pull taken from bit planes of the level-2 counts (ge_features.h,
ge_f64_walk_env, GE_F64_PLANES) against a -DGE_F64_PLANES=0 build of the same sources.

The planes are exact, so nothing here has a tolerance: the comparison is f64_shortcuts_check.check_shortcuts -- after reset(seed)
and after each random_rollout(1) step the x slab has the BYTES of the baseline's, every other slab is equal, work_count is equal and
work_list is the same set, and a sample of slots equals the C oracle.

What a shape is here for is asserted, not assumed: the BFS levels and the level-2 counts of the compared slots are recomputed in
pure Python from the engine's own edge_index slab, after the reset and after every step, and classified per WAVE-ROUND -- the eight
searches s = 8 g .. 8 g + 7 that one wave of a walk item holds at a time, the unit the kernel's gate decides for (a source s >= n
does not exist: a search without levels).  With Dw the deepest search of the wave-round and mx its largest level-2 count:
    third   Dw >= 3 and 4 <= mx <= 7: the gate is open and the third plane is in use
    second  Dw >= 3 and mx <= 3: the gate is open, the third plane is empty
    closed  Dw >= 3 and mx >= 8: the wave-round keeps the pull for level 3
    mixed   a slot with a closed wave-round and an open one (mx <= 7, Dw >= 3): both paths meet in one betweenness sum
    ragged  Dw >= 3 and a search of the wave-round without a level 3 (shallower, or a source that does not exist)
    uneven  Dw >= 3 and a search of the wave-round that exists and ends above level Dw
    high    an open wave-round with a node >= 32 in level 2: the high word of a plane
    none    no wave-round of any compared slot has a level 3 (every slot is looked at)"""
import numpy as np

import f64_shortcuts_check as sc

SP = sc.SP
VARIANTS = dict(base=["-DGE_F64_PLANES=0"])  # product: no flag (the switch defaults to 1)

# (id, n, m, what the comparison must have shown (f64_shortcuts_check.expect), wave-round classes that must have occurred)
SHAPES = [
    ("n64-m192", 64, 192, dict(unlisted=True), ("third", "high")),             # the workload's own graph family
    ("n64-m400", 64, 400, dict(unlisted=True), ("third", "closed", "mixed")),  # gate open and closed inside one slot
    ("n40-m200", 40, 200, dict(unlisted=True), ("third", "closed", "mixed", "ragged")),  # the same mix; sources 40 .. 63 do not exist
    ("n64-m100", 64, 100, dict(unlisted=True), ("second", "uneven")),          # sparse: counts 1 .. 3, searches of different depth in a wave
                                                                               # (none as shallow as 2: the shallowest search of 2 400
                                                                               # wave-rounds of connected G(64, 100) has depth 4, so a search
                                                                               # without a level 3 is left to the two shapes with n < 64)
    ("n33-m70", 33, 70, dict(unlisted=True), ("third", "high", "ragged")),     # n no multiple of 8; a plane's high word holds node 32 alone
    ("n28-m32", 28, 32, dict(listed=True), ()),                                # deep slots: no plane path, the lists must match
    ("n8-m28", 8, 28, dict(unlisted=True), ("none",)),                         # complete: no level 2
    ("n5-m7", 5, 7, dict(unlisted=True), ("none",)),                           # diameter <= 2: no level 3
]


def _levels(adj, s):
    lv, seen = [1 << s], 1 << s
    while True:
        nxt, cur = 0, lv[-1]
        while cur:
            low = cur & -cur
            nxt |= adj[low.bit_length() - 1]
            cur ^= low
        nxt &= ~seen
        if not nxt:
            return lv
        seen |= nxt
        lv.append(nxt)


def classify(n, links):
    """the classes of the slot's wave-rounds (module docstring); links: [E, 2] local node ids of the slot"""
    adj = [0] * n
    for a, b in np.asarray(links).tolist():
        adj[a] |= 1 << b
        adj[b] |= 1 << a
    seen, opened, closed = set(), False, False
    for base in range(0, n, 8):
        depth, mx, high = [], 0, False
        for s in range(base, base + 8):
            lv = _levels(adj, s) if s < n else [0]
            depth.append(len(lv) - 1)
            if len(lv) > 2:
                high |= (lv[2] >> 32) != 0
                cur = lv[2]
                while cur:
                    low = cur & -cur
                    mx = max(mx, bin(adj[low.bit_length() - 1] & lv[1]).count("1"))
                    cur ^= low
        if max(depth) < 3:
            continue
        seen.add("level3")
        seen.add("third" if 4 <= mx <= 7 else "second" if mx <= 3 else "closed")
        opened, closed = opened or mx <= 7, closed or mx >= 8
        if min(depth) < 3:
            seen.add("ragged")
        if min(depth[:n - base]) < max(depth):
            seen.add("uneven")
        if high and mx <= 7:
            seen.add("high")
    if opened and closed:
        seen.add("mixed")
    return seen


class _Recorded:
    """a fused_check engine that keeps the local edge lists of its slots after the reset and after every step"""

    def __init__(self, eng):
        self._eng, self.snapshots = eng, []
        self._snap()

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def _snap(self):
        self._eng.slabs()  # (waits for the engine's stream)
        links = self._eng.env.edge_links()
        rows = [row for cl in (links if isinstance(links, (list, tuple)) else [links]) for row in cl.cpu().numpy()]
        self.snapshots.append(rows)

    def fused(self, ps):
        self._eng.fused(ps)
        self._snap()


def coverage(rec, want):
    """the wave-round classes of the engine's slots over all snapshots; stops at the first slot that completes `want` ("none": never)"""
    ns = [kw["n_nodes"] for kw in rec.oracle_kwargs()]
    seen, last = set(), [None] * len(ns)
    for rows in rec.snapshots:
        for i, links in enumerate(rows):
            if last[i] is not None and np.array_equal(last[i], links):
                continue  # the slot was not regenerated
            last[i] = links
            seen |= classify(ns[i], links)
            if "none" not in want and set(want) <= seen:
                return seen
    if "level3" not in seen:
        seen.add("none")
    return seen


def check_planes(make, libs, env_id, K, sample, cover):
    """f64_shortcuts_check.check_shortcuts on the two builds, and the wave-round classes of the product engine's slots (`cover`: the
    classes looked for).  Returns check_shortcuts' record with the classes seen under "cover"."""
    recorded = []

    def make_recorded(lib):
        eng = make(lib)
        if lib is libs["product"] and not recorded:
            eng = _Recorded(eng)
            recorded.append(eng)
        return eng

    st = sc.check_shortcuts(make_recorded, libs, env_id, K, sample)
    st["cover"] = sorted(coverage(recorded[0], cover))
    return st


def expect(st, want, cover):
    sc.expect(st, want)
    missing = [c for c in cover if c not in st["cover"]]
    assert not missing, ("wave-round classes the shape is here for did not occur", missing, st)
