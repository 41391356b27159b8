"""Trip model of the two Brandes pulls of ge_f64_walk_env (ge_features.h), on the CPU: no GPU, pure Python.

usage: python tools/f64_trip_model.py [--graphs 200] [--n 64] [--m 192] [--seed 1] > profiles/r12_trip_model.txt

Seeded connected G(n, m) graphs (uniform edge sets, redrawn until connected).  A wave holds eight BFS sources (s = 32 r + 8 w + sl),
eight lanes per source; lane o of a source takes the entries k = lo + o + 8 t of a level's stretch of the (level, node) order.  An
OUTER trip is one pass of the `k += 8` loop, which the wave leaves when no lane has an entry; an INNER trip is one pass of the
GE_F64_U = 2 set-bit loop over one 32-bit half of the node's predecessor / successor set.  The wave pays the busiest lane of every
outer trip.  Printed: mean trips per wave and round of both pulls as shipped before round 10, with the level-2 popcount
(GE_F64_L2POP: level 2 has no inner trips), with a dependency pull over the nodes that have a successor only (built, measured and not
shipped, profiles/README.md round 10), with level 3 from bit planes of the level-2 counts (GE_F64_PLANES: level 3 has no inner trips in
a wave-round whose largest level-2 count is at most 7), and with each level sorted by set size on top (not built).  Behind the table:
the forward pull's trips level by level, and the distribution of the largest level-2 count of a wave-round (what the gate of
GE_F64_PLANES lets through, and how many planes such a wave-round needs)."""
import argparse
import random

U = 2


def connected_gnm(n, m, rng):
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    while True:
        adj = [0] * n
        for a, b in rng.sample(pairs, m):
            adj[a] |= 1 << b
            adj[b] |= 1 << a
        seen, cur = 1, 1
        while cur:
            nxt = 0
            for v in range(n):
                if cur >> v & 1:
                    nxt |= adj[v]
            cur = nxt & ~seen
            seen |= cur
        if seen == (1 << n) - 1:
            return adj


def levels_of(adj, s):
    lv, seen = [1 << s], 1 << s
    while True:
        nxt = 0
        for v in range(len(adj)):
            if lv[-1] >> v & 1:
                nxt |= adj[v]
        nxt &= ~seen
        if not nxt:
            return lv
        seen |= nxt
        lv.append(nxt)


def inner(bits):
    lo, hi = bin(bits & 0xFFFFFFFF).count("1"), bin(bits >> 32).count("1")
    return (lo + U - 1) // U + (hi + U - 1) // U


def nodes(bits):
    return [v for v in range(64) if bits >> v & 1]


def pull(stretches):
    """stretches: per source of the wave, the list of inner trip counts of the nodes a level's pull visits, in the order dealt.
    -> (outer, inner) trips the wave pays for the level"""
    outer = max((len(s) + 7) // 8 for s in stretches)
    return outer, sum(max([max(s[8 * t:8 * t + 8], default=0) for s in stretches]) for t in range(outer))


def l2max(adj, lv):
    """the largest level-2 path count over the wave's searches (0: no search has a level 2)"""
    return max((bin(adj[v] & l[1]).count("1") for l in lv if len(l) > 2 for v in nodes(l[2])), default=0)


def wave(adj, sources, variant, levels=None):
    """variant: set of "l2pop", "planes", "leafskip", "sorted" -> ((outer, inner) forward, (outer, inner) backward);
    levels: a dict that takes the forward pull's (outer, inner) trips of this wave-round per level"""
    lv = [levels_of(adj, s) for s in sources]
    dw = max(len(l) for l in lv) - 1
    at = lambda l, d: l[d] if d < len(l) else 0
    order = (lambda c: sorted(c, reverse=True)) if "sorted" in variant else (lambda c: c)
    fo = fi = bo = bi = 0
    for d in range(2, dw + 1):
        st = [order([inner(adj[v] & at(l, d - 1)) for v in nodes(at(l, d))]) for l in lv]
        o, i = pull(st)
        if (d == 2 and "l2pop" in variant) or (d == 3 and "planes" in variant and l2max(adj, lv) <= 7):
            i = 0
        fo, fi = fo + o, fi + i
        if levels is not None:
            po, pi = levels.get(d, (0, 0))
            levels[d] = (po + o, pi + i)
    for d in range(dw - 1, 0, -1):
        st = []
        for l in lv:
            vs = nodes(at(l, d)) if d < len(l) - 1 else []  # (level D of a search is not visited)
            cs = [inner(adj[v] & at(l, d + 1)) for v in vs]
            if "leafskip" in variant:
                cs = [c for c in cs if c]
            st.append(order(cs))
        o, i = pull(st)
        bo, bi = bo + o, bi + i
    return fo, fi, bo, bi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=200)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--m", type=int, default=192)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = random.Random(a.seed)
    variants = [("shipped before round 10", set()), ("GE_F64_L2POP (shipped)", {"l2pop"}), ("+ level 3 from bit planes", {"l2pop", "planes"}),
                ("+ successor-bearing nodes only", {"l2pop", "planes", "leafskip"}),
                ("+ levels sorted by set size", {"l2pop", "planes", "leafskip", "sorted"})]
    split, largest = {}, {}  # forward trips per level with GE_F64_L2POP alone; wave-rounds by their largest level-2 count
    tot = {name: [0, 0, 0, 0] for name, _ in variants}
    waves = leaves = pairs = depth = 0
    for _ in range(a.graphs):
        adj = connected_gnm(a.n, a.m, rng)
        for base in range(0, a.n, 8):
            src = list(range(base, min(base + 8, a.n)))
            waves += 1
            for name, v in variants:
                for k, x in enumerate(wave(adj, src, v, split if v == {"l2pop"} else None)):
                    tot[name][k] += x
            lv = [levels_of(adj, s) for s in src]
            largest[l2max(adj, lv)] = largest.get(l2max(adj, lv), 0) + 1
            depth += max(len(l) for l in lv) - 1
            for l in lv:
                for d in range(1, len(l)):
                    for v in nodes(l[d]):
                        pairs += 1
                        leaves += not (d + 1 < len(l) and adj[v] & l[d + 1])
    print(f"# tools/f64_trip_model.py --graphs {a.graphs} --n {a.n} --m {a.m} --seed {a.seed}: a model, not a GPU measurement")
    print(f"# {a.graphs} connected G({a.n}, {a.m}), {waves} wave-rounds of eight sources; mean largest BFS depth of a wave {depth / waves:.2f};")
    print(f"# {100.0 * leaves / pairs:.1f} % of the (source, node) pairs below level 0 are leaves of the BFS DAG")
    print(f"{'per wave and round':34s} {'fwd outer':>10s} {'fwd inner':>10s} {'bwd outer':>10s} {'bwd inner':>10s} {'inner, both':>12s}")
    ref = None
    for name, _ in variants:
        fo, fi, bo, bi = (x / waves for x in tot[name])
        ref = ref or fi + bi
        print(f"{name:34s} {fo:10.1f} {fi:10.1f} {bo:10.1f} {bi:10.1f} {fi + bi:8.1f} {100.0 * (fi + bi) / ref - 100.0:+5.1f} %")
    print("# forward pull with GE_F64_L2POP, per level of the pulled nodes (mean trips per wave and round)")
    print(f"{'level':>34s} {'fwd outer':>10s} {'fwd inner':>10s}")
    for d in sorted(split):
        print(f"{d:34d} {split[d][0] / waves:10.1f} {split[d][1] / waves:10.1f}")
    print("# wave-rounds by the largest level-2 path count of their eight searches (GE_F64_PLANES: three planes, open up to 7)")
    print(f"{'largest count':>34s} {'wave-rounds':>12s} {'planes':>8s}")
    for c in sorted(largest):
        print(f"{c:34d} {largest[c]:12d} {('closed' if c > 7 else str(c.bit_length())):>8s}")
    gate = sum(k for c, k in largest.items() if c <= 7)
    print(f"# gate open in {gate} of {waves} wave-rounds ({100.0 * gate / waves:.1f} %)")


if __name__ == "__main__":
    main()
