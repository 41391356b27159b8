"""TEST INFRASTRUCTURE ONLY -- golden-vector generator (runs in the build container only).

Imports the real reference from /root/reference through oracle/refshim.py, rolls every
in-scope env with two deterministic policies and writes compact fixtures to
tests/golden/<case>.npz.  A fixture is data only: inputs (env id, kwargs, seeds, actions) and
the reference's outputs (obs, masks, rewards, done flags, info values).  No reference source
is stored.  Re-run:  python oracle/gen_golden.py [--only NAME[,NAME...]]
"""
import argparse
import hashlib
import json
import os
import platform
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

# name -> (env_id, kwargs, seeds)
CASES = {
    # BASELINE config 1 (plumbing) and SURVEY section 10 rows
    "sp_n10_m20_eval": ("ShortestPath-v0", dict(n_nodes=10, n_edges=20, is_eval_env=True), list(range(16))),
    "sp_n10_m20_unweighted": ("ShortestPath-v0", dict(n_nodes=10, n_edges=20, weighted=False, is_eval_env=True), list(range(4))),
    "sp_n5_m7": ("ShortestPath-v0", dict(n_nodes=5, n_edges=7), list(range(8))),
    # BASELINE config 2 (headline)
    "sp_n64_m192_eval": ("ShortestPath-v0", dict(n_nodes=64, n_edges=192, is_eval_env=True), [0, 1, 2, 3, 4, 5, 6, 7, 12345, 4294967295]),
    "sp_n33_m70": ("ShortestPath-v0", dict(n_nodes=33, n_edges=70, is_eval_env=True), list(range(4))),
    "lp_n10_m20_p0": ("LongestPath-v0", dict(n_nodes=10, n_edges=20, parenting=0, is_eval_env=True), list(range(6))),
    "lp_n10_m20_p1": ("LongestPath-v0", dict(n_nodes=10, n_edges=20, parenting=1, is_eval_env=True), list(range(8))),
    "lp_n10_m20_p2": ("LongestPath-v0", dict(n_nodes=10, n_edges=20, parenting=2, is_eval_env=True), list(range(8))),
    "lp_n64_m192_p2": ("LongestPath-v0", dict(n_nodes=64, n_edges=192, parenting=2), list(range(4))),
    # parenting 3 (longest_path.py:141-143) re-opens every residual node once <= n // 3 are left; the step asserts then reject a
    # non-neighbour (:153).  The fixture records where the reference raised (policy_raised / policy_raise_action).
    "lp_n12_m24_p3": ("LongestPath-v0", dict(n_nodes=12, n_edges=24, parenting=3, is_eval_env=True), list(range(12))),
    "lp_n30_m60_p3": ("LongestPath-v0", dict(n_nodes=30, n_edges=60, parenting=3), list(range(6))),
    "st_n10_m20_d3_eval": ("SteinerTree-v0", dict(n_nodes=10, n_edges=20, n_dests=3, is_eval_env=True), list(range(8))),
    "st_n10_m20_d1_eval": ("SteinerTree-v0", dict(n_nodes=10, n_edges=20, n_dests=1, is_eval_env=True), list(range(6))),
    "st_n10_m20_d9_eval": ("SteinerTree-v0", dict(n_nodes=10, n_edges=20, n_dests=9, is_eval_env=True), list(range(6))),
    "st_n5_m10_d4": ("SteinerTree-v0", dict(n_nodes=5, n_edges=10, n_dests=4), list(range(4))),
    "st_n10_m20_d3_unweighted": ("SteinerTree-v0", dict(n_nodes=10, n_edges=20, n_dests=3, weighted=False), list(range(3))),
    # BASELINE config 4
    "st_n256_m1024_d8": ("SteinerTree-v0", dict(n_nodes=256, n_edges=1024, n_dests=8), [0, 1]),
    "tsp_n8_m28_p1": ("TSP-v0", dict(n_nodes=8, n_edges=28, parenting=1), list(range(6))),
    "tsp_n10_m20_p1": ("TSP-v0", dict(n_nodes=10, n_edges=20, parenting=1), list(range(8))),
    "tsp_n10_m20_p2": ("TSP-v0", dict(n_nodes=10, n_edges=20, parenting=2), list(range(8))),
    "tsp_n12_m30_p2_spatial": ("TSP-v0", dict(n_nodes=12, n_edges=30, parenting=2, spatial=True), list(range(4))),
    "tsp_n12_m30_p1_unweighted": ("TSP-v0", dict(n_nodes=12, n_edges=30, parenting=1, weighted=False), list(range(3))),
    # BASELINE config 3
    "tsp_n128_complete_p1": ("TSP-v0", dict(n_nodes=128, n_edges=8128, parenting=1), [0]),
    "mis_n6_m8": ("MaxIndependentSet-v0", dict(n_nodes=6, n_edges=8), list(range(6))),
    "mis_n5_m7_unweighted": ("MaxIndependentSet-v0", dict(n_nodes=5, n_edges=7, weighted=False), list(range(4))),
    "mis_n64_m192": ("MaxIndependentSet-v0", dict(n_nodes=64, n_edges=192), list(range(4))),
    "ds_n10_m20_p1": ("DensestSubgraph-v0", dict(n_nodes=10, n_edges=20, parenting=1), list(range(8))),
    "ds_n10_m20_p0_eval": ("DensestSubgraph-v0", dict(n_nodes=10, n_edges=20, parenting=0, is_eval_env=True), list(range(8))),
    "ds_n64_m192_p1": ("DensestSubgraph-v0", dict(n_nodes=64, n_edges=192, parenting=1), list(range(4))),
    # BASELINE config 5 (ragged sizes; the three env types at the extremes of n in [32,512], m=3n)
    "sp_n32_m96": ("ShortestPath-v0", dict(n_nodes=32, n_edges=96), [0, 1]),
    "sp_n512_m1536": ("ShortestPath-v0", dict(n_nodes=512, n_edges=1536), [0]),
    "mis_n200_m600": ("MaxIndependentSet-v0", dict(n_nodes=200, n_edges=600), [0]),
    "ds_n100_m300_p1": ("DensestSubgraph-v0", dict(n_nodes=100, n_edges=300, parenting=1), [0, 1]),
    # reference values of the heavy baselines (Kou, Christofides, clique-removal MIS), for the bound checks
    "st_n20_m45_d5_eval": ("SteinerTree-v0", dict(n_nodes=20, n_edges=45, n_dests=5, is_eval_env=True), list(range(8))),
    "tsp_n10_m20_p1_eval": ("TSP-v0", dict(n_nodes=10, n_edges=20, parenting=1, is_eval_env=True), list(range(8))),
    "tsp_n12_m30_p2_spatial_eval": ("TSP-v0", dict(n_nodes=12, n_edges=30, parenting=2, spatial=True, is_eval_env=True), list(range(4))),
    "mis_n12_m20_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=12, n_edges=20, weighted=False, is_eval_env=True), list(range(8))),
    # MulticastRouting (multicast_routing.py)
    "mc_n10_m20_p4": ("MulticastRouting-v0", dict(n_nodes=10, n_edges=20), list(range(10))),
    "mc_n10_m20_p3_d2": ("MulticastRouting-v0", dict(n_nodes=10, n_edges=20, n_dests=2, parenting=3), list(range(6))),
    "mc_n10_m20_p2": ("MulticastRouting-v0", dict(n_nodes=10, n_edges=20, parenting=2), list(range(8))),
    "mc_n10_m20_p1": ("MulticastRouting-v0", dict(n_nodes=10, n_edges=20, parenting=1), list(range(8))),
    "mc_n12_auto_edges_p4_unweighted": ("MulticastRouting-v0", dict(n_nodes=12, weighted=False), list(range(4))),
    "mc_n10_m20_p4_eval": ("MulticastRouting-v0", dict(n_nodes=10, n_edges=20, is_eval_env=True), list(range(8))),
    "mc_n64_m192_p4_d5": ("MulticastRouting-v0", dict(n_nodes=64, n_edges=192, n_dests=5), list(range(4))),
    "mc_n64_m192_p2_d8": ("MulticastRouting-v0", dict(n_nodes=64, n_edges=192, n_dests=8, parenting=2), list(range(3))),
    "mc_n200_m600_p4_d6": ("MulticastRouting-v0", dict(n_nodes=200, n_edges=600, n_dests=6), [0]),
    "mc_n64_m192_p4_d40_eval": ("MulticastRouting-v0", dict(n_nodes=64, n_edges=192, n_dests=40, is_eval_env=True), list(range(3))),
    # DistributionCenter (distribution_center.py)
    "dc_n10_m20_p2": ("DistributionCenter-v0", dict(n_nodes=10, n_edges=20), list(range(10))),
    "dc_n10_m20_p1": ("DistributionCenter-v0", dict(n_nodes=10, n_edges=20, parenting=1), list(range(6))),
    "dc_n12_m25_p2_unweighted_t4": ("DistributionCenter-v0", dict(n_nodes=12, n_edges=25, weighted=False, target_count=4), list(range(6))),
    "dc_n20_m40_p2_dist1p5_eval": ("DistributionCenter-v0", dict(n_nodes=20, n_edges=40, max_distance=1.5, is_eval_env=True), list(range(6))),
    "dc_n64_m192_p2": ("DistributionCenter-v0", dict(n_nodes=64, n_edges=192), list(range(6))),
    "dc_n64_m192_p2_dist0p7": ("DistributionCenter-v0", dict(n_nodes=64, n_edges=192, max_distance=0.7, target_count=20), list(range(4))),
    "dc_n200_m600_p2": ("DistributionCenter-v0", dict(n_nodes=200, n_edges=600), [0, 1]),
    "dc_n300_m900_p1_dist2": ("DistributionCenter-v0", dict(n_nodes=300, n_edges=900, parenting=1, max_distance=2), [0]),
    # PerishableProductDelivery (perishable_product_delivery.py); parenting must be 1
    "ppd_n10_m20": ("PerishableProductDelivery-v0", dict(n_nodes=10, n_edges=20, parenting=1), list(range(10))),
    "ppd_n12_m30_p5_eval": ("PerishableProductDelivery-v0", dict(n_nodes=12, n_edges=30, n_products=5, parenting=1, is_eval_env=True), list(range(6))),
    "ppd_n8_m9_p3": ("PerishableProductDelivery-v0", dict(n_nodes=8, n_edges=9, parenting=1), list(range(12))),
    "ppd_n12_auto_unweighted": ("PerishableProductDelivery-v0", dict(n_nodes=12, n_edges=-1, weighted=False, n_products=2, parenting=1), list(range(4))),
    "ppd_n64_m192_eval": ("PerishableProductDelivery-v0", dict(n_nodes=64, n_edges=192, parenting=1, is_eval_env=True), list(range(4))),
    "ppd_n100_m300_p4": ("PerishableProductDelivery-v0", dict(n_nodes=100, n_edges=300, n_products=4, parenting=1), [0, 1]),
    # complete graphs ([nx] complete_graph: sorted adjacency) through the widened envs
    "ppd_n7_m21_complete": ("PerishableProductDelivery-v0", dict(n_nodes=7, n_edges=21, n_products=2, parenting=1, is_eval_env=True), list(range(8))),
    "mc_n8_m28_complete_p4_eval": ("MulticastRouting-v0", dict(n_nodes=8, n_edges=28, n_dests=3, is_eval_env=True), list(range(6))),
    "dc_n8_m28_complete_dist0p6": ("DistributionCenter-v0", dict(n_nodes=8, n_edges=28, max_distance=0.6, target_count=3), list(range(6))),
    "mc_n300_m900_p3_d4_eval": ("MulticastRouting-v0", dict(n_nodes=300, n_edges=900, n_dests=4, parenting=3, is_eval_env=True), [0]),
    # round 3: the heavy is_eval_env baselines at sizes where the restated dict / set iteration orders do real work on the device
    # (the engine and the C oracle share that source text, so these reference values -- not the oracle -- are their pin)
    "st_n256_m1024_d8_eval": ("SteinerTree-v0", dict(n_nodes=256, n_edges=1024, n_dests=8, is_eval_env=True), [0]),
    "st_n64_m192_d8_eval": ("SteinerTree-v0", dict(n_nodes=64, n_edges=192, n_dests=8, is_eval_env=True), [0, 1, 2]),
    "mis_n64_m192_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=64, n_edges=192, weighted=False, is_eval_env=True), [0, 1, 2, 3]),
    "mis_n200_m600_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=200, n_edges=600, weighted=False, is_eval_env=True), [0]),
    "tsp_n64_m400_p1_eval": ("TSP-v0", dict(n_nodes=64, n_edges=400, parenting=1, is_eval_env=True), [0]),
    # round 3: sizes the engine refused before (parenting >= 2 and spatial TSP above 512 nodes)
    "lp_n600_m1800_p2": ("LongestPath-v0", dict(n_nodes=600, n_edges=1800, parenting=2), [0]),
    "lp_n530_m1500_p3": ("LongestPath-v0", dict(n_nodes=530, n_edges=1500, parenting=3), [0]),
    "tsp_n520_m1700_p2": ("TSP-v0", dict(n_nodes=520, n_edges=1700, parenting=2), [0]),
    "tsp_n600_m2000_p1_spatial": ("TSP-v0", dict(n_nodes=600, n_edges=2000, parenting=1, spatial=True), [0]),
    "ppd_n200_m600_eval": ("PerishableProductDelivery-v0", dict(n_nodes=200, n_edges=600, parenting=1, is_eval_env=True), [0, 1]),
    "ppd_n300_m900_unweighted": ("PerishableProductDelivery-v0", dict(n_nodes=300, n_edges=900, n_products=2, weighted=False, parenting=1), [0]),
    # round 4: weighted PerishableProductDelivery above 256 nodes (the n x n delay matrix no longer fits LDS: the engine keeps the codes of
    # the attempt's edges only)
    "ppd_n300_m900": ("PerishableProductDelivery-v0", dict(n_nodes=300, n_edges=900, n_products=3, parenting=1), [0, 1]),
    # round 4: ten more reference values of the two baselines whose source text the engine and the C oracle share (networkx's Kou tree
    # with 2 and n - 2 destinations, clique removal on sparse and dense graphs) at n = 32 / 100 / 300
    "st_n32_m80_d2_eval": ("SteinerTree-v0", dict(n_nodes=32, n_edges=80, n_dests=2, is_eval_env=True), [0, 1, 2, 3]),
    "st_n32_m80_d30_eval": ("SteinerTree-v0", dict(n_nodes=32, n_edges=80, n_dests=30, is_eval_env=True), [0, 1, 2, 3]),
    "st_n100_m300_d2_eval": ("SteinerTree-v0", dict(n_nodes=100, n_edges=300, n_dests=2, is_eval_env=True), [0, 1]),
    "st_n100_m300_d98_eval": ("SteinerTree-v0", dict(n_nodes=100, n_edges=300, n_dests=98, is_eval_env=True), [0, 1]),
    "st_n300_m900_d2_eval": ("SteinerTree-v0", dict(n_nodes=300, n_edges=900, n_dests=2, is_eval_env=True), [0]),
    "st_n300_m900_d298_unweighted_eval": ("SteinerTree-v0", dict(n_nodes=300, n_edges=900, n_dests=298, weighted=False, is_eval_env=True), [0]),
    "mis_n32_m40_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=32, n_edges=40, weighted=False, is_eval_env=True), [0, 1, 2, 3]),
    "mis_n32_m300_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=32, n_edges=300, weighted=False, is_eval_env=True), [0, 1, 2, 3]),
    "mis_n100_m180_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=100, n_edges=180, weighted=False, is_eval_env=True), [0, 1]),
    "mis_n100_m2500_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=100, n_edges=2500, weighted=False, is_eval_env=True), [0, 1]),
    "mis_n300_m6000_unweighted_eval": ("MaxIndependentSet-v0", dict(n_nodes=300, n_edges=6000, weighted=False, is_eval_env=True), [0]),
    # round 4: spatial TSP seeds on which the reference's (dx)**2 -- Python float ** int, libm pow(dx, 2.0) -- differs from dx * dx in
    # the last bit and the edge weight sqrt(dx**2 + dy**2) with it (found by search: 3 of 400 seeds at this size; one square in 1 200
    # differs under glibc 2.35).  The engine and the checker multiply, so rewards of such an edge agree to 1 ulp of float64, not exactly:
    # the replay compares the rewards of spatial TSP within north_star's 1e-6 and reports how many were inexact
    "tsp_n12_m30_p1_spatial_pow2": ("TSP-v0", dict(n_nodes=12, n_edges=30, parenting=1, spatial=True), [42, 217, 277]),
    # above 600 nodes, up to the largest graphs the engine admits (tests/test_geometry_limits.py finds that edge: n = 794 at m = 3 n,
    # n = 768 at the m = 4 n of TSP, whose reset would reject about every graph of m = 3 n for a node of degree 1): node sets of 10 to
    # 13 words, the generic feature kernel at its lowest wave counts.  One seed each; few destinations keep the edge-action episodes
    # (and their packed masks) short
    "sp_n794_m2382_eval": ("ShortestPath-v0", dict(n_nodes=794, n_edges=2382, is_eval_env=True), [0]),
    "sp_n705_m2000": ("ShortestPath-v0", dict(n_nodes=705, n_edges=2000), [0]),
    "lp_n700_m2100_p2": ("LongestPath-v0", dict(n_nodes=700, n_edges=2100, parenting=2), [0]),
    "lp_n793_m2379_p2": ("LongestPath-v0", dict(n_nodes=793, n_edges=2379, parenting=2), [0]),
    "tsp_n768_m3072_p2": ("TSP-v0", dict(n_nodes=768, n_edges=3072, parenting=2), [0]),
    "tsp_n615_m2100_p1_spatial": ("TSP-v0", dict(n_nodes=615, n_edges=2100, parenting=1, spatial=True), [0]),  # (larger ones pass the size of tsp_n128_complete_p1.npz)
    "ds_n720_m2160_p1": ("DensestSubgraph-v0", dict(n_nodes=720, n_edges=2160, parenting=1), [0]),
    "mis_n790_m2370": ("MaxIndependentSet-v0", dict(n_nodes=790, n_edges=2370), [0]),
    "dc_n680_m2040_p2": ("DistributionCenter-v0", dict(n_nodes=680, n_edges=2040), [0]),
    "mc_n750_m2250_p4_d3": ("MulticastRouting-v0", dict(n_nodes=750, n_edges=2250, n_dests=3), [0]),
    "ppd_n640_m1920_p2": ("PerishableProductDelivery-v0", dict(n_nodes=640, n_edges=1920, n_products=2, parenting=1), [0]),
    "st_n792_m2376_d3": ("SteinerTree-v0", dict(n_nodes=792, n_edges=2376, n_dests=3), [0]),
}

# constructor calls whose outcome in the reference (built, or the exception its asserts raise) is recorded once in
# tests/golden/constructor_refusals.json (--constructors): every parenting value around each env's range, the weighted / spatial /
# n_products asserts and a kwarg an env does not take.  n_nodes = 12, n_edges = 30 throughout
_G = dict(n_nodes=12, n_edges=30)
CONSTRUCTORS = (
    [("ShortestPath-v0", dict(_G, **kw)) for kw in (dict(), dict(parenting=-1), dict(parenting=0), dict(parenting=1), dict(weighted=False))]
    + [("LongestPath-v0", dict(_G, **kw)) for kw in (dict(),) + tuple(dict(parenting=p) for p in (-1, 0, 1, 2, 3, 4))]
    + [("SteinerTree-v0", dict(_G, **kw)) for kw in (dict(), dict(parenting=-1), dict(parenting=1), dict(parenting=2), dict(n_dests=5))]
    + [("TSP-v0", dict(_G, **kw)) for kw in (dict(),) + tuple(dict(parenting=p) for p in (-1, 0, 1, 2, 3))
       + (dict(parenting=1, spatial=True), dict(parenting=1, spatial=True, weighted=False), dict(parenting=2, weighted=False))]
    + [("DensestSubgraph-v0", dict(_G, **kw)) for kw in (dict(),) + tuple(dict(parenting=p) for p in (-1, 0, 1, 2))
       + (dict(parenting=1, weighted=True), dict(parenting=0, weighted=True), dict(parenting=1, weighted=False))]
    + [("MaxIndependentSet-v0", dict(_G, **kw)) for kw in (dict(), dict(weighted=False), dict(parenting=1))]
    + [("MulticastRouting-v0", dict(_G, **kw)) for kw in (dict(),) + tuple(dict(parenting=p) for p in (-1, 0, 1, 2, 3, 4, 5))]
    + [("DistributionCenter-v0", dict(_G, **kw)) for kw in (dict(),) + tuple(dict(parenting=p) for p in (-1, 0, 1, 2, 3))]
    + [("PerishableProductDelivery-v0", dict(_G, **kw)) for kw in (dict(),) + tuple(dict(parenting=p) for p in (-1, 0, 1, 2))
       + tuple(dict(parenting=1, n_products=k) for k in (1, 5, 6, 7)) + (dict(parenting=2, n_products=6),)]
)

POLICIES = ("first", "rand")


def sha64(a: np.ndarray) -> np.uint64:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], dtype=np.uint64)[0]


def pick(policy, mask, rng):
    va = np.nonzero(mask)[0]
    if len(va) == 0:
        return -1
    return int(va[0]) if policy == "first" else int(rng.choice(va))


def terminals_of(env, env_id):
    if env_id in ("ShortestPath-v0", "LongestPath-v0"):
        return [int(env.src), int(env.dest)]
    if env_id == "SteinerTree-v0":
        return [int(env.src)] + [int(d) for d in env.dests]
    if env_id == "TSP-v0":
        return [0]
    if env_id == "MulticastRouting-v0":
        return [int(env.src)] + [int(d) for d in env.dests]
    if env_id == "PerishableProductDelivery-v0":
        return [int(v) for v in env.pickups] + [int(v) for v in env.dropoffs]
    if env_id == "DistributionCenter-v0":
        return [int(t) for t in env.in_range_dict]  # targets, in the order they were drawn
    return []


def roll(gym, env_id, kwargs, seed, policy, max_steps=4000):
    env = gym.make(env_id, **kwargs)
    obs, info = env.reset(seed=seed)
    rec = dict(reset_obs=obs.copy(), reset_mask=info["mask"].copy(), terminals=terminals_of(env, env_id))
    rng = np.random.default_rng(1000 + seed)
    acts, rews, dones, masks, shas = [], [], [], [], []
    mask = info["mask"]
    final = dict(solved=-1, solution_cost=np.nan, heuristic_solution=np.nan, raised=0, raise_action=-1)
    for _ in range(max_steps):
        a = pick(policy, mask, rng)
        if a < 0:
            break
        try:
            obs, r, d, trunc, info = env.step(a)
        except AssertionError:  # the reference's own asserts on an action its mask allowed (LongestPath parenting 3)
            final["raised"], final["raise_action"] = 1, a
            break
        assert trunc is False
        acts.append(a); rews.append(float(r)); dones.append(bool(d)); shas.append(sha64(obs))
        if "mask" in info:
            mask = info["mask"]
        masks.append(np.asarray(mask, dtype=bool).copy())
        if d:
            if "solved" in info:
                final["solved"] = int(bool(info["solved"]))
            final["solution_cost"] = float(info["solution_cost"])
            final["heuristic_solution"] = float(info["heuristic_solution"])
            break
    rec.update(actions=acts, rewards=rews, dones=dones, masks=masks, obs_sha=shas, final_obs=obs.copy(), **final)
    # reset(seed=None) continues the process-global streams (shortest_path.py:49-52)
    obs2, info2 = env.reset()
    rec["reset2_obs_sha"] = sha64(obs2)
    rec["reset2_mask"] = info2["mask"].copy()
    return rec


def build_case(gym, name):
    import networkx, scipy
    env_id, kwargs, seeds = CASES[name]
    out = {}
    for policy in POLICIES:
        recs = [roll(gym, env_id, kwargs, s, policy) for s in seeds]
        S = len(recs)
        T = max(len(r["actions"]) for r in recs)
        A = len(recs[0]["reset_mask"])
        L = len(recs[0]["reset_obs"])
        K = len(recs[0]["terminals"])
        P = policy + "_"
        out[P + "length"] = np.array([len(r["actions"]) for r in recs], dtype=np.int32)
        acts = np.full((S, T), -1, dtype=np.int32)
        rews = np.zeros((S, T), dtype=np.float64)
        dones = np.zeros((S, T), dtype=bool)
        shas = np.zeros((S, T), dtype=np.uint64)
        masks = np.zeros((S, T, (A + 7) // 8), dtype=np.uint8)
        for i, r in enumerate(recs):
            t = len(r["actions"])
            acts[i, :t] = r["actions"]; rews[i, :t] = r["rewards"]; dones[i, :t] = r["dones"]; shas[i, :t] = r["obs_sha"]
            if t:
                masks[i, :t] = np.packbits(np.stack(r["masks"]), axis=1, bitorder="little")
        out[P + "actions"], out[P + "rewards"], out[P + "dones"] = acts, rews, dones
        out[P + "obs_sha"], out[P + "masks_packed"] = shas, masks
        out[P + "final_obs"] = np.stack([r["final_obs"] for r in recs]).astype(np.float32)
        out[P + "solved"] = np.array([r["solved"] for r in recs], dtype=np.int8)
        out[P + "solution_cost"] = np.array([r["solution_cost"] for r in recs], dtype=np.float64)
        out[P + "heuristic_solution"] = np.array([r["heuristic_solution"] for r in recs], dtype=np.float64)
        if any(r["raised"] for r in recs):
            out[P + "raised"] = np.array([r["raised"] for r in recs], dtype=np.int8)
            out[P + "raise_action"] = np.array([r["raise_action"] for r in recs], dtype=np.int32)
        out[P + "reset2_obs_sha"] = np.array([r["reset2_obs_sha"] for r in recs], dtype=np.uint64)
        out[P + "reset2_mask"] = np.stack([r["reset2_mask"] for r in recs])
        if policy == POLICIES[0]:
            out["reset_obs"] = np.stack([r["reset_obs"] for r in recs]).astype(np.float32)
            out["reset_mask"] = np.stack([r["reset_mask"] for r in recs]).astype(bool)
            out["terminals"] = np.array([r["terminals"] for r in recs], dtype=np.int32).reshape(S, K)
            assert out["reset_obs"].shape == (S, L)
    meta = dict(case=name, env_id=env_id, kwargs=kwargs, seeds=[int(s) for s in seeds], policies=list(POLICIES),
                rand_policy="numpy default_rng(1000+seed).choice(valid_actions)",
                versions=dict(python=platform.python_version(), numpy=np.__version__,
                              networkx=networkx.__version__, scipy=scipy.__version__),
                source="reference teshnizi/GraphEnvs graph-envs 0.0.54 via oracle/refshim.py")
    out["meta"] = np.array(json.dumps(meta))
    out["seeds"] = np.array(seeds, dtype=np.int64)
    return out


def record_constructors(gym):
    """data only: the (env id, kwargs) of CONSTRUCTORS and, for each, whether the reference's constructor raised and with what type"""
    rows = []
    for env_id, kwargs in CONSTRUCTORS:
        try:
            gym.make(env_id, **kwargs)
            raised = None
        except (AssertionError, ValueError, TypeError) as e:
            raised = type(e).__name__
        rows.append(dict(env_id=env_id, kwargs=kwargs, raised=raised is not None, error=raised))
    path = os.path.join(OUT, "constructor_refusals.json")
    with open(path, "w") as f:
        json.dump(dict(source="reference teshnizi/GraphEnvs graph-envs 0.0.54 via oracle/refshim.py", cases=rows), f, indent=1)
        f.write("\n")
    print(f"constructor_refusals.json: {len(rows)} calls, {sum(r['raised'] for r in rows)} refused")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--constructors", action="store_true", help="record the constructor outcomes only")
    args = ap.parse_args()
    gym, _ = refshim.load_reference()
    os.makedirs(OUT, exist_ok=True)
    if args.constructors:
        record_constructors(gym)
        return
    for name in CASES:
        if args.only and name not in args.only.split(","):
            continue
        t0 = time.time()
        data = build_case(gym, name)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **data)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB in {time.time() - t0:.1f}s", flush=True)


if __name__ == "__main__":
    main()
