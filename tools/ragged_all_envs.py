"""Size curricula of the env ids the multi-class engine took on last (everything but BASELINE config 5's three): per id 16 384 slots
over 32 classes, n from 32 to 256 and m = 3 n (MST: SteinerTree with n_dests = n - 1, n from 32 to 128).  Steady-state env-steps/s
of (a) one multi-class engine (RaggedVectorEnv), (b) one uniform VectorGraphEnv per class in MixedVectorEnv(concurrent=False), (c)
the same classes in the default MixedVectorEnv (a HIP stream per member).  random_rollout; a settle of two of the longest episode
(2 n_max steps: the node walks end within n steps; PerishableProductDelivery's cap is 150 n, so its settle is the same 2 n_max
steps, not two of its longest episodes), then a window of at least 0.3 s.  Also one SteinerTree class (16 384 slots, n = 256,
m = 1 024) as a multi-class engine against the uniform engine.  Prints one JSON line.
usage: python tools/ragged_all_envs.py [--ids TSP-v0,...] [--slots 16384] [--classes 32] [--no-one-class]  (--ids "": the one-class
comparison alone)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphenvs_amd as ge  # noqa: E402
from graphenvs_amd import _lib  # noqa: E402

IDS = {
    "LongestPath-v0": (dict(parenting=2), 32, 256, False),
    "SteinerTree-v0": (dict(n_dests=3), 32, 256, False),
    "MST": ({}, 32, 128, True),
    "TSP-v0": (dict(parenting=1), 32, 256, False),
    "MulticastRouting-v0": (dict(parenting=4), 32, 256, False),
    "DistributionCenter-v0": (dict(parenting=2), 32, 256, False),
    "PerishableProductDelivery-v0": (dict(parenting=1), 32, 256, False),
}


def curriculum(slots, classes, lo, hi):
    ns = np.unique(np.linspace(lo, hi, classes).round().astype(int))
    per = [slots // len(ns) + (1 if c < slots % len(ns) else 0) for c in range(len(ns))]
    return [(b, int(n), 3 * int(n)) for b, n in zip(per, ns)]


def rate(env, B, settle, min_s=0.3):
    env.reset(seed=0)
    env.random_rollout(settle, policy_seed=1)
    torch.cuda.synchronize()
    k = 8
    while True:
        t0 = time.perf_counter()
        env.random_rollout(k, policy_seed=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return B * k / dt
        k = max(2 * k, int(k * min_s * 1.3 / max(dt, 1e-6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", default=",".join(IDS))
    ap.add_argument("--slots", type=int, default=16384)
    ap.add_argument("--classes", type=int, default=32)
    ap.add_argument("--no-one-class", action="store_true", help="skip the one-class SteinerTree comparison")
    args = ap.parse_args()
    out = {"source_hash": _lib.source_hash(), "slots": args.slots, "classes": args.classes, "env_steps_per_s": {}}
    for key in filter(None, args.ids.split(",")):
        common, lo, hi, mst = IDS[key]
        eid = "SteinerTree-v0" if mst else key
        sizes = curriculum(args.slots, args.classes, lo, hi)
        entries = [(b, n, m, dict(n_dests=n - 1)) for b, n, m in sizes] if mst else sizes
        settle = 2 * hi
        res = {}
        env = ge.RaggedVectorEnv(eid, entries, device="cuda", **common)
        res["a_ragged"] = rate(env, env.num_envs, settle)
        env.close()
        for name, concurrent in (("b_uniform_serial", False), ("c_uniform_streams", True)):
            members, start = [], 0
            for b, n, m in sizes:
                kw = dict(common, n_dests=n - 1) if mst else dict(common)
                members.append(ge.VectorGraphEnv(eid, b, n, m, device="cuda", env_index_base=start, seed_stride=args.slots, **kw))
                start += b
            mixed = ge.MixedVectorEnv(members, concurrent=concurrent)
            res[name] = rate(mixed, mixed.num_envs, settle)
            mixed.close()
        res["a_over_b"] = res["a_ragged"] / res["b_uniform_serial"]
        out["env_steps_per_s"][key] = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in res.items()}
        print(key, json.dumps(out["env_steps_per_s"][key]), file=sys.stderr, flush=True)
    if not args.no_one_class:
        # the ragged edge-action kernel on ONE class against the uniform engine's (n = 256, m = 1 024: both take the quad kernel);
        # the kernel durations themselves come from a --kernel-trace run of this tool
        one = {}
        env = ge.RaggedVectorEnv("SteinerTree-v0", [(args.slots, 256, 1024)], device="cuda", n_dests=3)
        one["ragged"] = rate(env, args.slots, 512)
        env.close()
        env = ge.VectorGraphEnv("SteinerTree-v0", args.slots, 256, 1024, device="cuda", n_dests=3)
        one["uniform"] = rate(env, args.slots, 512)
        env.close()
        one["uniform_over_ragged"] = one["uniform"] / one["ragged"]
        out["steiner_one_class_n256_m1024"] = {k: round(v, 3) for k, v in one.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
