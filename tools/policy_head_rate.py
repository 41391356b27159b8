"""The masked categorical policy head against the torch composition it replaces, on the same engine, logits and box.

(a) what a user writes today: masked_fill(~mask) -> log_softmax -> Gumbel-max draw -> gather -> entropy (a multi-class engine: that
    chain looped over the classes' [B_c, A_c] blocks);
(b) env.sample_actions(logits).
All variants are timed warm with HIP events in ALTERNATION -- repetition r times every variant once, `--inner` back-to-back calls
each -- so that clock and thermal drift falls on all of them alike.  Call k reads logits buffer k mod `--buffers`: the buffers
together exceed the 256 MB Infinity Cache, so no call finds its logits cached by the call before (`--buffers 1` shows the
cache-resident rate).  Printed: median and min .. max of the per-call time, the bytes (b) must move (logits once, mask words, slot
records, the three outputs), the fraction of the 8 TB/s HBM peak those bytes over the median time are, and one JSON line per shape.
No rate is printed without a GPU."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import graphenvs_amd as ge

HBM_PEAK = 8.0e12  # bytes/s (spec)

SHAPES = {
    "headline": ("ShortestPath-v0", dict(n_nodes=64, n_edges=192), 65536),
    "config4": ("SteinerTree-v0", dict(n_nodes=256, n_edges=1024, n_dests=8), 16384),
    "ragged3": ("ShortestPath-v0", [(24576, 16, 40), (24576, 32, 96), (16384, 64, 192)], None),
    "ragged3-wide": ("ShortestPath-v0", [(8192, 12, 30), (8192, 64, 192), (8192, 100, 300)], None),
}


def torch_chain(blocks, gumbel):
    """the composition per [B_c, A_c] block; blocks: (logits, bool mask, noise)"""
    out = []
    for x, mask, u in blocks:
        lp = torch.log_softmax(x.masked_fill(~mask, float("-inf")), dim=1)
        p = lp.exp()
        if gumbel:
            a = (lp - torch.log(-torch.log(u.uniform_(1e-20, 1.0)))).argmax(dim=1)
        else:
            a = torch.multinomial(p, 1).squeeze(1)
        out.append((a, lp.gather(1, a[:, None]).squeeze(1), -(p * lp.masked_fill(~mask, 0.0)).sum(dim=1)))
    return out


def timed(variants, reps, inner):
    """variants: {name: fn(k)}, k the running call number.  Every repetition times each variant once, one after the other"""
    calls = 0
    for fn in variants.values():
        for _ in range(3):
            fn(calls); calls += 1
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn(calls); calls += 1
            t1.record(); torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) * 1e3 / inner)
    out = {}
    for name, v in ms.items():
        v.sort()
        out[name] = dict(median_us=v[len(v) // 2], min_us=v[0], max_us=v[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,config4,ragged3,ragged3-wide")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=0, help="logits buffers rotated through (0: as many as exceed 320 MB together)")
    ap.add_argument("--rollout", type=int, default=40, help="random steps before timing, so that masks have thinned out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_head_rate: no GPU visible (a rate measured elsewhere says nothing about the MI355X)")
    for name in args.shapes.split(","):
        env_id, geo, B = SHAPES[name]
        ragged = B is None
        env = ge.RaggedVectorEnv(env_id, geo) if ragged else ge.VectorGraphEnv(env_id, B, **geo)
        env.reset(seed=0); env.random_rollout(args.rollout, policy_seed=1)
        members = env.classes if ragged else [env]
        numel = sum(c.num_envs * c.A for c in members)
        g = torch.Generator(device="cuda"); g.manual_seed(0)
        nbuf = args.buffers or max(2, -(-320_000_000 // (numel * 4)))
        bufs = [(torch.randn(numel, device="cuda", generator=g) * 2).clamp_(-8, 8) for _ in range(nbuf)]
        sets = []  # per buffer: the (logits, bool mask, noise) blocks of the classes
        for logits in bufs:
            blocks, off = [], 0
            for c in members:
                x = logits[off:off + c.num_envs * c.A].view(c.num_envs, c.A); off += c.num_envs * c.A
                blocks.append((x, c.mask, torch.empty_like(x) if not sets else sets[0][len(blocks)][2]))
            sets.append(blocks)
        a, lp, en = env.sample_actions(bufs[0], 1)
        a, en = a.clone(), en.clone()
        ref = torch_chain(sets[0], True)
        en_ref = torch.cat([r[2] for r in ref])
        live = a >= 0
        # (same masked softmax: the entropies agree to float32 rounding; the draws differ by construction)
        err = float((en[live] - en_ref[live]).abs().max())
        res = dict(shape=name, env_id=env_id, slots=env.num_envs, logits=numel, buffers=nbuf, entropy_max_abs_diff_vs_torch=err)
        mask_flat = torch.cat([c.t["mask"].reshape(-1) for c in members])
        res.update(timed({
            "torch_gumbel": lambda k: torch_chain(sets[k % nbuf], True),
            "torch_multinomial": lambda k: torch_chain(sets[k % nbuf], False),
            "sample_actions": lambda k: env.sample_actions(bufs[k % nbuf], 1),
            "sample_actions_greedy": lambda k: env.sample_actions(bufs[k % nbuf], 1, greedy=True),
            "evaluate_actions": lambda k: env.evaluate_actions(bufs[k % nbuf], a, mask_flat),
        }, args.reps, args.inner))
        Bt = env.num_envs
        res["bytes_sample"] = numel * 4 + sum(c.num_envs * ((c.A + 63) // 64) * 8 for c in members) + Bt * 8 + Bt * 16 + (Bt * 4 if ragged else 0)
        res["bytes_evaluate"] = numel * 5 + Bt * 8 + Bt * 8 + (Bt * 4 if ragged else 0)
        res["hbm_frac_sample"] = res["bytes_sample"] / (res["sample_actions"]["median_us"] * 1e-6) / HBM_PEAK
        res["hbm_frac_evaluate"] = res["bytes_evaluate"] / (res["evaluate_actions"]["median_us"] * 1e-6) / HBM_PEAK
        res["speedup_vs_torch_gumbel"] = res["torch_gumbel"]["median_us"] / res["sample_actions"]["median_us"]
        res["speedup_vs_torch_multinomial"] = res["torch_multinomial"]["median_us"] / res["sample_actions"]["median_us"]
        for k in ("torch_gumbel", "torch_multinomial", "sample_actions", "sample_actions_greedy", "evaluate_actions"):
            t = res[k]
            print(f"{name:13s} {k:22s} median {t['median_us']:9.1f} us   min {t['min_us']:9.1f}   max {t['max_us']:9.1f}", flush=True)
        print(f"{name:13s} sample_actions moves {res['bytes_sample'] / 1e6:.1f} MB = {100 * res['hbm_frac_sample']:.1f} % of the 8 TB/s HBM peak; "
              f"{res['speedup_vs_torch_gumbel']:.1f}x the Gumbel-max chain, {res['speedup_vs_torch_multinomial']:.1f}x the multinomial chain", flush=True)
        print(json.dumps(res), flush=True)
        env.close(); del env, sets, bufs


if __name__ == "__main__":
    main()
