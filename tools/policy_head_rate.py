"""The masked categorical policy head against the torch composition it replaces, on the same engine, logits and box.

(a) what a user writes today: masked_fill(~mask) -> log_softmax -> Gumbel-max draw -> gather -> entropy (a multi-class engine: that
    chain looped over the classes' [B_c, A_c] blocks);
(b) env.sample_actions(logits).
All variants are timed warm with HIP events in ALTERNATION -- repetition r times every variant once, `--inner` back-to-back calls
each -- so that clock and thermal drift falls on all of them alike.  Call k reads logits buffer k mod `--buffers`: the buffers
together exceed the 256 MB Infinity Cache, so no call finds its logits cached by the call before (`--buffers 1` shows the
cache-resident rate).  Printed: median and min .. max of the per-call time, the bytes (b) must move (logits once, mask words, slot
records, the three outputs), the fraction of the 8 TB/s HBM peak those bytes over the median time are, and one JSON line per shape.
No rate is printed without a GPU.

`--dtype bfloat16|float16` and `--temperature T`: the logits buffers hold that type (what a network under autocast emits) and the
variants are (c) env.sample_actions(x, temperature=T) / evaluate_actions(x, ..., temperature=T) on the 16-bit tensor against
(d) what a user wrote before the head took 16-bit logits, on the same tensor: x.float() * s, s = float32(1) / float32(T), then the
float32 head of this same build.  The bytes are then 2 per logit.

`--against PATH`: instead of the above, the float32 head of this build against ANOTHER build of the library (PATH: a
libgraphenvs_hip.so compiled from another commit, e.g. the parent's) -- both loaded into this one process, one engine each
(prefetch off) on the same box, the raw C entry points ge_policy_sample / ge_policy_evaluate / ge_policy_backward on the same
logits buffers, alternated like the other variants; outputs and gradient are compared bit for bit first."""
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


def half_rate(args, env, members, name, env_id, numel, nbuf, bufs, T, lb):
    """16-bit logits: the head on them against x.float() * s in front of the float32 head (module docstring, (c) and (d))"""
    import numpy as np
    s = torch.tensor(float(np.float32(1) / np.float32(T)), dtype=torch.float32, device="cuda")
    ragged, Bt = len(members) > 1 or members[0] is not env, env.num_envs
    a, lp, en = (v.clone() for v in env.sample_actions(bufs[0], 1, temperature=T))
    a2, lp2, en2 = env.sample_actions(bufs[0].float() * s, 1)
    assert torch.equal(a, a2) and torch.equal(lp, lp2) and torch.equal(en, en2), "the 16-bit head and the float32 head on x.float() * s differ"
    mask_flat = torch.cat([c.t["mask"].reshape(-1) for c in members])
    res = dict(shape=name, env_id=env_id, slots=Bt, logits=numel, buffers=nbuf, dtype=args.dtype, temperature=T)
    res.update(timed({
        "float_scale_then_sample_actions": lambda k: env.sample_actions(bufs[k % nbuf].float() * s, 1),
        "sample_actions": lambda k: env.sample_actions(bufs[k % nbuf], 1, temperature=T),
        "float_scale_then_evaluate_actions": lambda k: env.evaluate_actions(bufs[k % nbuf].float() * s, a, mask_flat),
        "evaluate_actions": lambda k: env.evaluate_actions(bufs[k % nbuf], a, mask_flat, temperature=T),
    }, args.reps, args.inner))
    res["bytes_sample"] = numel * lb + sum(c.num_envs * ((c.A + 63) // 64) * 8 for c in members) + Bt * 8 + Bt * 16 + (Bt * 4 if ragged else 0)
    res["bytes_evaluate"] = numel * (lb + 1) + Bt * 8 + Bt * 8 + (Bt * 4 if ragged else 0)
    res["hbm_frac_sample"] = res["bytes_sample"] / (res["sample_actions"]["median_us"] * 1e-6) / HBM_PEAK
    res["hbm_frac_evaluate"] = res["bytes_evaluate"] / (res["evaluate_actions"]["median_us"] * 1e-6) / HBM_PEAK
    res["speedup_vs_float_scale_sample"] = res["float_scale_then_sample_actions"]["median_us"] / res["sample_actions"]["median_us"]
    res["speedup_vs_float_scale_evaluate"] = res["float_scale_then_evaluate_actions"]["median_us"] / res["evaluate_actions"]["median_us"]
    for k in ("float_scale_then_sample_actions", "sample_actions", "float_scale_then_evaluate_actions", "evaluate_actions"):
        t = res[k]
        print(f"{name:13s} {k:34s} median {t['median_us']:9.1f} us   min {t['min_us']:9.1f}   max {t['max_us']:9.1f}", flush=True)
    print(f"{name:13s} {args.dtype} T={T}: sample_actions moves {res['bytes_sample'] / 1e6:.1f} MB = {100 * res['hbm_frac_sample']:.1f} % of the 8 TB/s HBM peak; "
          f"{res['speedup_vs_float_scale_sample']:.2f}x float-and-scale in front of the float32 head (evaluate: {res['speedup_vs_float_scale_evaluate']:.2f}x)", flush=True)
    print(json.dumps(res), flush=True)


class OtherBuild:
    """the library of another commit behind _lib.bind: the four *_as entry points, which a build from before ABI 8 lacks and this
    comparison never calls, become placeholders; any other missing symbol is the AttributeError it would be"""
    OPTIONAL = ("ge_policy_sample_as", "ge_policy_evaluate_as", "ge_policy_backward_as", "ge_policy_step_as")

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            if name not in self.OPTIONAL:
                raise
            from types import SimpleNamespace
            self.__dict__[name] = SimpleNamespace()
            return self.__dict__[name]


def against_rate(args, name):
    """float32 entry points of this build and of the library at args.against, alternated (module docstring)"""
    import ctypes as C

    from graphenvs_amd import _lib
    other = _lib.bind(OtherBuild(C.CDLL(os.path.abspath(args.against))))
    env_id, geo, B = SHAPES[name]
    make = (lambda **kw: ge.RaggedVectorEnv(env_id, geo, prefetch=0, **kw)) if B is None else (lambda **kw: ge.VectorGraphEnv(env_id, B, prefetch=0, **geo, **kw))
    envs = {"this": make(), "other": make(_library=other)}
    for e in envs.values():
        e.reset(seed=0); e.random_rollout(args.rollout, policy_seed=1)
    flat = lambda e: torch.cat([c.t["mask"].reshape(-1) for c in (e.classes if B is None else [e])])
    assert torch.equal(flat(envs["this"]), flat(envs["other"]))
    mask = flat(envs["this"]).clone().view(torch.uint8)
    numel, Bt = mask.numel(), envs["this"].num_envs
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    nbuf = args.buffers or max(2, -(-320_000_000 // (numel * 4)))
    bufs = [(torch.randn(numel, device="cuda", generator=g) * 2).clamp_(-8, 8) for _ in range(nbuf)]
    f = lambda n=Bt, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    outs = {k: dict(a=f(dt=torch.int64), lp=f(), en=f(), grad=f(numel)) for k in envs}
    gl, gh = torch.randn(Bt, device="cuda", generator=g), torch.randn(Bt, device="cuda", generator=g)
    acts = f(dt=torch.int64)

    def sample(k, w):
        e, o = envs[w], outs[w]
        assert e._L.ge_policy_sample(e._h, bufs[k % nbuf].data_ptr(), 1, 0, o["a"].data_ptr(), o["lp"].data_ptr(), o["en"].data_ptr(), e._stream()) == 0

    def evaluate(k, w):
        e, o = envs[w], outs[w]
        assert e._L.ge_policy_evaluate(e._h, bufs[k % nbuf].data_ptr(), mask.data_ptr(), acts.data_ptr(), o["lp"].data_ptr(), o["en"].data_ptr(), e._stream()) == 0

    def backward(k, w):
        e, o = envs[w], outs[w]
        assert e._L.ge_policy_backward(e._h, bufs[k % nbuf].data_ptr(), mask.data_ptr(), acts.data_ptr(), gl.data_ptr(), gh.data_ptr(),
                                       o["grad"].data_ptr(), e._stream()) == 0

    sample(0, "this"); sample(0, "other"); torch.cuda.synchronize()
    acts.copy_(outs["this"]["a"])
    evaluate(0, "this"); evaluate(0, "other"); backward(0, "this"); backward(0, "other"); torch.cuda.synchronize()
    for key in ("a", "lp", "en", "grad"):
        assert torch.equal(outs["this"][key], outs["other"][key]), f"{name}: {key} differs between the two builds"
    variants = {f"{fn.__name__}_{w}": (lambda k, fn=fn, w=w: fn(k, w)) for fn in (sample, evaluate, backward) for w in ("other", "this")}
    res = dict(shape=name, env_id=env_id, slots=Bt, logits=numel, buffers=nbuf, against=os.path.basename(args.against))
    res.update(timed(variants, args.reps, args.inner))
    for fn in ("sample", "evaluate", "backward"):
        o, t = res[f"{fn}_other"], res[f"{fn}_this"]
        print(f"{name:13s} {fn:9s} other build median {o['median_us']:8.1f} us ({o['min_us']:.1f} .. {o['max_us']:.1f})   this build median {t['median_us']:8.1f} us "
              f"({t['min_us']:.1f} .. {t['max_us']:.1f})   ratio {t['median_us'] / o['median_us']:.3f}   inside the other's min .. max: "
              f"{o['min_us'] <= t['median_us'] <= o['max_us']}", flush=True)
    print(json.dumps(res), flush=True)
    for e in envs.values():
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,config4,ragged3,ragged3-wide")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=0, help="logits buffers rotated through (0: as many as exceed 320 MB together)")
    ap.add_argument("--rollout", type=int, default=40, help="random steps before timing, so that masks have thinned out")
    ap.add_argument("--dtype", default="float32", choices=("float32", "bfloat16", "float16"), help="storage type of the logits")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--against", default=None, metavar="PATH", help="another build of libgraphenvs_hip.so: time this build's float32 head against it")
    args = ap.parse_args()
    dtype, T = getattr(torch, args.dtype), args.temperature
    lb = torch.empty((), dtype=dtype).element_size()  # bytes per logit
    if not torch.cuda.is_available():
        raise SystemExit("policy_head_rate: no GPU visible (a rate measured elsewhere says nothing about the MI355X)")
    for name in args.shapes.split(","):
        if args.against:
            against_rate(args, name)
            continue
        env_id, geo, B = SHAPES[name]
        ragged = B is None
        env = ge.RaggedVectorEnv(env_id, geo) if ragged else ge.VectorGraphEnv(env_id, B, **geo)
        env.reset(seed=0); env.random_rollout(args.rollout, policy_seed=1)
        members = env.classes if ragged else [env]
        numel = sum(c.num_envs * c.A for c in members)
        g = torch.Generator(device="cuda"); g.manual_seed(0)
        nbuf = args.buffers or max(2, -(-320_000_000 // (numel * lb)))
        bufs = [(torch.randn(numel, device="cuda", generator=g) * 2).clamp_(-8, 8).to(dtype) for _ in range(nbuf)]
        if dtype != torch.float32:
            half_rate(args, env, members, name, env_id, numel, nbuf, bufs, T, lb)
            env.close(); del env, bufs
            continue
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
            "sample_actions": lambda k: env.sample_actions(bufs[k % nbuf], 1, temperature=T),
            "sample_actions_greedy": lambda k: env.sample_actions(bufs[k % nbuf], 1, greedy=True, temperature=T),
            "evaluate_actions": lambda k: env.evaluate_actions(bufs[k % nbuf], a, mask_flat, temperature=T),
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
