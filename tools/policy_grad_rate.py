"""The policy head's gradient against the torch composition it replaces, forward AND backward, on the same engine, logits and box.

(a) what a user writes today: masked_fill(~mask, -inf) -> log_softmax -> gather -> entropy (the masked lp zeroed before it is multiplied,
    so that the backward is NaN-free), then torch.autograd of (logp, entropy) with upstream gradients of both; a multi-class engine
    loops that over the classes' [B_c, A_c] blocks;
(b) env.evaluate_actions(logits, actions, mask) on logits that require a gradient, then the same torch.autograd call: ge_policy_evaluate
    and ge_policy_backward, one launch each;
(c) the ge_policy_backward launch alone (the C call on preallocated tensors).
The method is tools/policy_head_rate.py's: every variant timed warm with HIP events in ALTERNATION on the same tensors, call k on logits
buffer k mod `--buffers` (together larger than the 256 MB Infinity Cache).  Printed: median and min .. max per call, the bytes (b) and
(c) must move -- forward: 4 B of logit and 1 B of mask per element; backward: those again and 4 B of gradient, 9 B per element -- and
the fraction of the 8 TB/s HBM peak those bytes over the median time are; one JSON line per shape.  No rate is printed without a GPU.

`--dtype bfloat16|float16` and `--temperature T`: the leaves hold that type and (b) / (c) run on them with the temperature (2 B of
logit and 2 B of gradient per element); (a) becomes what a user wrote before the head took 16-bit logits, on the same 16-bit leaf:
x.float() * s, s = float32(1) / float32(T), the float32 evaluate_actions of this same build, and autograd back to the leaf."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import graphenvs_amd as ge
from policy_head_rate import HBM_PEAK, SHAPES, timed


def torch_chain(blocks, s=None):
    """forward and backward of the composition per [B_c, A_c] block; blocks: (leaf logits, bool mask, actions, gl, gh); s: the
    float32 scalar 1 / temperature the logits are multiplied by first (None: 1)"""
    outs, ups = [], []
    for x, mask, a, gl, gh in blocks:
        lp = torch.log_softmax((x if s is None else x * s).masked_fill(~mask, float("-inf")), dim=1)
        outs += [lp.gather(1, a[:, None]).squeeze(1), -(lp.exp() * lp.masked_fill(~mask, 0.0)).sum(dim=1)]
        ups += [gl, gh]
    return torch.autograd.grad(outs, [b[0] for b in blocks], ups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,config4,ragged3,ragged3-wide")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--buffers", type=int, default=0, help="logits buffers rotated through (0: as many as exceed 320 MB together)")
    ap.add_argument("--rollout", type=int, default=40, help="random steps before timing, so that masks have thinned out")
    ap.add_argument("--dtype", default="float32", choices=("float32", "bfloat16", "float16"), help="storage type of the logits")
    ap.add_argument("--temperature", type=float, default=1.0)
    args = ap.parse_args()
    dtype, T = getattr(torch, args.dtype), args.temperature
    half = dtype != torch.float32
    lb = torch.empty((), dtype=dtype).element_size()  # bytes per logit
    if not torch.cuda.is_available():
        raise SystemExit("policy_grad_rate: no GPU visible (a rate measured elsewhere says nothing about the MI355X)")
    for name in args.shapes.split(","):
        env_id, geo, B = SHAPES[name]
        ragged = B is None
        env = ge.RaggedVectorEnv(env_id, geo) if ragged else ge.VectorGraphEnv(env_id, B, **geo)
        env.reset(seed=0); env.random_rollout(args.rollout, policy_seed=1)
        members = env.classes if ragged else [env]
        numel, Bt = sum(c.num_envs * c.A for c in members), env.num_envs
        g = torch.Generator(device="cuda"); g.manual_seed(0)
        nbuf = args.buffers or max(2, -(-320_000_000 // (numel * lb)))
        bufs = [(torch.randn(numel, device="cuda", generator=g) * 2).clamp_(-8, 8).to(dtype).requires_grad_(True) for _ in range(nbuf)]
        s32 = torch.tensor(float(np.float32(1) / np.float32(T)), dtype=torch.float32, device="cuda")
        scale_t = None if T == 1.0 else s32  # (float32 logits with a temperature: the torch composition scales its logits too)
        mask_flat = torch.cat([c.mask.reshape(-1) for c in members]).clone()  # (bool)
        a = env.sample_actions(bufs[0].detach(), 1, temperature=T)[0].clone()
        gl, gh = torch.randn(Bt, device="cuda", generator=g), torch.randn(Bt, device="cuda", generator=g)
        sets = []  # per buffer: the (leaf logits, bool mask, actions clamped into the row, gl, gh) blocks of the classes
        for logits in bufs:
            blocks, off, slot = [], 0, 0
            for c in members:
                n = c.num_envs * c.A
                x = logits.detach()[off:off + n].view(c.num_envs, c.A).requires_grad_(True)  # (the buffer's memory, a leaf of its own)
                sl = slice(slot, slot + c.num_envs)
                blocks.append((x, mask_flat[off:off + n].view(c.num_envs, c.A), a[sl].clamp(min=0), gl[sl], gh[sl]))
                off += n; slot += c.num_envs
            sets.append(blocks)

        def ours(k):
            x = bufs[k % nbuf]
            return torch.autograd.grad(env.evaluate_actions(x, a, mask_flat, temperature=T), x, (gl, gh))[0]

        def float_scale(k):  # (16-bit leaves: the casts and the scale as passes of their own, around the float32 head)
            x = bufs[k % nbuf]
            return torch.autograd.grad(env.evaluate_actions(x.float() * s32, a, mask_flat), x, (gl, gh))[0]

        # (a row whose mask has emptied gives NaN in the torch chain -- log_softmax of all -inf; its time is the same and the
        # comparison below leaves such rows out.)  Same masked softmax: on the rows that drew an action the two gradients agree to float32 rounding
        live = (a >= 0).repeat_interleave(torch.cat([torch.full((c.num_envs,), c.A, device="cuda") for c in members]))
        if half:
            err = 0.0
            assert torch.equal(ours(0).view(torch.int16), float_scale(0).view(torch.int16)), f"{name}: the 16-bit gradient words differ from the float32 path's"
        else:
            err = float((ours(0) - torch.cat([v.reshape(-1) for v in torch_chain(sets[0], scale_t)]))[live].abs().max())
        # (both sides are float32 within the band of tests/policy_grad_check.py of the same float64 value: around 1e-6 here, and a
        # wrong pairing of rows, masks or upstream gradients shows as a difference of the gradients' own size, ~1)
        assert err < 1e-3, f"{name}: evaluate_actions' gradient and the torch composition's differ by {err}"
        out = torch.empty(numel, device="cuda", dtype=dtype)
        code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]
        L, mk8 = env._L, mask_flat.view(torch.uint8)

        def kernel(k):
            rc = L.ge_policy_backward_as(env._h, bufs[k % nbuf].data_ptr(), code, float(s32), mk8.data_ptr(), a.data_ptr(), gl.data_ptr(), gh.data_ptr(),
                                         out.data_ptr(), env._stream())
            assert rc == 0

        res = dict(shape=name, env_id=env_id, slots=Bt, logits=numel, buffers=nbuf, grad_max_abs_diff_vs_torch=err, dtype=args.dtype, temperature=T,
                   baseline="float_scale_f32_head" if half else "torch_composition")  # (what the key torch_fwd_bwd timed)
        res.update(timed({"torch_fwd_bwd": float_scale if half else (lambda k: torch_chain(sets[k % nbuf], scale_t)), "evaluate_actions_fwd_bwd": ours,
                          "ge_policy_backward": kernel}, args.reps, args.inner))
        extra = Bt * 4 if ragged else 0
        res["bytes_forward"] = numel * (lb + 1) + Bt * 16 + extra
        res["bytes_backward"] = numel * (2 * lb + 1) + Bt * 16 + extra
        res["hbm_frac_fwd_bwd"] = (res["bytes_forward"] + res["bytes_backward"]) / (res["evaluate_actions_fwd_bwd"]["median_us"] * 1e-6) / HBM_PEAK
        res["hbm_frac_backward"] = res["bytes_backward"] / (res["ge_policy_backward"]["median_us"] * 1e-6) / HBM_PEAK
        res["speedup_vs_torch"] = res["torch_fwd_bwd"]["median_us"] / res["evaluate_actions_fwd_bwd"]["median_us"]
        for k in ("torch_fwd_bwd", "evaluate_actions_fwd_bwd", "ge_policy_backward"):
            t = res[k]
            k = "float_scale_f32_head_fwd_bwd" if half and k == "torch_fwd_bwd" else k
            print(f"{name:13s} {k:26s} median {t['median_us']:9.1f} us   min {t['min_us']:9.1f}   max {t['max_us']:9.1f}", flush=True)
        print(f"{name:13s} forward + backward move {(res['bytes_forward'] + res['bytes_backward']) / 1e6:.1f} MB = {100 * res['hbm_frac_fwd_bwd']:.1f} % of the "
              f"8 TB/s HBM peak, the backward launch alone {res['bytes_backward'] / 1e6:.1f} MB = {100 * res['hbm_frac_backward']:.1f} %; "
              f"{res['speedup_vs_torch']:.2f}x " + ("float-and-scale around the float32 head" if half else "the torch composition"), flush=True)
        print(json.dumps(res), flush=True)
        env.close(); del env, sets, bufs, out


if __name__ == "__main__":
    main()
