"""Bodies shared by the CPU-harness tests (tests/test_policy_dtype.py) and the GPU tests (tests/test_gpu_policy_dtype.py) of the policy
head on bfloat16 / float16 logits with a temperature: ge_policy_sample_as / _evaluate_as / _backward_as / _step_as behind
sample_actions / evaluate_actions / step_policy (kernel: graphenvs_amd/csrc/ge_policy.h, contract: DESIGN.md 5).

There is no tolerance in this file.  The contract is an identity between two paths of the SAME library: a 16-bit element is converted
to float32 (exact), multiplied by scale = float32(1) / float32(temperature) and the product rounded to float32 once; the float32
path given x.float() * scale (torch does the same two operations, as passes over memory) starts from the same float32 values and
runs the same (chunk, lane) arithmetic.  So
 - forward (sample, greedy, evaluate, step_policy): every output equals the float32 path's under torch.equal (-inf included);
 - gradient: grad has the logits' dtype and its 16-bit words equal, as int16, those torch.autograd gives the 16-bit leaf through
   x.float() * scale and the float32 path -- the float32 gradient times scale (one float32 multiply), rounded to nearest even.
What the float32 path itself computes is checked against float64 in tests/policy_head_check.py and tests/policy_grad_check.py.

Anchors that need no second path: a masked element's gradient word is +0.0 (0x0000) exactly; a row with one valid action has logp
0.0, entropy 0.0 and a gradient that is zero in every element (of either sign: gl * (1 - 1) with gl < 0 is -0.0 in the float32
contract already, and rounds to the 16-bit -0.0; DESIGN.md 5 says so); temperature=1.0 on float32 logits is the call without the keyword."""
import numpy as np
import pytest
import torch

import fused_check as fc
import policy_head_check as pc

DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]
TEMPERATURES = [1.0, 0.7, 3.0]
CASE_IDS = ("a5-subwave-unaligned", "a33-group64", "a64-full-wave", "a70-two-chunks", "a200-aw4", "a2048-config4", "a2080-read-twice")
CASES = [c for c in pc.CASES if c.id in CASE_IDS]
RAGGED = [c for c in pc.RAGGED if c.id in ("sp-3-classes", "sp-3-classes-subwave")]
assert len(CASES) == len(CASE_IDS) and len(RAGGED) == 2
POISON = 0x7FC1  # a NaN word of both 16-bit types
SEED = pc.POLICY_SEED
K_STEP_POLICY = 6


def scale_of(temperature):
    """what the host hands the engine (EngineHandle.sample_actions documents exactly this)"""
    return float(np.float32(1) / np.float32(temperature))


def _dev(device):
    return torch.device(device)


def _x16(x_np, dtype, device):
    """float32 values rounded to the dtype ONCE: the tensor both paths start from"""
    return torch.from_numpy(x_np).to(dtype).to(_dev(device))


def _as_f32(x16, temperature, device):
    """what a user writes in front of the float32 path: x.float() * s, s a float32 scalar"""
    return x16.float() * torch.tensor(scale_of(temperature), dtype=torch.float32, device=_dev(device))


def _clone3(out):
    return tuple(v.clone() for v in out)  # (the three tensors are engine-owned and overwritten by the next call)


def _same3(got, want, what):
    for name, g, w in zip(("actions", "logp", "entropy"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), (what, name, int((g != w).sum()))


def check_forward(eng, device, dtype, T, rng, k):
    """sample and greedy on (x16, T) against the float32 path on x16.float() * s; evaluate on the cloned mask with the drawn and with
    planted actions.  Returns (x16, mask, planted actions) for the gradient check"""
    env, blocks = eng.env, eng.blocks()
    x_np, _ = pc.logit_set("normal", rng, blocks)
    x16 = _x16(x_np, dtype, device)
    x32 = _as_f32(x16, T, device)
    got = _clone3(env.sample_actions(x16, SEED + k, temperature=T))
    _same3(got, env.sample_actions(x32, SEED + k), "sample")
    act, lp, en = got
    drew = act >= 0
    assert int(drew.sum()) > 0
    # greedy on multiples of 0.5 (exact in both 16-bit types, ties survive the rounding and the positive scale): also the lowest
    # valid index of the largest element, whatever the temperature
    h_np, _ = pc.logit_set("half", rng, blocks)
    h16 = _x16(h_np, dtype, device)
    assert np.array_equal(pc._np(h16.float()), h_np)
    ggot = _clone3(env.sample_actions(h16, SEED + k, greedy=True, temperature=T))
    _same3(ggot, env.sample_actions(_as_f32(h16, T, device), SEED + k, greedy=True), "greedy")
    ga, off, ties = pc._np(ggot[0]), 0, 0
    for b in blocks:
        B, A, s0 = b["B"], b["A"], b["slot"]
        top = np.where(b["mask"], h_np[off:off + B * A].reshape(B, A), -np.inf); off += B * A
        live = b["mask"].any(axis=1) & (b["status"] != 1) & (b["status"] != 4)
        assert np.array_equal(ga[s0:s0 + B][live], top.argmax(axis=1)[live]), "greedy: the lowest valid index of the maximum"
        ties += int(((top == top.max(axis=1, keepdims=True)).sum(axis=1) > 1)[live].sum())
    assert ties > 0, "the greedy check met no tie"
    # evaluate re-scores the sample call bit for bit on the 16-bit input
    mask = eng.mask_flat().clone()
    elp, een = env.evaluate_actions(x16, act, mask.view(torch.bool), temperature=T)
    assert torch.equal(elp[drew], lp[drew]) and torch.equal(een[drew], en[drew]), "evaluate_actions != the sample_actions call it re-scores"
    assert bool(torch.isneginf(elp[~drew]).all())
    # planted actions: -1, out of range, masked out; one row with a single valid action (the mask is the caller's)
    acts, mask_np = pc._np(act).copy(), pc._np(mask).astype(bool).copy()
    bad, single, off = [], [], 0
    for b in blocks:
        B, A, s0 = b["B"], b["A"], b["slot"]
        rows = mask_np[off:off + B * A].reshape(B, A)  # (a view: the planted row lands in mask_np)
        # rows 0, 1 (and 2 where the block has more than three rows) get the three kinds in turn, starting at kind k: the two passes
        # of a three-row block meet all of them
        for r in range(min(3, B - 1)):
            kind = (k + r) % 3
            masked_out = np.flatnonzero(~rows[r])
            if kind == 2 and not len(masked_out):
                continue
            acts[s0 + r] = (-1, A, masked_out[-1] if len(masked_out) else 0)[kind]
            bad.append(s0 + r)
        j = int(rng.integers(A))
        rows[B - 1] = False; rows[B - 1, j] = True
        acts[s0 + B - 1] = j; single.append(s0 + B - 1)
        off += B * A
    acts_t, mask_t = torch.from_numpy(acts).to(_dev(device)), torch.from_numpy(mask_np).to(_dev(device))
    e16 = _clone3(env.evaluate_actions(x16, acts_t, mask_t, temperature=T))
    e32 = env.evaluate_actions(x32, acts_t, mask_t)
    for name, g, w in zip(("logp", "entropy"), e16, e32):
        assert torch.equal(g, w), ("evaluate", name)
    assert bool(torch.isneginf(e16[0][bad]).all())
    assert bool((e16[0][single] == 0.0).all()) and bool((e16[1][single] == 0.0).all()), "one valid action: logp 0.0 and entropy 0.0"
    return x16, mask_t, acts_t, single


def check_gradient(eng, device, dtype, T, rng, x16, mask, acts, single):
    """autograd through evaluate_actions(x16, temperature=T) against autograd through x16.float() * s and the float32 path"""
    env, dev = eng.env, _dev(device)
    B = env.num_envs
    gl = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev)
    gh = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev)
    assert bool((gl != 0).all())  # (rows with an invalid action carry a logp weight too: the kernel has to drop it)
    a_leaf, b_leaf = x16.clone().requires_grad_(), x16.clone().requires_grad_()
    torch.autograd.backward(list(env.evaluate_actions(a_leaf, acts, mask, temperature=T)), [gl, gh])
    s32 = torch.tensor(scale_of(T), dtype=torch.float32, device=dev)
    torch.autograd.backward(list(env.evaluate_actions(b_leaf.float() * s32, acts, mask)), [gl, gh])
    ga, gb = a_leaf.grad, b_leaf.grad
    assert ga.dtype == dtype and gb.dtype == dtype and ga.shape == x16.shape
    wa, wb = ga.view(torch.int16), gb.view(torch.int16)
    diff = wa != wb
    assert not bool(diff.any()), ("gradient words differ", int(diff.sum()), pc._np(torch.nonzero(diff)[:4]).tolist())
    assert bool(torch.isfinite(ga.float()).all()) and bool((wa != 0).any())
    # the same launch into a buffer that holds NaN words: every element is written
    out = torch.full((x16.numel(),), POISON, dtype=torch.int16, device=dev)
    code = {torch.bfloat16: 1, torch.float16: 2}[dtype]
    m8 = mask.view(torch.uint8)
    rc = env._L.ge_policy_backward_as(env._h, x16.data_ptr(), code, scale_of(T), m8.data_ptr(), acts.data_ptr(), gl.data_ptr(), gh.data_ptr(),
                                      out.data_ptr(), env._stream())
    assert rc == 0
    env._quiesce()
    assert not bool((out == POISON).any()), "an element of grad_logits kept what the buffer held"
    assert torch.equal(out, wa.reshape(-1))
    # anchors: a masked element is +0.0 exactly; the row with one valid action has a zero gradient
    assert bool((wa.reshape(-1)[~mask.reshape(-1)] == 0).all()), "a masked element's gradient word is not +0.0"
    off = 0
    flat = wa.reshape(-1)
    members = eng.members
    starts = np.cumsum([0] + [c.num_envs for c in members])
    for c, s0 in zip(members, starts):
        for i in single:
            if s0 <= i < s0 + c.num_envs:
                row = flat[off + (i - s0) * c.A: off + (i - s0 + 1) * c.A]
                assert bool(((row & 0x7FFF) == 0).all()), "one valid action: the row's gradient is not zero"
        off += c.num_envs * c.A


def check_fp32_anchor(eng, device, rng, k):
    """temperature=1.0 on float32 logits returns exactly what the call without the keyword returns"""
    env = eng.env
    x_np, _ = pc.logit_set("normal", rng, eng.blocks())
    x = torch.from_numpy(x_np).to(_dev(device))
    _same3(_clone3(env.sample_actions(x, SEED + k, temperature=1.0)), env.sample_actions(x, SEED + k), "float32, temperature 1.0")
    act, mask = env.sample_actions(x, SEED + k)[0].clone(), eng.mask_flat().clone().view(torch.bool)
    want = _clone3(env.evaluate_actions(x, act, mask))
    got = env.evaluate_actions(x, act, mask, temperature=1.0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def check_engine(make, device, dtype, T, steps=3, shared=None, key=None):
    """every check on a reset engine, and again after `steps` steps (the draw is keyed by the slot's transition count).  `shared`: a
    dict that keeps the engine of `key` for the other (dtype, temperature) entries of the same case -- in the CPU harness a reset of
    the 2 048-action rows takes ten seconds and a policy call a fraction of one; the first test of a case to run finds the engine
    freshly reset, the others some steps further on, and whoever owns the dict closes the engines"""
    env = shared.get(key) if shared is not None else None
    if env is None:
        env = make()
        env.reset(seed=pc.S0)
        if shared is not None:
            shared[key] = env
    eng = pc.Engine(env)
    rng = np.random.default_rng(4321)
    for phase in range(2):
        if phase:
            for j in range(steps):
                env.step(env.sample_random_actions(policy_seed=11 + j).clone())
        # where a failure happened: a shared engine is as many transitions past its reset as the entries before this one left it, so
        # the entry fails alone (-k) only if it fails on a fresh engine; the transition count says which state to go back to
        at = f"[pass {phase}, slot 0 is {int(eng.blocks()[0]['tstep'][0])} transitions past reset(seed={pc.S0}), {steps} random steps (policy_seed 11..) between passes]"
        try:
            saved = check_forward(eng, device, dtype, T, rng, phase)
            check_gradient(eng, device, dtype, T, rng, *saved)
            check_fp32_anchor(eng, device, rng, phase)
        except AssertionError as e:
            raise AssertionError(f"{e} {at}") from e
    flags = int((env.g if hasattr(env, "g") else env.t)["work_count"][1].item())
    assert flags == 0, f"device error flags {flags:#x}"
    if shared is None:
        env.close()


def check_uniform(ge, device, lib, env_id, kw, B, dtype, T, **share):
    make = lambda: ge.VectorGraphEnv(env_id, B, seed_stride=pc.STRIDE, env_index_base=pc.BASE, **pc._extra(device, lib), **kw)
    check_engine(make, device, dtype, T, **share)


def check_ragged(ge, device, lib, env_id, sizes, prefetch, dtype, T, **share):
    make = lambda: ge.RaggedVectorEnv(env_id, sizes, seed_stride=pc.STRIDE, env_index_base=pc.BASE, prefetch=prefetch, **pc._extra(device, lib))
    check_engine(make, device, dtype, T, **share)


def _flat_obs(env):
    v = env.flat_obs()
    return torch.cat([t.reshape(-1) for t in v]) if isinstance(v, (list, tuple)) else v


def check_step_policy(ge, device, make, dtype, T, K=K_STEP_POLICY):
    """two engines built and reset alike, one fed (x16, T) through step_policy, the other x16.float() * s: after every step the
    outputs, the flat observation and every live slab are equal"""
    a, b = make(), make()
    a.reset(seed=pc.S0); b.reset(seed=pc.S0)
    eng, rng = pc.Engine(a), np.random.default_rng(7)
    moved = 0
    for k in range(K):
        x_np, _ = pc.logit_set("normal", rng, eng.blocks())
        x16 = _x16(x_np, dtype, device)
        oa = a.step_policy(x16, SEED + k, temperature=T)
        ob = b.step_policy(_as_f32(x16, T, device), SEED + k)
        ia, ib = oa[4], ob[4]
        for key in ("action", "logp", "entropy", "solved", "solution_cost", "heuristic_solution", "invalid_action", "episode_length"):
            assert torch.equal(ia[key], ib[key]), (k, key)
        assert torch.equal(oa[1], ob[1]) and torch.equal(oa[2], ob[2]) and torch.equal(oa[3], ob[3]), k  # reward, terminated, truncated
        assert torch.equal(pc.Engine(a).mask_flat(), pc.Engine(b).mask_flat()), k
        assert torch.equal(_flat_obs(a), _flat_obs(b)), k
        moved += int((ia["action"] >= 0).sum())
        skip = set(fc._prefetch_skip()) if getattr(a, "spare", None) is not None else set()
        fc._same_slabs(pc._slabs(a), pc._slabs(b), skip, k)
    assert moved > 0
    a.close(); b.close()


def check_halves_equal_one(one, parts, device, dtype, T):
    """`parts` (two engines over the halves of `one`'s slots behind a MixedVectorEnv) gives, on the same 16-bit logits and temperature,
    bit for bit what `one` gives: sample_actions, evaluate_actions, the gradient words and step_policy"""
    members = parts.members
    assert len(members) == 2 and sum(m.num_envs for m in members) == one.num_envs
    one.reset(seed=pc.S0); parts.reset(seed=pc.S0)
    rng, dev = np.random.default_rng(3), _dev(device)
    cat = lambda vs: torch.cat(list(vs))
    cuts = np.cumsum([0] + [m.num_envs for m in members])
    for k in range(3):
        x_np, _ = pc.logit_set("normal", rng, pc.Engine(one).blocks())
        x = _x16(x_np, dtype, device).view(one.num_envs, one.A)
        xs = [x[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        want = _clone3(one.sample_actions(x, SEED + k, temperature=T))
        outs = parts.sample_actions(xs, SEED + k, temperature=T)
        _same3(tuple(cat(o[j] for o in outs) for j in range(3)), want, ("halves", k))
        act, mask = want[0], one.mask.clone()
        gl = torch.from_numpy(rng.normal(size=one.num_envs).astype(np.float32)).to(dev)
        gh = torch.from_numpy(rng.normal(size=one.num_envs).astype(np.float32)).to(dev)
        leaf = x.clone().requires_grad_()
        ev_one = one.evaluate_actions(leaf, act, mask, temperature=T)
        torch.autograd.backward(list(ev_one), [gl, gh])
        leaves = [v.clone().requires_grad_() for v in xs]
        ev = parts.evaluate_actions(leaves, [act[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])], [mask[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])],
                                    temperature=T)
        assert torch.equal(cat(e[0] for e in ev), ev_one[0]) and torch.equal(cat(e[1] for e in ev), ev_one[1]), k
        torch.autograd.backward([t for e in ev for t in e], [g[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:]) for g in (gl, gh)])
        assert leaf.grad.dtype == dtype and torch.equal(cat(v.grad for v in leaves).view(torch.int16), leaf.grad.view(torch.int16)), k
        w = one.step_policy(x, SEED + k, temperature=T)
        got = parts.step_policy(xs, SEED + k, temperature=T)
        for name in ("action", "logp", "entropy"):
            assert torch.equal(cat(i[name] for i in got[4]), w[4][name]), (k, name)
        for j in (1, 2, 3):
            assert torch.equal(cat(got[j]), w[j]), (k, j)
    one.close(); parts.close()


def check_errors(ge, device, lib):
    env = ge.VectorGraphEnv(pc._SP, 6, n_nodes=10, n_edges=20, **pc._extra(device, lib))
    dev = _dev(device)
    env.reset(seed=1)
    good = torch.zeros(6, 10, dtype=torch.bfloat16, device=dev)
    act, mask = env.sample_actions(good, temperature=2.0)[0].clone(), env.mask.clone()
    with pytest.raises(TypeError, match="float32"):
        env.sample_actions(good.double())
    with pytest.raises(TypeError, match="float32"):
        env.evaluate_actions(good.double(), act, mask)
    with pytest.raises(ValueError, match="elements"):
        env.sample_actions(torch.zeros(6, 9, dtype=torch.bfloat16, device=dev))
    for bad in (0, -1, float("inf"), float("nan")):
        for call in (lambda t: env.sample_actions(good, temperature=t), lambda t: env.step_policy(good, temperature=t),
                     lambda t: env.evaluate_actions(good, act, mask, temperature=t)):
            with pytest.raises(ValueError, match="temperature"):
                call(bad)
    # the raw entry points: GE_E_BADARG (-1) for a dtype outside GE_LOGITS_* and for a scale that is not finite or not > 0
    L, h, st = env._L, env._h, env._stream()
    lp, en, grad = torch.zeros(6, device=dev), torch.zeros(6, device=dev), torch.zeros(6, 10, dtype=torch.bfloat16, device=dev)
    m8 = mask.view(torch.uint8)
    for code, scale in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (1, float("inf")), (1, float("nan"))):
        assert L.ge_policy_sample_as(h, good.data_ptr(), code, scale, 0, 0, act.data_ptr(), lp.data_ptr(), en.data_ptr(), st) == -1
        assert b"scale" in L.ge_last_error() or b"logits_dtype" in L.ge_last_error()
        assert L.ge_policy_step_as(h, good.data_ptr(), code, scale, 0, 0, act.data_ptr(), lp.data_ptr(), en.data_ptr(), st) == -1
        assert L.ge_policy_evaluate_as(h, good.data_ptr(), code, scale, m8.data_ptr(), act.data_ptr(), lp.data_ptr(), en.data_ptr(), st) == -1
        assert L.ge_policy_backward_as(h, good.data_ptr(), code, scale, m8.data_ptr(), act.data_ptr(), None, None, grad.data_ptr(), st) == -1
    assert L.ge_policy_sample_as(h, good.data_ptr(), 1, 0.5, 0, 0, act.data_ptr(), None, None, st) == 0  # logp and entropy may be NULL
    env._quiesce()
    env.close()
