"""Bodies shared by the CPU-harness tests (tests/test_policy_head.py) and the GPU tests (tests/test_gpu_policy_head.py) of the masked
categorical policy head: ge_policy_sample / ge_policy_evaluate / ge_policy_step behind EngineHandle.sample_actions /
evaluate_actions / step_policy (kernel: graphenvs_amd/csrc/ge_policy.h, contract: DESIGN.md 5).

Reference.  numpy float64 from the float32 logits and the engine's own mask bytes: p = softmax over the valid actions,
F_lo(a) = sum of p over the valid b < a, F_hi(a) = F_lo(a) + p[a], logp = log p, entropy = -sum p log p.  The uniform u of a slot is
recomputed exactly: z = mix64(policy_seed + gi * 0x9E3779B97F4A7C15 + ts * 0xD1B54A32D192ED03) (mod 2^64; mix64 is restated below),
gi = env_index_base + slot, ts = the slot's transition count, u = (z >> 40) * 2^-24.

Error model (float32 kernel against the float64 reference).  expf and logf are good to about 1 ulp; d[a] = l[a] - mx carries one
rounding of size 2^-24 |d|, which expf turns into a relative error of 2^-24 |d| in w[a]; a float32 sum of A non-negative terms is
good to A 2^-24 relative in any association order.  With R = max |d| over the row's valid actions every w[a], Z and every prefix
sum is therefore good to 2^-24 (A + 2 + R) relative, a ratio of two of them to twice that, hence
    eps = 2^-23 (A + 4 + R)
bounds the error of every F the kernel compares u * Z against, relative to Z.  Acceptance, for EVERY slot: the sampled action is
valid and F_lo(a) - eps <= u <= F_hi(a) + eps; logp and entropy are within eps (1 + R) absolute (logp = d - log Z: eps from log Z,
2^-24 R from d; the entropy adds sum p |d| <= R times the relative error of p).  Idle slots (no valid action, or status 1 / 4) are
exact: -1, 0.0, 0.0.  Exact anchors besides: greedy actions on logits quantised to multiples of 0.5 (ties occur: the lowest valid
index of the maximum), rows with one valid action (that action, logp 0.0, entropy 0.0), and -- logits all zero but one valid action
raised by 20 -- the raised action in every row: the others hold e^-20 ~ 2e-9 of the mass each."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_check as fc

STRIDE, BASE, S0 = fc.STRIDE, fc.BASE, fc.S0
K_STEPS = 12
POLICY_SEED = 0x5EED0123456789AB  # (the key arithmetic wraps around 2^64)

# row-length thresholds of ge_k_policy_head: the lane group of a row is the power of two covering A (4, 8, 16, 32, 64: a case on
# each side of 4 | 5, 8 | 9, 16 | 17, 32 | 33); above 64 actions a wave per row in chunks of 64 (64 | 70), held in registers by the
# instantiation for 1, 2, 4, 8, 16 or 32 chunks that covers the row (64 | 70, 128 | 130, 256 | 258, 512 | 514, 1 024 | 1 026); rows above
# GE_POL_REG_CHUNKS * 64 = 2 048 actions are read twice (2 048 | 2 080); the mask words of such a row are fetched 64 at a time
# (4 096 | 4 120 actions)
_SP, _MIS, _ST, _DC = "ShortestPath-v0", "MaxIndependentSet-v0", "SteinerTree-v0", "DistributionCenter-v0"
# (env id, kwargs, slots on the GPU, slots in the CPU harness: 70 for the rows of up to 200 actions, 3 above; 20 -- two waves of rows,
# the second partial -- for the group-width cases, whose code path the 70-slot cases share)
CASES = [
    pytest.param(_SP, dict(n_nodes=5, n_edges=7), 300, 70, id="a5-subwave-unaligned"),
    pytest.param(_SP, dict(n_nodes=64, n_edges=192), 300, 70, id="a64-full-wave"),
    pytest.param(_MIS, dict(n_nodes=70, n_edges=200), 300, 70, id="a70-two-chunks"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=100, n_dests=5), 300, 70, id="a200-aw4"),
    pytest.param(_ST, dict(n_nodes=256, n_edges=1024, n_dests=8), 260, 3, id="a2048-config4"),
    pytest.param(_ST, dict(n_nodes=260, n_edges=1040, n_dests=8), 260, 3, id="a2080-read-twice"),
    pytest.param(_SP, dict(n_nodes=4, n_edges=4), 300, 20, id="a4-group4"),
    pytest.param(_SP, dict(n_nodes=8, n_edges=12), 300, 20, id="a8-group8"),
    pytest.param(_SP, dict(n_nodes=9, n_edges=14), 300, 20, id="a9-group16"),
    pytest.param(_SP, dict(n_nodes=16, n_edges=32), 300, 20, id="a16-group16"),
    pytest.param(_SP, dict(n_nodes=17, n_edges=34), 300, 20, id="a17-group32"),
    pytest.param(_SP, dict(n_nodes=32, n_edges=80), 300, 20, id="a32-group32"),
    pytest.param(_SP, dict(n_nodes=33, n_edges=80), 300, 20, id="a33-group64"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=64, n_dests=5), 300, 3, id="a128-regs2"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=65, n_dests=5), 300, 3, id="a130-regs4"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=128, n_dests=5), 300, 3, id="a256-regs4"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=129, n_dests=5), 300, 3, id="a258-regs8"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=256, n_dests=5), 260, 3, id="a512-regs8"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=257, n_dests=5), 260, 3, id="a514-regs16"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=512, n_dests=5), 260, 3, id="a1024-regs16"),
    pytest.param(_ST, dict(n_nodes=40, n_edges=513, n_dests=5), 260, 3, id="a1026-regs32"),
    pytest.param(_ST, dict(n_nodes=66, n_edges=2048, n_dests=8), 130, 3, id="a4096-mask-words-once"),
    pytest.param(_ST, dict(n_nodes=66, n_edges=2060, n_dests=8), 130, 3, id="a4120-mask-words-twice"),
]
RAGGED = [
    pytest.param(_SP, [(70, 12, 30), (130, 64, 192), (100, 100, 300)], 0, id="sp-3-classes"),
    pytest.param(_ST, [(70, 12, 30, dict(n_dests=3)), (130, 64, 144, dict(n_dests=6)), (100, 100, 300, dict(n_dests=99))], 0, id="st-3-classes"),
    pytest.param(_ST, [(70, 12, 30, dict(n_dests=3)), (130, 64, 144, dict(n_dests=6)), (100, 100, 300, dict(n_dests=99))], 4, id="st-3-classes-prefetch4"),
    # every class within 64 actions: rows of three classes share a wave (lane groups of 16)
    pytest.param(_SP, [(70, 5, 7), (130, 12, 30), (100, 16, 32)], 0, id="sp-3-classes-subwave"),
]


def _mix64(z):
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def uniform_of(policy_seed, gi, ts):
    z = _mix64((policy_seed + gi * 0x9E3779B97F4A7C15 + ts * 0xD1B54A32D192ED03) & ((1 << 64) - 1))
    return (z >> 40) * 2.0 ** -24


def _np(v):
    return v.detach().cpu().numpy()


def _extra(device, lib):
    return dict(device=device, _library=lib) if lib is not None else dict(device=device)


def reference(logits, valid):
    """float64 softmax over the valid actions of every row: dict of p, F_lo, F_hi, logp [B, A], entropy, R, eps, any [B]"""
    l = logits.astype(np.float64)
    any_ = valid.any(axis=1)
    mx = np.where(valid, l, -np.inf).max(axis=1)
    mx = np.where(any_, mx, 0.0)
    d = np.where(valid, l - mx[:, None], 0.0)
    w = np.where(valid, np.exp(d), 0.0)
    Z = np.where(any_, w.sum(axis=1), 1.0)
    p = w / Z[:, None]
    F_hi = np.cumsum(p, axis=1)
    R = np.abs(d).max(axis=1)
    eps = 2.0 ** -23 * (logits.shape[1] + 4 + R)
    return dict(p=p, F_lo=F_hi - p, F_hi=F_hi, logp=d - np.log(Z)[:, None], entropy=np.log(Z) - (w * d).sum(axis=1) / Z, R=R, eps=eps, any=any_)


class Engine:
    """a VectorGraphEnv or a RaggedVectorEnv seen as blocks of rows: (first slot, env_index_base of it, mask, status, tstep) per class"""

    def __init__(self, env):
        self.env = env
        self.members = list(env.classes) if hasattr(env, "classes") else [env]
        self.numel = sum(c.num_envs * c.A for c in self.members)

    def blocks(self):
        out, slot = [], 0
        for c in self.members:
            out.append(dict(slot=slot, B=c.num_envs, A=c.A, base=c.env_index_base, mask=_np(c.t["mask"]).astype(bool),
                            status=_np(c.t["status"]).astype(np.int64), tstep=_np(c.t["tstep"]).astype(np.uint64)))
            slot += c.num_envs
        return out

    def mask_flat(self):
        return torch.cat([c.t["mask"].reshape(-1) for c in self.members])


def logit_set(kind, rng, blocks):
    """one flat float32 logits array in the engine's layout.  Returns (logits, raised): raised[slot] is the action raised by 20 (-1: none)"""
    parts, raised = [], []
    for b in blocks:
        B, A = b["B"], b["A"]
        r = np.full(B, -1, dtype=np.int64)
        if kind == "normal":
            x = np.clip(rng.normal(0.0, 2.0, size=(B, A)), -8.0, 8.0).astype(np.float32)
        elif kind == "half":  # multiples of 0.5 in [-2, 2]: ties occur
            x = (rng.integers(-4, 5, size=(B, A)) * 0.5).astype(np.float32)
        else:
            x = np.zeros((B, A), dtype=np.float32)
        if kind == "raised":
            for i in range(B):
                v = np.flatnonzero(b["mask"][i])
                if len(v):
                    r[i] = v[rng.integers(len(v))]
                    x[i, r[i]] = 20.0
        parts.append(x.reshape(-1)); raised.append(r)
    return np.concatenate(parts), np.concatenate(raised)


def check_outputs(blocks, logits, policy_seed, greedy, actions, logp, entropy, stats, raised=None):
    """the acceptance of the module docstring for every slot of every block"""
    off = 0
    for b in blocks:
        B, A, s0 = b["B"], b["A"], b["slot"]
        x = logits[off:off + B * A].reshape(B, A); off += B * A
        ref = reference(x, b["mask"])
        act, lp, en = actions[s0:s0 + B], logp[s0:s0 + B], entropy[s0:s0 + B]
        idle = ~ref["any"] | (b["status"] == 1) | (b["status"] == 4)
        assert (act[idle] == -1).all() and (lp[idle] == 0.0).all() and (en[idle] == 0.0).all(), "idle slots return -1, 0.0, 0.0"
        live = np.flatnonzero(~idle)
        stats["idle"] += int(idle.sum()); stats["rows"] += B
        if not len(live):
            continue
        a = act[live]
        assert ((a >= 0) & (a < A)).all() and b["mask"][live, a].all(), "a sampled action is a valid action"
        eps, R = ref["eps"][live], ref["R"][live]
        if greedy:
            want = np.where(b["mask"], x, -np.inf).argmax(axis=1)[live]  # (argmax: the lowest index of the maximum)
            assert np.array_equal(a, want), ("greedy", np.flatnonzero(a != want)[:8])
            top = np.where(b["mask"], x, -np.inf)[live]
            stats["ties"] += int(((top == top.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())  # rows whose maximum occurs twice
        else:
            u = np.array([uniform_of(policy_seed, int(b["base"]) + int(i), int(b["tstep"][i])) for i in live])
            lo, hi = ref["F_lo"][live, a] - u, u - ref["F_hi"][live, a]
            worst = np.maximum(lo, hi) / eps  # <= 1: inside the band
            stats["sample"] = max(stats["sample"], float(worst.max()))
            assert (worst <= 1.0).all(), ("u outside [F_lo - eps, F_hi + eps]", live[worst > 1.0][:8], worst.max())
            if raised is not None:
                assert np.array_equal(a, raised[s0:s0 + B][live]), "the action raised by 20 is the sampled one in every row"
        tol = eps * (1.0 + R)
        e_lp, e_en = np.abs(lp[live] - ref["logp"][live, a]) / tol, np.abs(en[live] - ref["entropy"][live]) / tol
        stats["logp"] = max(stats["logp"], float(e_lp.max())); stats["entropy"] = max(stats["entropy"], float(e_en.max()))
        stats["logp_abs"] = max(stats["logp_abs"], float(np.abs(lp[live] - ref["logp"][live, a]).max()))
        stats["entropy_abs"] = max(stats["entropy_abs"], float(np.abs(en[live] - ref["entropy"][live]).max()))
        assert (e_lp <= 1.0).all() and (e_en <= 1.0).all(), ("logp / entropy outside eps (1 + R)", e_lp.max(), e_en.max())
        single = live[b["mask"][live].sum(axis=1) == 1]
        stats["single"] += len(single)
        assert (lp[single] == 0.0).all() and (en[single] == 0.0).all(), "one valid action: logp 0.0 and entropy 0.0 exactly"
        assert np.array_equal(act[single], b["mask"][single].argmax(axis=1))


def new_stats():
    return dict(rows=0, idle=0, single=0, ties=0, sample=0.0, logp=0.0, entropy=0.0, logp_abs=0.0, entropy_abs=0.0)


def _rollout(eng, device, K, stats, rng):
    """K steps of sample_actions + step with the three logit sets in turn; every step also the greedy anchor and evaluate_actions of
    what the previous step saved (the engine has stepped on in between)"""
    env, saved = eng.env, None
    dev = torch.device(device)
    for k in range(K):
        blocks = eng.blocks()
        kind = ("normal", "zeros", "raised")[k % 3]
        x_np, raised = logit_set(kind, rng, blocks)
        x = torch.from_numpy(x_np).to(dev)
        # exact anchor: greedy on quantised logits (nothing is stepped)
        h_np, _ = logit_set("half", rng, blocks)
        ga, glp, gen = env.sample_actions(torch.from_numpy(h_np).to(dev), POLICY_SEED + k, greedy=True)
        check_outputs(blocks, h_np, POLICY_SEED + k, True, _np(ga), _np(glp), _np(gen), stats)
        # the three accepted shapes of the same logits
        shaped = x if k % 3 == 0 else (x.view(-1, 1) if k % 3 == 1 else (x.view(blocks[0]["B"], -1) if len(blocks) == 1 else x))
        act, lp, en = env.sample_actions(shaped, POLICY_SEED + k)
        check_outputs(blocks, x_np, POLICY_SEED + k, False, _np(act), _np(lp), _np(en), stats, raised if kind == "raised" else None)
        if saved is not None:
            check_evaluate(env, *saved)
        saved = (x, eng.mask_flat().clone(), act.clone(), lp.clone(), en.clone())
        env.step(act.clone())
    check_evaluate(env, *saved)


def check_evaluate(env, x, mask, act, lp, en):
    """evaluate_actions on the saved (logits, mask, actions) of a sample_actions call reproduces that call bit for bit; a slot that was
    idle (action -1) scores -inf"""
    elp, een = env.evaluate_actions(x, act, mask.view(torch.bool))
    drew = act >= 0
    assert torch.equal(elp[drew], lp[drew]) and torch.equal(een[drew], en[drew]), "evaluate_actions != the sample_actions call it re-scores"
    assert bool(torch.isneginf(elp[~drew]).all())
    empty = torch.tensor(np.concatenate([np.repeat(~m.any(axis=1), 1) for m in _split_rows(env, _np(mask))]))
    assert bool((een.cpu()[empty] == 0.0).all()), "an all-zero mask row has entropy 0"


def _split_rows(env, flat):
    members = list(env.classes) if hasattr(env, "classes") else [env]
    out, off = [], 0
    for c in members:
        out.append(flat[off:off + c.num_envs * c.A].reshape(c.num_envs, c.A).astype(bool)); off += c.num_envs * c.A
    return out


def _finish(eng, stats, what):
    print(what, {k: (round(v, 4) if isinstance(v, float) and v >= 1e-3 else v) for k, v in stats.items()})
    assert stats["rows"] > stats["idle"]
    env = eng.env
    flags = int((env.g if hasattr(env, "g") else env.t)["work_count"][1].item())
    assert flags == 0, f"device error flags {flags:#x}"
    env.close()
    return stats


def check_uniform(ge, device, lib, env_id, kw, B, K=K_STEPS, autoreset=True):
    env = ge.VectorGraphEnv(env_id, B, seed_stride=STRIDE, env_index_base=BASE, autoreset=autoreset, **_extra(device, lib), **kw)
    env.reset(seed=S0)
    eng, stats = Engine(env), new_stats()
    _rollout(eng, device, K, stats, np.random.default_rng(1234 + B))
    assert stats["ties"] > 0, "the greedy anchor met no tie"
    if env.A <= 5:  # (the case that is there for them: a handful of actions, most of them masked after a few steps)
        assert stats["single"] > 0, "the single-valid-action anchor met no such row"
    return _finish(eng, stats, (env_id, kw, B))


def check_ragged(ge, device, lib, env_id, sizes, prefetch, K=K_STEPS):
    env = ge.RaggedVectorEnv(env_id, sizes, seed_stride=STRIDE, env_index_base=BASE, prefetch=prefetch, **_extra(device, lib))
    env.reset(seed=S0)
    eng, stats = Engine(env), new_stats()
    assert eng.numel == env.mask_flat.numel()
    _rollout(eng, device, K, stats, np.random.default_rng(99))
    assert stats["ties"] > 0, "the greedy anchor met no tie"
    return _finish(eng, stats, (env_id, sizes, prefetch))


def check_frozen(ge, device, lib, env_id=_SP, kw=None, B=70):
    """autoreset off, until every slot is frozen and two steps beyond: a frozen slot returns -1, 0.0, 0.0 and none of its slabs change"""
    kw = kw or dict(n_nodes=10, n_edges=20)
    env = ge.VectorGraphEnv(env_id, B, seed_stride=STRIDE, env_index_base=BASE, autoreset=False, **_extra(device, lib), **kw)
    env.reset(seed=S0)
    eng, stats, rng = Engine(env), new_stats(), np.random.default_rng(5)
    rows = lambda: {k: dict.__getitem__(env.t, k).reshape(B, -1).clone() for k in fc._SLOT_ROWS if dict.__getitem__(env.t, k) is not None}
    beyond = k = 0
    while beyond < 2:
        assert k < 8 * kw["n_nodes"], "slots still running at the step cap"
        blocks = eng.blocks()
        frozen = torch.from_numpy((blocks[0]["status"] == 1) | (blocks[0]["status"] == 4))
        beyond += int(bool(frozen.all()))
        before = rows()
        x_np, _ = logit_set("normal", rng, blocks)
        act, lp, en = env.sample_actions(torch.from_numpy(x_np).to(torch.device(device)), POLICY_SEED + k)
        check_outputs(blocks, x_np, POLICY_SEED + k, False, _np(act), _np(lp), _np(en), stats)
        assert bool((act.cpu()[frozen] == -1).all()) and bool((lp.cpu()[frozen] == 0).all()) and bool((en.cpu()[frozen] == 0).all())
        env.step(act.clone())
        for key, v in rows().items():
            assert torch.equal(v.cpu()[frozen], before[key].cpu()[frozen]), (k, key)
        k += 1
    assert stats["idle"] >= 2 * B
    return _finish(eng, stats, ("frozen", env_id, kw))


def _slabs(env):
    if hasattr(env, "_quiesce"):
        env._quiesce()
    if hasattr(env, "classes"):
        out = [("g." + k, k, v) for k, v in env.g.items()]
        for ci, c in enumerate(env.classes):
            out += [(f"class{ci}.{k}", k, v) for k, v in dict.items(c.t)]
        return out
    return [(k, k, v) for k, v in dict.items(env.t)]


def check_step_policy_equals_sample_then_step(ge, device, lib, make, K=K_STEPS):
    """step_policy on one engine, sample_actions + step on its twin: every output and every live slab equal after each of the K steps"""
    a, b = make(), make()
    a.reset(seed=S0); b.reset(seed=S0)
    eng, rng = Engine(a), np.random.default_rng(7)
    moved = 0
    for k in range(K):
        x_np, _ = logit_set("normal", rng, eng.blocks())
        x = torch.from_numpy(x_np).to(torch.device(device))
        oa = a.step_policy(x, POLICY_SEED + k)
        act, lp, en = b.sample_actions(x, POLICY_SEED + k)
        ob = b.step(act.clone())
        ia, ib = oa[4], ob[4]
        assert torch.equal(ia["action"], act) and torch.equal(ia["logp"], lp) and torch.equal(ia["entropy"], en), k
        assert torch.equal(oa[1], ob[1]) and torch.equal(oa[2], ob[2]) and torch.equal(oa[3], ob[3]), k
        for key in ("solved", "solution_cost", "heuristic_solution", "invalid_action", "episode_length"):
            assert torch.equal(ia[key], ib[key]), (k, key)
        moved += int((act >= 0).sum())
        skip = set(fc._prefetch_skip()) if getattr(a, "spare", None) is not None else set()
        fc._same_slabs(_slabs(a), _slabs(b), skip, k)
    assert moved > 0
    a.close(); b.close()


def check_shards_equal_one_engine(one, parts, device):
    """`parts` (a MixedVectorEnv or ShardedVectorEnv of two engines over consecutive slices of `one`'s slots, env_index_base
    following) gives, on the same logits, bit for bit what `one` gives: actions, logp and entropy from sample_actions, from
    evaluate_actions on what that call saved, and from step_policy (every other step is taken through it)"""
    members = parts.members
    assert len(members) == 2 and sum(m.num_envs for m in members) == one.num_envs
    one.reset(seed=S0); parts.reset(seed=S0)
    rng = np.random.default_rng(3)
    cat = lambda vs: torch.cat(list(vs))
    for k in range(4):
        blocks = Engine(one).blocks()
        x_np, _ = logit_set("normal", rng, blocks)
        x = torch.from_numpy(x_np).to(torch.device(device)).view(one.num_envs, one.A)
        act, lp, en = one.sample_actions(x, POLICY_SEED + k)
        cuts = np.cumsum([0] + [m.num_envs for m in members])
        xs = [x[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        outs = parts.sample_actions(xs, POLICY_SEED + k)
        for j, name in enumerate(("actions", "logp", "entropy")):
            assert torch.equal(cat(o[j] for o in outs), (act, lp, en)[j]), (k, name)
        drew = act >= 0
        assert int(drew.sum()) > 0
        acts = [o[0].clone() for o in outs]
        ev = parts.evaluate_actions(xs, acts, [m.mask.clone() for m in members])
        assert torch.equal(cat(e[0] for e in ev)[drew], lp[drew]) and torch.equal(cat(e[1] for e in ev)[drew], en[drew]), k
        assert bool(torch.isneginf(cat(e[0] for e in ev)[~drew]).all())
        act, lp, en = act.clone(), lp.clone(), en.clone()
        want = one.step(act.clone())
        if k % 2 == 0:
            got = parts.step_policy(xs, POLICY_SEED + k)
            for name, v in (("action", act), ("logp", lp), ("entropy", en)):
                assert torch.equal(cat(i[name] for i in got[4]), v), (k, name)
        else:
            got = parts.step(acts)
        for j in (1, 2, 3):
            assert torch.equal(cat(got[j]), want[j]), (k, j)
    one.close(); parts.close()


def check_errors(ge, device, lib):
    env = ge.VectorGraphEnv(_SP, 6, n_nodes=10, n_edges=20, **_extra(device, lib))
    dev = torch.device(device)
    good = torch.zeros(6, 10, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="holds no episode yet"):  # the library's GE_E_STATE message
        env.sample_actions(good)
    env.reset(seed=1)
    with pytest.raises(ValueError, match="elements"):
        env.sample_actions(torch.zeros(6, 9, dtype=torch.float32, device=dev))
    with pytest.raises(TypeError, match="float32"):
        env.sample_actions(good.double())
    with pytest.raises(ValueError, match="is on"):
        env.sample_actions(torch.empty(6, 10, dtype=torch.float32, device="meta"))
    with pytest.raises(TypeError):
        env.evaluate_actions(good, torch.zeros(6, dtype=torch.int64, device=dev), torch.zeros(6, 10, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="elements"):
        env.evaluate_actions(good, torch.zeros(6, dtype=torch.int64, device=dev), torch.zeros(6, 9, dtype=torch.bool, device=dev))
    L = env._L
    assert L.ge_policy_sample(env._h, good.data_ptr(), 0, 0, None, None, None, env._stream()) == -1  # GE_E_BADARG: actions is required
    assert L.ge_policy_step(env._h, good.data_ptr(), 0, 0, None, None, None, env._stream()) == -1
    assert L.ge_policy_evaluate(env._h, good.data_ptr(), None, None, None, None, env._stream()) == -1
    # logp and entropy may be NULL
    act = torch.zeros(6, dtype=torch.int64, device=dev)
    assert L.ge_policy_sample(env._h, good.data_ptr(), 0, 0, act.data_ptr(), None, None, env._stream()) == 0
    env._quiesce()
    a2, _, _ = env.sample_actions(good)
    assert torch.equal(act, a2)
    # evaluate: a masked-out action, -1 and an action >= A give -inf; an all-zero row has entropy 0
    mask = env.mask.clone()
    mask[5] = False
    acts = a2.clone()
    acts[1], acts[2] = -1, 10
    acts[3] = int(torch.nonzero(~mask[3])[0]) if bool((~mask[3]).any()) else -1
    lp, en = env.evaluate_actions(good, acts, mask)
    assert bool(torch.isneginf(lp[[1, 2, 3, 5]]).all()) and float(en[5]) == 0.0
    assert bool(torch.isfinite(lp[[0, 4]]).all()) and bool((en[:5] >= 0).all())
    env.close()
