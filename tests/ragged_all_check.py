"""Shared body of the multi-class (ragged) engine tests for every env id: per-class kwargs, every slot replayed on the CPU oracle
through autoresets, and the equivalence of a ragged engine with one uniform engine per class."""
import numpy as np
import torch

def _kw(device, library):
    return dict(device=device, _library=library) if library is not None else dict(device=device)


def _entries(sizes):
    """(b, n, m, own kwargs) of every sizes entry"""
    return [(int(e[0]), int(e[1]), int(e[2]), dict(e[3]) if len(e) == 4 else {}) for e in sizes]


def make_ragged(ge, env_id, sizes, common, device, library=None, prefetch=0, **extra):
    return ge.RaggedVectorEnv(env_id, sizes, prefetch=prefetch, **_kw(device, library), **extra, **common)


def _slot_obs(env, c, i):
    """(x, edge_links, edge_attr) of local slot i of class c, from the shared slabs"""
    noff, eoff, slot, moff, b, n, E, A = env._offsets[c]
    lo = noff + i * n
    x = env.x[lo:lo + n].cpu().numpy()
    ea = env.edge_attr[eoff + i * E:eoff + (i + 1) * E].cpu().numpy()
    ei = env.edge_index[:, eoff + i * E:eoff + (i + 1) * E].cpu().numpy().T - lo
    return x, ei, ea


def check_ragged_all(ge, oracle, env_id, sizes, common, device="cpu", library=None, steps=20, prefetch=0, seed=11, policy_seed=5,
                     want_episodes=1):
    """every slot of a ragged engine replayed on the oracle through autoresets: observation (x, edge_index, edge_attr), mask bytes,
    the device policy's picks, reward, done, solution_cost, heuristic_solution and episode_length after every step; flat_obs() at
    the end"""
    env = make_ragged(ge, env_id, sizes, common, device, library, prefetch)
    B = env.num_envs
    assert [(b, n) for b, n, _ in env.sizes] == [(b, n) for b, n, _, _ in _entries(sizes)]
    env.reset(seed=seed)
    refs = []  # (oracle env, class, local slot, global slot)
    g = 0
    for c, ((b, n, m), own) in enumerate(zip(env.sizes, env.class_kwargs)):
        for i in range(b):
            r = oracle.OracleEnv(env_id, n_nodes=n, n_edges=m, **own)
            r.reset(seed=seed + g)
            refs.append(dict(r=r, c=c, i=i, g=g, t=0, ep=0, len=0))
            g += 1
    links = env.edge_links()

    def check_slot(p, what):
        r, c, i = p["r"], p["c"], p["i"]
        x, ei, ea = _slot_obs(env, c, i)
        assert np.array_equal(x, r.nodes()), what + " (x)"
        assert np.array_equal(ei, r.edge_links()), what + " (edge_index)"
        assert np.array_equal(links[c][i].cpu().numpy(), r.edge_links()), what + " (edge_links())"
        assert np.array_equal(ea, r.edges()), what + " (edge_attr)"
        assert np.array_equal(env.classes[c].mask[i].cpu().numpy(), r.mask()), what + " (mask)"

    for p in refs:
        check_slot(p, f"{env_id} slot {p['g']} after reset")
    episodes = 0
    for k in range(steps):
        acts = env.sample_random_actions(policy_seed=policy_seed).clone()
        obs, rew, term, trunc, info = env.step(acts)
        a, rw, tm = acts.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
        cost, heur, elen = info["solution_cost"].cpu().numpy(), info["heuristic_solution"].cpu().numpy(), info["episode_length"].cpu().numpy()
        flat = info["mask_flat"].cpu().numpy()
        links = env.edge_links()
        off = 0
        for p in refs:
            r, gs = p["r"], p["g"]
            want_a = oracle.policy_pick(r.mask(), policy_seed, gs, p["t"])
            assert int(a[gs]) == want_a, (env_id, gs, k, int(a[gs]), want_a)
            _, rr, dd, _, rinf = r.step(int(a[gs]))
            p["t"] += 1
            p["len"] += 1
            assert rr == rw[gs] and dd == bool(tm[gs]), (env_id, gs, k, rr, rw[gs], dd, tm[gs])
            if dd:
                assert float(cost[gs]) == rinf["solution_cost"], (env_id, gs, k, "solution_cost")
                assert float(heur[gs]) == rinf["heuristic_solution"], (env_id, gs, k, "heuristic_solution")
                assert int(elen[gs]) == p["len"], (env_id, gs, k, "episode_length")
                episodes += 1
                p["ep"] += 1
                p["len"] = 0
                r.reset(seed=(seed + gs + B * p["ep"]) % 2**32)
            check_slot(p, f"{env_id} slot {gs} step {k}")
            assert np.array_equal(flat[off:off + r.A].astype(bool), r.mask()), (env_id, gs, k, "mask_flat")
            off += r.A
    assert episodes >= want_episodes, (env_id, episodes)
    flats = env.flat_obs()
    for p in refs:
        assert np.array_equal(flats[p["c"]][p["i"]].cpu().numpy(), p["r"].obs()), (env_id, p["g"], "flat_obs")
    env.close()
    return episodes


def check_equals_uniform(ge, env_id, sizes, common, device="cpu", library=None, steps=20, prefetch=0, seed=7, policy_seed=3):
    """a ragged engine and, per class c, a uniform engine with env_index_base = start_c and seed_stride = B_total: bit-equal outputs
    after every step of the device policy"""
    env = make_ragged(ge, env_id, sizes, common, device, library, prefetch)
    B = env.num_envs
    unis, start = [], 0
    for (b, n, m), own in zip(env.sizes, env.class_kwargs):
        unis.append(ge.VectorGraphEnv(env_id, b, n, m, env_index_base=start, seed_stride=B, prefetch=prefetch, **_kw(device, library), **own))
        start += b
    env.reset(seed=seed)
    for u in unis:
        u.reset(seed=seed)

    def same(k):
        rl = env.edge_links()
        for c, (u, cls) in enumerate(zip(unis, env.classes)):
            lo, hi = env.slot_ptr[c], env.slot_ptr[c + 1]
            for key in ("x", "edge_attr", "mask", "mask_bits", "slot_rec", "heuristic", "node_bits"):
                assert torch.equal(cls.t[key].reshape(-1)[:u.t[key].numel()].cpu(), u.t[key].reshape(-1).cpu()), (env_id, c, k, key)
            assert torch.equal(rl[c].cpu(), u.edge_links().cpu()), (env_id, c, k, "edge_links")
            for key in ("reward", "terminated", "invalid", "solved", "final_cost", "final_heur", "final_len", "episode", "seed"):
                assert torch.equal(env.g[key][lo:hi].cpu(), u.t[key].cpu()), (env_id, c, k, key)

    same(-1)
    for k in range(steps):
        a = env.sample_random_actions(policy_seed=policy_seed).clone()
        au = [u.sample_random_actions(policy_seed=policy_seed).clone() for u in unis]
        assert torch.equal(a.cpu(), torch.cat([x.cpu() for x in au])), (env_id, k, "actions")
        env.step(a)
        for u, x in zip(unis, au):
            u.step(x)
        same(k)
    for c, (u, fl) in enumerate(zip(unis, env.flat_obs())):
        assert torch.equal(fl.cpu(), u.flat_obs().cpu()), (env_id, c, "flat_obs")
    terms = int(env.g["episode"].sum())
    env.close()
    for u in unis:
        u.close()
    return terms


def full_size_sizes(env_id, n_slots=16384, n_classes=64, lo=32, hi=256, seed=0):
    """a size curriculum: n_slots over n_classes distinct n in [lo, hi] (both ends included), m = 3 n; MST (SteinerTree with
    n_dests = n - 1) carries its per-class n_dests"""
    rng = np.random.default_rng(seed)
    ns = {lo, hi}
    while len(ns) < n_classes:
        ns.add(int(rng.integers(lo, hi + 1)))
    ns = sorted(ns)
    per = [n_slots // n_classes + (1 if c < n_slots % n_classes else 0) for c in range(n_classes)]
    return [(b, n, 3 * n) for b, n in zip(per, ns)]


def check_full_size(ge, oracle, env_id, sizes, common, device, sampled=16, steps=40, seed=11, policy_seed=5):
    """invariants over EVERY slot after every step (episode counters against the terminations seen, nobody frozen, mask bytes ==
    mask bits for a spread of classes) and `sampled` slots replayed on the oracle, policy draws and regenerated observations included"""
    env = make_ragged(ge, env_id, sizes, common, device, prefetch=None)
    B = env.num_envs
    starts = np.cumsum([0] + [b for b, _, _ in env.sizes])
    pick = np.random.default_rng(1)
    slots = sorted(set([0, B - 1] + pick.integers(0, B, sampled - 2).tolist()))
    plan = []
    for gs in slots:
        c = int(np.searchsorted(starts, gs, side="right") - 1)
        b, n, m = env.sizes[c]
        plan.append(dict(g=gs, c=c, i=gs - int(starts[c]), r=oracle.OracleEnv(env_id, n_nodes=n, n_edges=m, **env.class_kwargs[c]), t=0, ep=0, len=0))
    env.reset(seed=seed)

    def check_obs(p, what):
        x, ei, ea = _slot_obs(env, p["c"], p["i"])
        assert np.array_equal(x, p["r"].nodes()), what + " (x)"
        assert np.array_equal(ei, p["r"].edge_links()), what + " (edge_index)"
        assert np.array_equal(ea, p["r"].edges()), what + " (edge_attr)"
        assert np.array_equal(env.classes[p["c"]].mask[p["i"]].cpu().numpy(), p["r"].mask()), what + " (mask)"

    for p in plan:
        p["r"].reset(seed=seed + p["g"])
        check_obs(p, f"{env_id} slot {p['g']} after reset")
    seen = 0
    for k in range(steps):
        acts = env.sample_random_actions(policy_seed=policy_seed).clone()
        obs, rew, term, trunc, info = env.step(acts)
        seen += int(term.sum())
        packed = env.g["slot_rec"][:, 1]
        assert int(env.g["episode"].sum()) == seen, (env_id, k)       # same-step autoreset: one new episode per termination
        assert int(((packed >> 16) & 0xFF).max()) == 0, (env_id, k)    # nobody is frozen or pending
        for cls in env.classes[:: max(1, len(env.classes) // 16)]:
            bits = cls.t["mask_bits"]
            unpacked = ((bits.unsqueeze(-1) >> torch.arange(64, device=bits.device)) & 1).reshape(cls.num_envs, -1)[:, :cls.A].to(torch.uint8)
            assert torch.equal(unpacked, cls.t["mask"]), (env_id, cls.n, k)
        a, rw, tm = acts.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
        cost, heur, elen = info["solution_cost"].cpu().numpy(), info["heuristic_solution"].cpu().numpy(), info["episode_length"].cpu().numpy()
        for p in plan:
            gs, r = p["g"], p["r"]
            want_a = oracle.policy_pick(r.mask(), policy_seed, gs, p["t"])
            assert int(a[gs]) == want_a, (env_id, gs, k)
            _, rr, dd, _, rinf = r.step(int(a[gs]))
            p["t"] += 1
            p["len"] += 1
            assert rr == rw[gs] and dd == bool(tm[gs]), (env_id, gs, k)
            if dd:
                assert float(cost[gs]) == rinf["solution_cost"] and float(heur[gs]) == rinf["heuristic_solution"], (env_id, gs, k)
                assert int(elen[gs]) == p["len"], (env_id, gs, k)
                p["ep"] += 1
                p["len"] = 0
                r.reset(seed=(seed + gs + B * p["ep"]) % 2**32)
            check_obs(p, f"{env_id} slot {gs} step {k}")
    assert seen > 0, env_id
    env.close()
