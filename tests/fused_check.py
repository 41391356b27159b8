"""Bodies shared by the GPU tests (tests/test_gpu_fused_rollout.py) and the CPU harness (tests/test_emu_kernels.py): the fused
policy+step kernels that ge_random_rollout launches -- ge_k_step<ENV, true, ..>, ge_k_step_edge<ENV, true, ..> (the quad sampler),
ge_k_step_path64<true, ..> -- against the CPU oracle slot by slot, and against an unfused twin engine slab by slab.

The engine under test is driven ONLY by random_rollout(1, policy_seed); the action every slot must have drawn is
oracle.policy_pick(oracle mask, policy_seed, global slot, executed transitions) and is read back from ge_buffers.actions_out."""
import numpy as np
import pytest
import torch

STRIDE, BASE, S0 = 7919, 11, 2**32 - 40  # seeds wrap around 2^32 inside the batch

# (env id, kwargs, B, K, autoreset, prefetch, episodes required) -- the smallest shapes that take every branch of the pieces the step
# kernels share (ge_policy_draw / ge_policy_idle, ge_bits8_to_bytes, ge_mask_slab_tail, ge_end_transition), run by the CPU harness and
# by the GPU test alike.  B = 6: one partial workgroup, fewer slots than threads.  n = 10: mask rows of single bytes; n = 16: of whole
# 8-byte groups.  Autoreset off runs until every slot has finished, K caps it.
_SP, _MIS, _ST = "ShortestPath-v0", "MaxIndependentSet-v0", "SteinerTree-v0"
_MIS10, _ST10 = dict(n_nodes=10, n_edges=20), dict(n_nodes=10, n_edges=20, n_dests=3, is_eval_env=True)
SMALL_CASES = [
    pytest.param(_SP, dict(n_nodes=10, n_edges=20, is_eval_env=True), 6, 40, True, 0, 6, id="small-path64-n10"),
    pytest.param(_SP, dict(n_nodes=16, n_edges=32, is_eval_env=True), 6, 40, True, 2, 6, id="small-path64-n16-spares"),
    pytest.param(_SP, dict(n_nodes=16, n_edges=32), 6, 40, "next_step", 0, 6, id="small-path64-n16-next-step"),
    pytest.param(_MIS, _MIS10, 6, 40, True, 0, 6, id="small-mis-n10"),
    pytest.param(_MIS, _MIS10, 6, 40, True, 3, 6, id="small-mis-n10-spares"),
    pytest.param(_MIS, dict(_MIS10, n_nodes=16, n_edges=32), 6, 40, "next_step", 0, 6, id="small-mis-n16-next-step"),
    pytest.param(_MIS, dict(_MIS10, n_nodes=16, n_edges=32), 6, 40, "next_step", 3, 6, id="small-mis-n16-next-step-spares"),
    pytest.param(_MIS, _MIS10, 6, 40, False, 0, 6, id="small-mis-n10-autoreset-off"),
    pytest.param(_ST, _ST10, 6, 40, True, 0, 6, id="small-quad-n10"),
    pytest.param(_ST, _ST10, 6, 40, True, 3, 6, id="small-quad-n10-spares"),
    pytest.param(_ST, _ST10, 6, 40, "next_step", 3, 6, id="small-quad-n10-next-step-spares"),
    pytest.param(_ST, _ST10, 6, 40, False, 0, 6, id="small-quad-n10-autoreset-off"),
]

# slabs with one row (or n, or E rows) per slot that a frozen slot must leave untouched
_SLOT_ROWS = ("x", "edge_attr", "mask", "mask_bits", "slot_rec", "node_bits", "target_bits", "counters", "terminals", "episode", "seed",
              "heuristic", "final_cost", "final_heur", "final_len", "cover_bits", "aux_bits", "node_aux")


def _extra(device, lib):
    return dict(device=device, _library=lib) if lib is not None else dict(device=device)


def _prefetch_skip():
    from test_gpu_parity import _PREFETCH_SKIP  # what an engine with spares need not reproduce: generator ring, queues, work space
    return _PREFETCH_SKIP


def _np(v):
    return v.cpu().numpy()


def _bits_match_bytes(bits, mask, what):
    """mask_bits [b, AW] int64 unpacked == mask [b, A] bytes"""
    A = mask.shape[1]
    unpacked = np.unpackbits(_np(bits).view(np.uint8).reshape(mask.shape[0], -1), axis=1, bitorder="little")[:, :A]
    assert np.array_equal(unpacked, _np(mask)), what


def _same_slabs(f, u, skip, where):
    """every non-None slab of f (label, name, tensor) except actions_out and the names in `skip` equals u's"""
    count = {label: a for label, key, a in f if key == "work_count"}
    for (label, key, a), (_, _, b) in zip(f, u):
        if a is None or key == "actions_out" or key in skip:
            continue
        if key == "work_list":  # filled through an atomic counter, workgroup after workgroup in whatever order they run: the same SET of slots
            k = int(count[label.replace("work_list", "work_count")][0])
            a, b = torch.sort(a[:k]).values, torch.sort(b[:k]).values
        assert torch.equal(a, b), (where, label)


class _Uniform:
    """one VectorGraphEnv, fused (random_rollout) or unfused (sample + step)"""

    def __init__(self, ge, device, lib, env_id, kw, B, autoreset, prefetch):
        self.env = ge.VectorGraphEnv(env_id, B, record_actions=True, obs_mode="flat", seed_stride=STRIDE, env_index_base=BASE,
                                     autoreset=autoreset, prefetch=prefetch, **_extra(device, lib), **kw)
        self.env.reset(seed=S0)
        self.B = B
        self.AW = [(self.env.A + 63) // 64] * B
        self.kw = kw

    def oracle_kwargs(self):
        return [self.kw] * self.B

    def fused(self, ps):
        self.env.random_rollout(1, policy_seed=ps)

    def unfused(self, ps):
        self.env.step(self.env.sample_random_actions(policy_seed=ps).clone())

    def out(self, key):
        return _np(self.env.t[key])

    def actions(self, scratch=False):
        return _np(self.env._actions_scratch if scratch else self.env.t["actions_out"])

    def masks(self):
        _bits_match_bytes(self.env.t["mask_bits"], self.env.t["mask"], "mask_bits != mask bytes")
        return list(_np(self.env.t["mask"]).astype(bool))

    def obs(self):
        return list(_np(self.env.flat_obs()))

    def slabs(self):
        self.env._quiesce()
        return [(k, k, v) for k, v in dict.items(self.env.t)]

    def slot_rows(self):
        return {k: dict.__getitem__(self.env.t, k).reshape(self.B, -1).clone() for k in _SLOT_ROWS if dict.__getitem__(self.env.t, k) is not None}

    def close(self):
        self.env.check_device_errors()
        self.env.close()


class _Ragged:
    """one RaggedVectorEnv (multi-class engine)"""

    def __init__(self, ge, device, lib, env_id, sizes, common, prefetch):
        self.env = ge.RaggedVectorEnv(env_id, sizes, record_actions=True, seed_stride=STRIDE, env_index_base=BASE, prefetch=prefetch,
                                      **_extra(device, lib), **common)
        self.env.reset(seed=S0)
        self.B = self.env.num_envs
        self.AW = [(c.A + 63) // 64 for c in self.env.classes for _ in range(c.num_envs)]

    def oracle_kwargs(self):
        return [dict(ckw, n_nodes=n, n_edges=m) for (b, n, m), ckw in zip(self.env.sizes, self.env.class_kwargs) for _ in range(b)]

    def fused(self, ps):
        self.env.random_rollout(1, policy_seed=ps)

    def unfused(self, ps):
        self.env.step(self.env.sample_random_actions(policy_seed=ps).clone())

    def out(self, key):
        return _np(self.env.g[key])

    def actions(self, scratch=False):
        return _np(self.env.g["actions_out"])

    def masks(self):
        rows = []
        for c in self.env.classes:
            _bits_match_bytes(c.t["mask_bits"], c.t["mask"], ("mask_bits != mask bytes", c.n))
            rows += list(_np(c.t["mask"]).astype(bool))
        return rows

    def obs(self):
        return [row for fl in self.env.flat_obs() for row in _np(fl)]

    def slabs(self):
        if self.env.device.type == "cuda":
            torch.cuda.synchronize(self.env.device)
        out = [("g." + k, k, v) for k, v in self.env.g.items()]
        for ci, c in enumerate(self.env.classes):
            out += [(f"class{ci}.{k}", k, v) for k, v in dict.items(c.t)]
        return out

    def close(self):
        flags = int(self.env.g["work_count"][1].item())
        assert flags == 0, f"device error flags {flags:#x}"
        self.env.close()


def _rollout(oracle, f, u, env_id, K, mode, prefetch, policy_seed, min_episodes, scratch_actions=False):
    """f: the engine driven by the fused rollout, u: its unfused twin; mode: True (same-step autoreset), "next_step" or False"""
    B = f.B
    refs = [oracle.OracleEnv(env_id, **kw) for kw in f.oracle_kwargs()]
    seeds = [(S0 + BASE + i) % 2**32 for i in range(B)]
    for r, s in zip(refs, seeds):
        r.reset(seed=s)
    for i, (got, r) in enumerate(zip(f.obs(), refs)):
        assert np.array_equal(got, r.obs()), ("reset obs", i)
    skip = set(_prefetch_skip()) if prefetch else set()
    tcount, pending, frozen = [0] * B, [False] * B, [False] * B
    words = [np.zeros(aw, dtype=np.int64) for aw in f.AW]
    episodes = minus_ones = 0
    k = beyond = 0
    while True:
        if mode is False:
            if all(frozen):
                beyond += 1
            if beyond > 2:
                break
            assert k < K, "slots still running at the step cap"
        elif k == K:
            break
        # ---- what every slot must draw in this step
        want = []
        for i, r in enumerate(refs):
            if pending[i]:  # next-step autoreset: regenerated at the start of this step; an action is still drawn, from the new mask
                seeds[i] = (seeds[i] + STRIDE) % 2**32
                r.reset(seed=seeds[i])
            want.append(-1 if frozen[i] else oracle.policy_pick(r.mask(), policy_seed, BASE + i, tcount[i]))
        was_frozen = [i for i in range(B) if frozen[i]]
        before = f.slot_rows() if was_frozen else None
        f.fused(policy_seed)
        u.unfused(policy_seed)
        got = f.actions(scratch_actions)
        assert got.tolist() == want, (k, [(i, int(g), w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])
        rew, term, solved, fc, fh = f.out("reward"), f.out("terminated"), f.out("solved"), f.out("final_cost"), f.out("final_heur")
        for i, r in enumerate(refs):
            a = want[i]
            if a >= 0:
                words[i][a >> 6] += 1
            if frozen[i] or pending[i] or a < 0:  # frozen, regenerated in this step (action ignored), or an empty mask: nothing moves
                assert rew[i] == 0 and not term[i], (k, i)
                minus_ones += int(frozen[i])
                pending[i] = False
                continue
            _, rr, dd, _, inf = r.step(a)
            tcount[i] += 1
            assert rr == rew[i], (k, i, rr, rew[i])
            assert dd == bool(term[i]), (k, i)
            assert int(solved[i]) == (int(inf["solved"]) if "solved" in inf else -1), (k, i)
            if dd:
                assert fc[i] == inf["solution_cost"], (k, i)
                if not np.isnan(inf["heuristic_solution"]):
                    assert fh[i] == inf["heuristic_solution"], (k, i)
                episodes += 1
                if mode is True:
                    seeds[i] = (seeds[i] + STRIDE) % 2**32
                    r.reset(seed=seeds[i])
                elif mode == "next_step":
                    pending[i] = True
                else:
                    frozen[i] = True
        if before is not None:  # none of a frozen slot's slabs change
            idx = torch.tensor(was_frozen, dtype=torch.int64)
            for key, rows in f.slot_rows().items():
                assert torch.equal(rows.cpu()[idx], before[key].cpu()[idx]), (k, key)
        for i, (m, r) in enumerate(zip(f.masks(), refs)):
            assert np.array_equal(m, r.mask()), (k, i)
        k += 1
        if k % 10 == 0 or (mode is not False and k == K):
            for i, (o, r) in enumerate(zip(f.obs(), refs)):
                assert np.array_equal(o, r.obs()), (k, i)
        # ---- the unfused twin holds the same slabs (what the oracle does not see: slot_rec, counters, node_bits, queues, dirty words)
        _same_slabs(f.slabs(), u.slabs(), skip, k)
    for i, (o, r) in enumerate(zip(f.obs(), refs)):
        assert np.array_equal(o, r.obs()), ("end", i)
    # ---- the case was not vacuous
    assert episodes >= min_episodes, episodes
    hit = np.zeros(max(f.AW), dtype=np.int64)
    for aw in sorted(set(f.AW)):  # every word of the mask row of every geometry was drawn from
        tot = sum(w for w, a in zip(words, f.AW) if a == aw)
        assert (tot > 0).all(), ("mask words never drawn", aw, tot.tolist())
        hit[:aw] += tot
    if mode is False:
        assert minus_ones > 0 and all(frozen)
    f.close(); u.close()
    return dict(episodes=episodes, steps=k, word_draws=hit.tolist(), minus_ones=minus_ones)


def check_fused_vs_oracle(ge, oracle, device, lib, env_id, kw, B, K, autoreset=True, prefetch=0, policy_seed=77, min_episodes=1,
                          scratch_actions=False):
    """A uniform engine with record_actions=True driven only by random_rollout(1, policy_seed), B slots, K steps
    (autoreset=False: until every slot has finished and two steps beyond; K caps it): recorded action, reward, terminated, solved,
    final cost / baseline, mask bytes and bits of every slot after every step, the flat observation every 10th step and at the end,
    all equal to the oracle's; every non-None slab equal to an unfused twin's after every step.
    scratch_actions: the env has no fused kernel (DistributionCenter, n <= 64): the picks are read from the actions scratch."""
    mode = "next_step" if autoreset == "next_step" else bool(autoreset)
    f = _Uniform(ge, device, lib, env_id, kw, B, autoreset, prefetch)
    u = _Uniform(ge, device, lib, env_id, kw, B, autoreset, prefetch)
    assert (f.env.spare is not None) == bool(prefetch and mode is not False)
    return _rollout(oracle, f, u, env_id, K, mode, prefetch, policy_seed, min_episodes, scratch_actions)


def check_fused_ragged_vs_oracle(ge, oracle, device, lib, env_id, sizes, common, K, prefetch=0, policy_seed=77, min_episodes=1):
    """the same for a multi-class engine (RaggedVectorEnv, same-step autoreset): slots of several geometries in one workgroup"""
    f = _Ragged(ge, device, lib, env_id, sizes, common, prefetch)
    u = _Ragged(ge, device, lib, env_id, sizes, common, prefetch)
    assert (f.env.spare is not None) == bool(prefetch)
    return _rollout(oracle, f, u, env_id, K, True, prefetch, policy_seed, min_episodes)


def check_timed_rollout_equals_random_rollout(ge, device, lib, env_id, kw, B=300, K=20, policy_seed=77):
    """ge_timed_rollout (what bench.py reads its kernel split from) leaves the slabs ge_random_rollout leaves"""
    a = ge.VectorGraphEnv(env_id, B, seed_stride=STRIDE, env_index_base=BASE, **_extra(device, lib), **kw)
    b = ge.VectorGraphEnv(env_id, B, seed_stride=STRIDE, env_index_base=BASE, **_extra(device, lib), **kw)
    a.reset(seed=S0); b.reset(seed=S0)
    ms = a.timed_rollout(K, policy_seed)
    b.random_rollout(K, policy_seed)
    a._quiesce(); b._quiesce()
    assert set(ms) == {"step_ms", "reset_ms", "policy_ms"}
    skip = set(_prefetch_skip()) if a.spare is not None else set()
    _same_slabs([(k, k, v) for k, v in dict.items(a.t)], [(k, k, v) for k, v in dict.items(b.t)], skip, "timed")
    assert int(a.t["episode"].sum()) > 0 and int(a.t["tstep"].sum()) > 0
    a.check_device_errors(); b.check_device_errors()
    a.close(); b.close()


def check_sharded_timed_rollout_equals_random_rollout(ge, device="cuda"):
    """ShardedVectorEnv.timed_rollout -- shard 0 timed, the other shards rolling out beside it between one fork and one join -- leaves
    what random_rollout leaves.  Ten slots of ten nodes: the smallest batch that still gives three uneven shards (4 / 3 / 3) and
    several finished episodes in 25 steps."""
    make = lambda: ge.make_vec("ShortestPath-v0", 10, shards=3, prefetch=0, n_nodes=10, n_edges=20, device=device)
    many, twin = make(), make()
    assert many.shards == twin.shards == len(many.members)  # (the stream probe may grant fewer than three)
    many.reset(seed=7); twin.reset(seed=7)
    ms = many.timed_rollout(25, 5)
    twin.random_rollout(25, 5)
    for m in many.members + twin.members:
        m._quiesce()
    assert set(ms) == {"step_ms", "reset_ms", "policy_ms"}
    for key in ("episode", "tstep", "seed", "reward", "terminated", "cost", "solved"):
        assert torch.equal(many.gather(key), twin.gather(key)), key
    for key in ("x", "mask"):
        assert torch.equal(torch.cat([m.t[key] for m in many.members]), torch.cat([m.t[key] for m in twin.members])), key
    assert int(many.gather("episode").sum()) > 0  # autoreset really ran
    many.check_device_errors(); twin.check_device_errors()
    many.close(); twin.close()
