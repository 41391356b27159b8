"""Shared body of the geometry-limit tests: where ge_get_layout stops admitting a graph (found by bisection, never assumed), that
ge_create / ge_create_ragged admit exactly what the layout query admits, and that the engine still equals the CPU oracle at the
largest admitted graph.  Runs on the CPU harness library (tests/emu) and on the device."""
import ctypes as C

import numpy as np
import torch

from graphenvs_amd import _lib
from graphenvs_amd.vector_env import make_config, normalize_kwargs

GE_E_BADARG, GE_E_UNSUPPORTED, GE_E_TOOBIG = -1, -2, -4  # include/graphenvs.h
N_LIMIT = 4095  # derive(): n_nodes must be in [3, 4095]

# one constructor per env id: the kwargs each needs, parenting 2 where the residual-graph walks then live in prune_scratch, n_dests
# small so that episodes of the edge-action envs stay short
ENV_KWARGS = {
    "ShortestPath-v0": dict(is_eval_env=True),
    "LongestPath-v0": dict(parenting=2),
    "SteinerTree-v0": dict(n_dests=4),
    "TSP-v0": dict(parenting=2),
    "DensestSubgraph-v0": dict(parenting=1),
    "MaxIndependentSet-v0": dict(),
    "MulticastRouting-v0": dict(n_dests=4),
    "DistributionCenter-v0": dict(target_count=6),  # (the default, n // 5 targets, makes episodes of hundreds of steps at 794 nodes)
    "PerishableProductDelivery-v0": dict(parenting=1),
}


def sparse_edges(lib, env_id, kw, n):
    """the fewest edges derive() does not refuse as too disconnected to sample (GE_E_UNSUPPORTED) at n nodes"""
    lo, hi = n - 2, 4 * n  # (lo: refused -- no connected graph, or hopeless; hi: sampled at once)
    assert layout_rc(lib, env_id, kw, n, hi)[0] != GE_E_UNSUPPORTED
    while hi - lo > 1:
        mid = (lo + hi) // 2
        rc = layout_rc(lib, env_id, kw, n, mid)[0]
        if rc == GE_E_UNSUPPORTED or (rc == GE_E_BADARG and mid < n):
            lo = mid
        else:
            hi = mid
    return hi


# density rules: n -> n_edges.  "dense": m = 3 n -- but 4 n for TSP, whose reset also rejects every graph with a node of degree 1
# (tsp.py:65-68): at m = 3 n and 800 nodes one graph in 2e5 passes, and derive() refuses m = 3 n as hopeless from 1 090 nodes on, so
# the refusals beyond the edge would not all be GE_E_TOOBIG.  "sparse": just above that refusal (layout / create checks only: a
# graph that sparse is connected once in 1e7 draws, a rollout on it would not end).  "complete": every edge.
def n_edges_of(lib, env_id, kw, density, n):
    if density == "dense":
        return 4 * n if env_id == "TSP-v0" else 3 * n
    if density == "complete":
        ng = n - 1 if env_id == "DensestSubgraph-v0" else n
        return ng * (ng - 1) // 2
    assert density == "sparse", density
    return sparse_edges(lib, env_id, kw, n)


def layout_rc(lib, env_id, kw, n, m, num_envs=2):
    """(return code, message) of ge_get_layout for the constructor call env_id(n_nodes=n, n_edges=m, **kw)"""
    cfg = make_config(env_id, num_envs, normalize_kwargs(env_id, n, m, **kw))
    lay = _lib.GeLayout()
    rc = lib.ge_get_layout(C.byref(cfg), C.byref(lay))
    return rc, (lib.ge_last_error() or b"").decode() if rc != 0 else ""


def find_n_max(lib, env_id, kw, density, lo=64):
    """the largest n the layout query admits, by bisection from an admitted lo to a refused hi"""
    rc = lambda n: layout_rc(lib, env_id, kw, n, n_edges_of(lib, env_id, kw, density, n))[0]
    assert rc(lo) == 0, (env_id, density, lo, rc(lo))
    hi = N_LIMIT
    assert rc(hi) == GE_E_TOOBIG, (env_id, density, rc(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rc(mid) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def check_monotone_edge(lib, env_id, kw, density, n_max, samples=24, seed=0):
    """every sampled n up to n_max is admitted, every sampled n beyond it is refused with GE_E_TOOBIG and a message; 4096 is a bad
    argument.  Sampled: both sides of the edge, every multiple of 64 (a node set gains a word there), and random sizes."""
    rng = np.random.default_rng(seed)
    lo = min(600, n_max)
    below = {lo, n_max, n_max - 1, n_max - 2} | {n for n in range(lo, n_max + 1) if n % 64 in (0, 1)}
    below |= set(int(v) for v in rng.integers(lo, n_max + 1, samples))
    above = {n_max + 1, n_max + 2, N_LIMIT} | {n for n in range(n_max + 1, N_LIMIT + 1) if n % 512 in (0, 1)}
    above |= set(int(v) for v in rng.integers(n_max + 1, N_LIMIT + 1, samples))
    for n in sorted(v for v in below if lo <= v <= n_max):
        rc, msg = layout_rc(lib, env_id, kw, n, n_edges_of(lib, env_id, kw, density, n))
        assert rc == 0, (env_id, density, n, rc, msg)
    for n in sorted(above):
        rc, msg = layout_rc(lib, env_id, kw, n, n_edges_of(lib, env_id, kw, density, n))
        assert rc == GE_E_TOOBIG and msg, (env_id, density, n, rc, msg)
    rc, msg = layout_rc(lib, env_id, kw, N_LIMIT + 1, n_edges_of(lib, env_id, kw, "dense", N_LIMIT + 1))
    assert rc == GE_E_BADARG and msg, (env_id, rc, msg)


def _extra(device, library):
    return dict(device=device, _library=library) if library is not None else dict(device=device)


SMALL = (2, 40, 160)  # the class of n <= 64 beside the wide one (m = 4 n: sampled at once by every env id)


def check_create_agrees(ge, lib, env_id, kw, density, n_max, device, library=None, below=(0, 1, 5)):
    """what the layout query admits is created, by ge_create (VectorGraphEnv) and by ge_create_ragged (a two-class RaggedVectorEnv
    with a class of 40 nodes beside it)"""
    for d in below:
        n = n_max - d
        m = n_edges_of(lib, env_id, kw, density, n)
        env = ge.VectorGraphEnv(env_id, 2, n, m, **_extra(device, library), **kw)
        env.close()
        for sizes in ([(1, n, m), SMALL], [SMALL, (1, n, m)]):
            env = ge.RaggedVectorEnv(env_id, sizes, prefetch=0, **_extra(device, library), **kw)
            env.close()


class _CountZeros:
    """counts the bytes torch.zeros hands out while it is active (every slab of the host is a torch.zeros)"""

    def __enter__(self):
        self.bytes, self._orig = 0, torch.zeros

        def zeros(*a, **k):
            t = self._orig(*a, **k)
            self.bytes += t.numel() * t.element_size()
            return t
        torch.zeros = zeros
        return self

    def __exit__(self, *exc):
        torch.zeros = self._orig


def check_refused_beyond(ge, lib, env_id, kw, density, n_max, device, library=None):
    """the first n beyond the edge: the host raises the engine's message before it allocates a slab"""
    import pytest
    n = n_max + 1
    m = n_edges_of(lib, env_id, kw, density, n)
    makers = [lambda: ge.VectorGraphEnv(env_id, 2, n, m, **_extra(device, library), **kw),
              lambda: ge.RaggedVectorEnv(env_id, [(1, n, m), SMALL], prefetch=0, **_extra(device, library), **kw),
              lambda: ge.RaggedVectorEnv(env_id, [SMALL, (1, n, m)], prefetch=0, **_extra(device, library), **kw)]
    if library is None:
        makers += [lambda: ge.make_vec(env_id, 2, n_nodes=n, n_edges=m, device=device, **kw),
                   lambda: ge.make(env_id, n_nodes=n, n_edges=m, device=device, **kw)]
    for k, make in enumerate(makers):
        with _CountZeros() as z:
            with pytest.raises(RuntimeError, match=r"code -4\): .*\S"):
                make()
        assert z.bytes == 0, (env_id, density, k, z.bytes)


def check_edge_rollout(ge, oracle, env_id, kw, n, m, device, library=None, B=2, K=10, want_episodes=0):
    """B slots of n nodes against the oracle with the device policy and same-step autoreset: the flat observation and the mask after
    the reset and after every step, reward, done, solved, solution_cost and heuristic_solution of every step"""
    stride, base, s0 = 7919, 11, 5
    env = ge.VectorGraphEnv(env_id, B, n, m, obs_mode="flat", seed_stride=stride, env_index_base=base, **_extra(device, library), **kw)
    if env_id in ("LongestPath-v0", "TSP-v0") and kw.get("parenting", 0) >= 2 and n > 512:
        assert env.t["prune_scratch"] is not None and env.t["prune_scratch"].numel() == B * 4 * env.W
    obs, info = env.reset(seed=s0)
    refs = [oracle.OracleEnv(env_id, n_nodes=n, n_edges=m, **kw) for _ in range(B)]
    seeds = [(s0 + base + i) % 2**32 for i in range(B)]
    want = np.stack([r.reset(seed=s)[0] for r, s in zip(refs, seeds)])
    assert np.array_equal(obs.cpu().numpy(), want), (env_id, n, "reset obs")
    assert np.array_equal(info["mask"].cpu().numpy(), np.stack([r.mask() for r in refs])), (env_id, n, "reset mask")
    tcount, episodes = [0] * B, 0
    for k in range(K):
        a = env.sample_random_actions(policy_seed=77).clone().cpu().numpy()
        assert a.tolist() == [oracle.policy_pick(r.mask(), 77, base + i, tcount[i]) for i, r in enumerate(refs)], (env_id, n, k)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a).to(env.device))
        rew, term = rew.cpu().numpy(), term.cpu().numpy()
        solved, fc, fh = info["solved"].cpu().numpy(), info["solution_cost"].cpu().numpy(), info["heuristic_solution"].cpu().numpy()
        assert not info["invalid_action"].any()
        for i, r in enumerate(refs):
            _, rr, dd, _, inf = r.step(int(a[i]))
            tcount[i] += 1
            assert rr == rew[i] and dd == bool(term[i]), (env_id, n, k, i, rr, rew[i])
            assert int(solved[i]) == (int(inf["solved"]) if "solved" in inf else -1), (env_id, n, k, i)
            if dd:
                assert fc[i] == inf["solution_cost"], (env_id, n, k, i)
                if not np.isnan(inf["heuristic_solution"]):
                    assert fh[i] == inf["heuristic_solution"], (env_id, n, k, i)
                episodes += 1
                seeds[i] = (seeds[i] + stride) % 2**32
                r.reset(seed=seeds[i])
        assert np.array_equal(info["mask"].cpu().numpy(), np.stack([r.mask() for r in refs])), (env_id, n, k)
        assert np.array_equal(obs.cpu().numpy(), np.stack([r.obs() for r in refs])), (env_id, n, k)
    assert episodes >= want_episodes, (env_id, n, episodes)
    env.check_device_errors()
    env.close()
    return episodes
