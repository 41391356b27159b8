"""GPU (MI355X): engines that share the chip.  The kernels set their issue priority by role (ge_platform.h, GE_PRIO_*): the n <= 64
step kernel and the probe of the generic feature kernel's fallback launch outrank the graph kernel and the feature kernels, which both stay at the default level (only a
retrying wave of the graph kernel is one above it).  A priority only reorders issue
between the waves on a SIMD, so nothing an engine computes may depend on it, on what runs beside it, or on how a batch is split:

  * ShortestPath n = 64 m = 192 (the headline's geometry), B = 768, as three shards on three streams and as one engine, 40 steps of
    random_rollout(1): the shards against the CPU oracle slot by slot (tests/fused_check.py), and the per-slot slabs of the three
    shards against the one engine's after every step;
  * the same on a deep geometry whose slots overflow the n <= 64 feature fast path (more than GE_F64_LV = 12 BFS levels), so that the
    LIST launch of the generic feature kernel finds a non-empty list, drops its priority and works: the test asserts it happened;
  * a SteinerTree n = 70 m = 210 engine with episode prefetch (generic feature kernel in queue mode) beside a ShortestPath engine in
    one MixedVectorEnv: the SteinerTree engine against the oracle and an unfused twin, the ShortestPath engine against a twin that
    runs alone.

Seeds, stride and policy seed are fused_check's."""
import pytest
import torch

import fused_check as fc

pytestmark = pytest.mark.gpu

# per-slot slabs: B rows (or B n, B E rows) in slot order whatever the engine's share of the batch.  (edge_index holds global node
# ids in a [2, B E] layout, the queues, generator ring and work space are engine-wide: the oracle comparison covers what they feed.)
_PER_SLOT = fc._SLOT_ROWS + ("reward", "terminated", "solved", "invalid", "row_ptr", "colw", "scode", "adj_bits", "node_rec")


def _ge():
    import graphenvs_amd as ge
    return ge


class _Batch:
    """ShortestPath slots [0, B) as `shards` engines (1: a VectorGraphEnv, else a ShardedVectorEnv), driven by random_rollout(1) only;
    the interface fused_check._rollout asks of an engine"""

    def __init__(self, ge, device, lib, kw, B, shards):
        self.env = ge.make_vec("ShortestPath-v0", B, shards=shards, record_actions=True, obs_mode="flat", seed_stride=fc.STRIDE,
                               env_index_base=fc.BASE, autoreset=True, prefetch=0, **fc._extra(device, lib), **kw)
        self.members = list(getattr(self.env, "members", [self.env]))
        assert len(self.members) == shards and sum(m.num_envs for m in self.members) == B
        self.env.reset(seed=fc.S0)
        self.B, self.kw = B, kw
        self.AW = [(self.members[0].A + 63) // 64] * B
        self.listed = []  # length of the feature fast path's fallback list after every step, summed over the engines

    def oracle_kwargs(self):
        return [self.kw] * self.B

    def fused(self, ps):
        self.env.random_rollout(1, policy_seed=ps)
        self.listed.append(sum(int(m.t["work_count"][0]) for m in self.members))

    unfused = fused  # (as the twin of _rollout: the one engine runs the same fused launches)

    def _cat(self, key):
        return torch.cat([dict.__getitem__(m.t, key).reshape(m.num_envs, -1) for m in self.members])

    def out(self, key):
        return fc._np(torch.cat([m.t[key] for m in self.members]))

    def actions(self, scratch=False):
        return self.out("actions_out")

    def masks(self):
        fc._bits_match_bytes(self._cat("mask_bits"), self._cat("mask"), "mask_bits != mask bytes")
        return list(fc._np(self._cat("mask")).astype(bool))

    def obs(self):
        return [row for m in self.members for row in fc._np(m.flat_obs())]

    def slabs(self):
        for m in self.members:
            m._quiesce()
        return [(k, k, self._cat(k)) for k in _PER_SLOT if dict.__getitem__(self.members[0].t, k) is not None]

    def close(self):
        for m in self.members:
            m.check_device_errors()
        self.env.close()


def check_shards_vs_oracle_and_one_engine(ge, oracle, device, lib, kw, B=768, K=40, shards=3):
    many, one = _Batch(ge, device, lib, kw, B, shards), _Batch(ge, device, lib, kw, B, 1)
    st = fc._rollout(oracle, many, one, "ShortestPath-v0", K, True, 0, 77, 1)
    assert many.listed == one.listed, (many.listed, one.listed)  # the same slots overflow the fast path however the batch is split
    return dict(st, listed=many.listed)


def test_three_shards_match_the_oracle_and_one_engine_on_the_headline_geometry():
    import oracle
    st = check_shards_vs_oracle_and_one_engine(_ge(), oracle, "cuda", None, dict(n_nodes=64, n_edges=192))
    print(st)
    assert st["episodes"] >= 768  # every shard regenerates in (nearly) every step, beside the others' step and feature kernels


# ShortestPath n = 28, m = 32: five edges more than a tree, so a BFS often runs deeper than the 12 levels the fast path keeps.
# (At n = 64 the sparsest m the constructor admits gives a connected G(n, m) once in millions of draws: a rollout would not end.)
DEEP = dict(n_nodes=28, n_edges=32)


def test_three_shards_with_a_non_empty_fallback_list_match_the_oracle_and_one_engine():
    import oracle
    st = check_shards_vs_oracle_and_one_engine(_ge(), oracle, "cuda", None, DEEP)
    print(st)
    assert sum(1 for c in st["listed"] if c > 0) >= 10, st["listed"]  # the LIST launch had slots to work on, not once by luck


class _Beside(fc._Uniform):
    """a uniform engine whose fused step is launched by a MixedVectorEnv that also holds a ShortestPath engine; that neighbour is
    compared, after every step, with a twin of its own that runs alone"""

    def attach(self, ge, device, lib, near_B):
        self.near_B = near_B
        kw = dict(record_actions=True, seed_stride=fc.STRIDE, env_index_base=fc.BASE, prefetch=0, n_nodes=64, n_edges=192, **fc._extra(device, lib))
        self.near, self.alone = ge.VectorGraphEnv("ShortestPath-v0", near_B, **kw), ge.VectorGraphEnv("ShortestPath-v0", near_B, **kw)
        self.near.reset(seed=fc.S0); self.alone.reset(seed=fc.S0)
        self.mixed = ge.MixedVectorEnv([self.env, self.near])
        return self

    def fused(self, ps):
        self.mixed.random_rollout(1, policy_seed=ps)
        self.alone.random_rollout(1, policy_seed=ps)
        self.near._quiesce(); self.alone._quiesce()
        fc._same_slabs([(k, k, v) for k, v in dict.items(self.near.t)], [(k, k, v) for k, v in dict.items(self.alone.t)], (), "neighbour")

    def close(self):
        assert int(self.near.t["episode"].sum()) >= self.near_B
        self.near.check_device_errors(); self.alone.check_device_errors()
        self.env.check_device_errors()
        self.mixed.close(); self.alone.close()


def check_generic_engine_beside_a_path_engine(ge, oracle, device, lib, B=300, K=40, near_B=768):
    kw = dict(n_nodes=70, n_edges=210, n_dests=3)
    f = _Beside(ge, device, lib, "SteinerTree-v0", kw, B, True, 3).attach(ge, device, lib, near_B)
    u = fc._Uniform(ge, device, lib, "SteinerTree-v0", kw, B, True, 3)
    assert f.env.spare is not None and u.env.spare is not None
    return fc._rollout(oracle, f, u, "SteinerTree-v0", K, True, 3, 77, 1)


def test_steiner_engine_with_prefetch_beside_a_shortest_path_engine():
    import oracle
    print(check_generic_engine_beside_a_path_engine(_ge(), oracle, "cuda", None))
