"""Ragged and mixed batches (BASELINE config 5): env instances of different (n_nodes, n_edges) -- and different env ids --
stepped together.  Every reference env instance has a fixed geometry (constructor kwargs), so a ragged batch is a list of size
classes.  ``RaggedVectorEnv`` is ONE multi-class engine per env id (``ge_create_ragged``): every kernel launch covers all classes
(a workgroup looks up the class of its slot), the classes share one set of PyG slabs (x, edge_index, edge_attr: variable-size CSR
packing, node ids offset per class through ``ge_config.node_id_base`` / ``edge_row_stride``), and the per-slot outputs are single
tensors over all slots.  Env ids side by side are a ``MixedVectorEnv`` (graphenvs_amd.mixed): one launch sequence per env id
(SURVEY 8d)."""
import ctypes as C

import torch

from . import _lib
from .mixed import MixedVectorEnv  # noqa: F401  (its earlier home)
from .vector_env import (PER_SLOT, EngineHandle, GraphBatch, VectorGraphEnv, engine_library, make_config, normalize_kwargs, slot_seeds,
                         spare_queues)

# per-slot arrays kept engine-wide (class c owns rows [start_c, start_c + B_c)): the ones every engine has in the same shape
_GLOBAL = PER_SLOT

# constructor kwargs a size class may set for itself (the per-instance scalars: ge_config.n_dests / max_distance / n_choices); every
# other kwarg is the same for all classes (ge_create_ragged refuses classes that differ in weighted, parenting, spatial or is_eval_env)
CLASS_KWARGS = ("n_dests", "n_products", "max_distance", "target_count", "n_choices")


class RaggedVectorEnv(EngineHandle):
    """One env id, several size classes: ``sizes = [(num_envs, n_nodes, n_edges), ...]``; an entry may carry a fourth element, a
    dict of the class's own values of ``CLASS_KWARGS`` (e.g. MST: ``("SteinerTree-v0", [(b, n, m, dict(n_dests=n - 1)), ...])``).
    ``n_edges = -1`` takes the reference's default where it has one.  Slots are numbered class after class; slot g runs seed
    (seed + g) like a uniform engine.  ``classes[c]`` are views of class c (``.mask`` [B_c, A_c] -- A_c = 2 m_c for the edge-action
    envs --, ``.t[...]``)."""

    def __init__(self, env_id, sizes, device="cuda", env_index_base=0, seed_stride=None, autoreset=True, _library=None, prefetch=None,
                 record_actions=False, **kwargs):
        self.env_id, self.device = env_id, torch.device(device)
        # every class normalised like a uniform engine (the reference's asserts and defaults), before any device allocation
        self.class_kwargs, self.sizes = [], []
        for entry in sizes:
            if len(entry) not in (3, 4):
                raise TypeError(f"a sizes entry is (num_envs, n_nodes, n_edges[, kwargs]), got {entry!r}")
            own = dict(entry[3]) if len(entry) == 4 else {}
            bad = sorted(k for k in own if k not in CLASS_KWARGS)
            if bad:
                raise TypeError(f"{env_id}: per-class kwargs {bad} are not allowed (only {', '.join(CLASS_KWARGS)} may differ between classes)")
            b, n = int(entry[0]), int(entry[1])
            ckw = dict(kwargs, **own)
            m = normalize_kwargs(env_id, n, int(entry[2]), **ckw)["n_edges"]
            self.class_kwargs.append(ckw)
            self.sizes.append((b, n, m))
        self.num_envs = B = sum(b for b, _, _ in self.sizes)
        stride = int(seed_stride) if seed_stride is not None else B
        self.seed_stride, self.env_index_base = stride, int(env_index_base)
        extra = dict(device=device, _library=_library) if _library is not None else dict(device=device)
        # every class must be one the engine admits before anything is allocated
        self._L = engine_library(self.device, _library)
        lays = [_lib.GeLayout() for _ in self.sizes]
        for (b, n, m), ckw, lay in zip(self.sizes, self.class_kwargs, lays):
            cfg = make_config(env_id, b, normalize_kwargs(env_id, n, m, **ckw))
            _lib.check(self._L, self._L.ge_get_layout(C.byref(cfg), C.byref(lay)), "ge_get_layout")
        F, Fe, edge_env = lays[0].F, lays[0].Fe, env_id in ("SteinerTree-v0", "MulticastRouting-v0")  # (an env id's feature widths: the same for every class)
        self.edge_env = edge_env
        dev = self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        Nn = sum(b * n for b, n, _ in self.sizes)
        Ne = sum(b * 2 * m for b, _, m in self.sizes)
        self.x, self.edge_index, self.edge_attr = z((Nn, F), torch.float32), z((2, Ne), torch.int64), z((Ne, Fe), torch.float32)
        A_of = lambda n, m: 2 * m if edge_env else n
        self.mask_flat = z((sum(b * A_of(n, m) for b, n, m in self.sizes),), torch.uint8)
        self.g = {k: z((B,) + shape, dt) for k, (shape, dt) in _GLOBAL.items()}
        self.g["reset_list"], self.g["reset_count"] = z((B,), torch.int32), z((_lib.queue_blocks(B),), torch.int32)
        self.g["work_list"], self.g["work_count"] = z((B,), torch.int32), z((4,), torch.int32)
        # where the fused policy+step launches record the actions they drew: one engine-wide array, which the engine takes from
        # class 0's ge_buffers (include/graphenvs.h, ge_create_ragged)
        self.g["actions_out"] = z((B,), torch.int64) if record_actions else None
        self.classes, self.slot_ptr, self._offsets = [], [0], []
        noff = eoff = slot = moff = 0
        ptr = [0]
        for (b, n, m), ckw in zip(self.sizes, self.class_kwargs):
            E, A = 2 * m, A_of(n, m)
            views = dict(x=self.x[noff:noff + b * n], edge_index=self.edge_index[0, eoff:], edge_attr=self.edge_attr[eoff:eoff + b * E],
                         mask=self.mask_flat[moff:moff + b * A].view(b, A))
            views.update({k: self.g[k][slot:slot + b] for k in _GLOBAL})
            views.update({k: self.g[k] for k in ("reset_list", "reset_count", "work_list", "work_count")})
            first = record_actions and slot == 0
            if first:
                views["actions_out"] = self.g["actions_out"]
            env = VectorGraphEnv(env_id, b, n, m, env_index_base=self.env_index_base + slot, seed_stride=stride, autoreset=autoreset,
                                 _views=views, node_id_base=noff, edge_row_stride=Ne, _defer_create=True, prefetch=0,
                                 record_actions=first, **extra, **ckw)
            self.classes.append(env)
            self._offsets.append((noff, eoff, slot, moff, b, n, E, A))
            ptr += [noff + (i + 1) * n for i in range(b)]
            noff += b * n; eoff += b * E; slot += b; moff += b * A
            self.slot_ptr.append(slot)
        nc = len(self.classes)
        # parenting >= 2 of LongestPath / TSP with a class above 512 nodes: the engine runs the residual-graph walks in memory for
        # every class, so every class gets a prune_scratch ([B_c, 4, W_c] words), also those a uniform engine would keep in registers
        if any(c.t["prune_scratch"] is not None for c in self.classes):
            for c in self.classes:
                if c.t["prune_scratch"] is None:
                    dict.__setitem__(c.t, "prune_scratch", z((c.num_envs * 4 * c.W,), torch.int64))
                    c.bufs = _lib.buffers(c.t)
        self._table = torch.zeros(int(self._L.ge_ragged_table_bytes(nc)), dtype=torch.uint8, device=dev)
        self._slot_class, self._class_start = z((B,), torch.int32), z((nc + 1,), torch.int32)
        cfgs = (_lib.GeConfig * nc)(*[c.cfg for c in self.classes])
        bufs = (_lib.GeBuffers * nc)(*[c.bufs for c in self.classes])
        h = C.c_void_p()
        _lib.check(self._L, self._L.ge_create_ragged(cfgs, bufs, nc, self._table.data_ptr(), self._slot_class.data_ptr(),
                                                     self._class_start.data_ptr(), C.byref(h)), "ge_create_ragged")
        self._h = h
        # episode prefetch (include/graphenvs.h, ge_attach_spares): a ragged batch is where it pays most -- every step a few slots of
        # many different sizes finish, and regenerated in place they cost the step the latency of the largest of them.  Refill every
        # 4 steps by default: on BASELINE config 5 (profiles/r03_c5_refill_period.txt) 0 / 2 / 4 / 6 / 8 / 16 / 32 steps give
        # 15.3 / 19.6 / 20.8 / 19.1 / 19.0 / 17.2 / 16.0 M env-steps/s -- the small classes' episodes last a handful of steps, and a
        # slot that finishes again before its image is refilled takes the in-place path
        self.prefetch = (4 if autoreset and _library is None else 0) if prefetch is None else int(prefetch)
        self.spare = None
        if self.prefetch and autoreset:
            self._attach_spares()
        self.ptr = torch.tensor(ptr, dtype=torch.int64, device=dev)
        self.batch = torch.repeat_interleave(torch.arange(B, device=dev), self.ptr[1:] - self.ptr[:-1])
        self._truncated = torch.zeros(B, dtype=torch.bool, device=dev)
        self._actions_scratch = z((B,), torch.int64)
        self._was_reset = False

    def _attach_spares(self):
        """a spare image of every class, packed like the live slabs (one x / edge_index / edge_attr / mask for all classes)"""
        shared = dict(x=torch.zeros_like(self.x), edge_index=torch.zeros_like(self.edge_index), edge_attr=torch.zeros_like(self.edge_attr),
                      mask=torch.zeros_like(self.mask_flat))
        shared.update({k: torch.zeros_like(self.g[k]) for k in _GLOBAL if k in _lib.IMAGE_FIELDS})
        sp = spare_queues(self.num_envs, self.device)
        images, recs = [], []
        for env, (noff, eoff, slot, moff, b, n, E, A) in zip(self.classes, self._offsets):
            views = dict(x=shared["x"][noff:noff + b * n], edge_index=shared["edge_index"][0, eoff:], edge_attr=shared["edge_attr"][eoff:eoff + b * E],
                         mask=shared["mask"][moff:moff + b * A].view(b, A))
            views.update({k: shared[k][slot:slot + b] for k in _GLOBAL if k in _lib.IMAGE_FIELDS})
            img = env._image_tensors(views)
            images.append(img)
            recs.append(_lib.spares(img, sp, self.prefetch))
        self._table_spare = torch.zeros_like(self._table)
        self.spare = dict(images=images, shared=shared, **sp)
        self._call("ge_attach_spares", (_lib.GeSpares * len(recs))(*recs), self._table_spare.data_ptr())

    def edge_links(self):
        """one [B_c, E_c, 2] tensor of local node ids per class (GraphInstance.edge_links of every slot of the class)"""
        out = []
        for noff, eoff, slot, moff, b, n, E, A in self._offsets:
            ei = self.edge_index[:, eoff:eoff + b * E].view(2, b, E)
            off = (torch.arange(b, device=self.device, dtype=torch.int64) * n + noff).view(1, -1, 1)
            out.append((ei - off).permute(1, 2, 0).contiguous())
        return out

    def graph(self):
        return GraphBatch(x=self.x, edge_index=self.edge_index, edge_attr=self.edge_attr, batch=self.batch, ptr=self.ptr,
                          num_graphs=self.num_envs)

    def _info(self, stepped):
        info = {"mask": [c.mask for c in self.classes],  # ragged: one [B_c, A_c] bool view per class
                "mask_flat": self.mask_flat.view(torch.bool)}
        if stepped:
            g = self.g
            info.update(solved=g["solved"], solution_cost=g["final_cost"], heuristic_solution=g["final_heur"],
                        invalid_action=g["invalid"].view(torch.bool), episode_length=g["final_len"])
        return info

    def reset(self, seed=0):
        self._seeds = slot_seeds(seed, self.num_envs, self.env_index_base, self.device)
        self._call("ge_reset", self._seeds.data_ptr(), self._stream())
        self._was_reset = True
        return self.graph(), self._info(False)

    def step(self, actions):
        actions = torch.as_tensor(actions).to(self.device, torch.int64).contiguous()
        assert actions.shape == (self.num_envs,) and self._was_reset
        self._act_keepalive = actions
        self._call("ge_step", actions.data_ptr(), self._stream())
        return self._after_step()

    def _policy_numel(self):
        return self.mask_flat.numel()  # the classes' [B_c, A_c] blocks one after the other: logits go in in this layout

    def _after_step(self, extra=None):
        g, info = self.g, self._info(True)
        if extra:
            info.update(extra)
        return self.graph(), g["reward"], g["terminated"].view(torch.bool), self._truncated, info

    def flat_obs(self):
        """utils.vectorize_graph of every slot, one [B_c, obs_len_c] tensor per class (views of one buffer)."""
        lens = [c.num_envs * c.obs_len for c in self.classes]
        flat = self._vectorized((sum(lens),))
        out, off = [], 0
        for c, ln in zip(self.classes, lens):
            out.append(flat[off:off + ln].view(c.num_envs, c.obs_len)); off += ln
        return out
