"""Batched graph environments on one MI355X: the host side of the C ABI.

Mirrors the reference's Gymnasium surface (graph_envs/__init__.py:9-56 and the six env classes):
same ids, same constructor kwargs/defaults/asserts, ``reset(seed=)`` / ``step(actions)`` /
``info['mask']``; the observation is the PyG-shaped view of utils.to_pyg_graph (utils.py:26-29)
kept resident in HBM.  All compute happens in the HIP kernels behind include/graphenvs.h; torch
is used for device memory and streams only.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

ENV_IDS = tuple(_lib.ENV_TYPES)

# constructor signatures of the reference
_DEFAULTS = {
    "ShortestPath-v0": dict(weighted=True, return_graph_obs=False, parenting=-1, structural_features=True, is_eval_env=False),
    "LongestPath-v0": dict(weighted=True, return_graph_obs=False, is_eval_env=False, parenting=-1),
    "SteinerTree-v0": dict(n_dests=3, weighted=True, parenting=-1, is_eval_env=False),
    "TSP-v0": dict(weighted=True, return_graph_obs=False, parenting=-1, spatial=False, is_eval_env=False),
    "DensestSubgraph-v0": dict(weighted=False, n_choices=-1, return_graph_obs=False, is_eval_env=False, parenting=-1),
    "MaxIndependentSet-v0": dict(weighted=True, return_graph_obs=False, is_eval_env=False),
    "MulticastRouting-v0": dict(n_dests=3, weighted=True, max_distance=-1, parenting=4, is_eval_env=False),
    "DistributionCenter-v0": dict(weighted=True, max_distance=1, target_count=-1, return_graph_obs=False, is_eval_env=False, parenting=2),
    "PerishableProductDelivery-v0": dict(n_products=3, delivery_time=-1, weighted=True, return_graph_obs=False, is_eval_env=False, parenting=-1),
}


def normalize_kwargs(env_id, n_nodes, n_edges=-1, **kwargs):
    """Apply the reference constructors' defaults and asserts (same messages)."""
    if env_id not in _DEFAULTS:
        raise KeyError(f"unknown env id {env_id!r}; hot-path ids are {ENV_IDS}")
    kw = dict(_DEFAULTS[env_id])
    for k, v in kwargs.items():
        if k not in kw:
            raise TypeError(f"{env_id}.__init__() got an unexpected keyword argument {k!r}")
        kw[k] = v
    if env_id == "ShortestPath-v0":
        assert kw["parenting"] == -1, "Parenting is not available for shortest path"  # shortest_path.py:26
    if env_id == "LongestPath-v0":
        assert kw["parenting"] in [0, 1, 2, 3]  # longest_path.py:29
    if env_id == "SteinerTree-v0":
        assert kw["parenting"] == -1, "Parenting not available for this environment"  # steiner_tree.py:29
    if env_id == "TSP-v0":
        assert kw["parenting"] in [1, 2], "Parenting must be either 1 or 2"  # tsp.py:25
        if kw["spatial"]:
            assert kw["weighted"] == True, "Spatial TSP must be weighted"  # noqa: E712  tsp.py:27
    if env_id == "DensestSubgraph-v0":
        assert kw["parenting"] in [0, 1], "Parenting must be 0 or 1"  # densest_subgraph.py:28
        assert kw["weighted"] == False, "Weighted graphs not supported for this env"  # noqa: E712
    if env_id == "DistributionCenter-v0":
        assert kw["parenting"] in [1, 2]  # distribution_center.py:32
        if kw["target_count"] == -1:
            kw["target_count"] = n_nodes // 5  # distribution_center.py:42-45
    if env_id == "MulticastRouting-v0" and kw["parenting"] not in [1, 2, 3, 4]:
        raise ValueError("Invalid parenting type")  # multicast_routing.py:34-35
    if env_id == "PerishableProductDelivery-v0":
        assert kw["parenting"] in [1], "Parenting must be 1!"  # perishable_product_delivery.py:30
        assert kw["n_products"] <= 5, "Max 5 products!"  # :35
        # with any other value the reference constructor leaves dt_mn / dt_mx unset and reset() raises AttributeError (:53,92)
        assert kw["delivery_time"] == -1, "delivery_time must be -1 (the reference only runs with its computed window)"
    if env_id in ("LongestPath-v0", "DensestSubgraph-v0", "MulticastRouting-v0", "PerishableProductDelivery-v0") and n_edges == -1:
        n_edges = int((n_nodes * (n_nodes - 1) // 2) * 0.30)  # longest_path.py:41-42, multicast_routing.py:53-54
    assert n_edges != -1, f"{env_id} needs n_edges"
    if env_id == "DensestSubgraph-v0" and kw["n_choices"] == -1:
        kw["n_choices"] = float(n_nodes // np.exp(1))  # densest_subgraph.py:38-39
    kw["n_nodes"], kw["n_edges"] = int(n_nodes), int(n_edges)
    if env_id == "PerishableProductDelivery-v0":  # perishable_product_delivery.py:53-61, in numpy as the reference computes it
        avg_dist = np.log(n_nodes) / np.log(2 * n_edges / n_nodes)
        if kw["weighted"]:
            avg_dist = avg_dist * (0.3 + 1.0) / 2.0
        kw["_dt_window"] = (float(avg_dist * 0.6), float(avg_dist * 1.4))
    return kw


def engine_library(device, _library=None):
    """the HIP library for a GPU device (no CPU path), or the handle a test passes in"""
    if _library is not None:
        return _library  # CPU sanitizer harness (tests/emu), host memory
    if torch.device(device).type != "cuda":
        raise RuntimeError("graphenvs_amd runs on a ROCm GPU only (device='cuda'); there is no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError("graphenvs_amd: no GPU visible to torch (torch.cuda.is_available() is False)")
    return _lib.load()


def make_config(env_id, num_envs, kw, autoreset_mode=1, env_index_base=0, seed_stride=None, node_id_base=0, edge_row_stride=0):
    """ge_config of include/graphenvs.h from normalize_kwargs() output: what ge_get_layout and ge_create are asked with"""
    return _lib.GeConfig(
        _lib.ENV_TYPES[env_id], int(num_envs), kw["n_nodes"], kw["n_edges"], int(bool(kw.get("weighted", False))),
        int(kw.get("parenting", -1)), int(kw.get("n_dests", kw.get("target_count", kw.get("n_products", 0)))), int(bool(kw.get("spatial", False))),
        int(bool(kw.get("is_eval_env", False))), int(autoreset_mode), float(kw.get("n_choices", -1)),
        int(env_index_base), int(seed_stride if seed_stride is not None else num_envs), int(node_id_base), int(edge_row_stride),
        float(kw["max_distance"]) if env_id == "DistributionCenter-v0" else 0.0, *kw.get("_dt_window", (0.0, 0.0)))


class GraphBatch(SimpleNamespace):
    """PyG ``Batch``-shaped view of the engine's observation slabs (x, edge_index, edge_attr, batch, ptr).
    Tensors alias engine memory and are valid until the next step()/reset(); ``to_pyg()`` upgrades to a
    real torch_geometric Batch when that package is installed."""

    def to_pyg(self):
        from torch_geometric.data import Batch, Data
        b = Batch(x=self.x, edge_index=self.edge_index, edge_attr=self.edge_attr, batch=self.batch, ptr=self.ptr)
        b._num_graphs = self.num_graphs
        return b

    def clone(self):
        return GraphBatch(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})


class _Space(SimpleNamespace):
    pass


def _gymnasium():
    """gymnasium when it is installed (it is not in the build image: everything gymnasium-specific is duck-typed otherwise)"""
    try:
        import gymnasium
        return gymnasium
    except ImportError:
        return None


_GYM = _gymnasium()
# gymnasium.vector.VectorEnv when importable, so that wrappers and trainers that check isinstance accept the engine
_VectorBase = _GYM.vector.VectorEnv if _GYM is not None and hasattr(_GYM, "vector") and hasattr(_GYM.vector, "VectorEnv") else object


class _Slabs(dict):
    """The engine's device slabs by name (what ge_buffers points at).  The scalar state of a slot is packed into
    ``slot_rec`` [B, 2] = {cost as float64 bits, head | status << 16 | aux << 24 | tstep << 32} (include/graphenvs.h
    GE_REC_*); ``t["cost"]`` / ``["head"]`` / ``["status"]`` / ``["tstep"]`` decode it on access (read-only views or copies,
    not slabs: they are not part of state_dict())."""
    DERIVED = ("cost", "head", "status", "tstep")

    def __missing__(self, key):
        rec = dict.__getitem__(self, "slot_rec")
        if key == "cost":
            return rec.view(torch.float64)[:, 0]
        packed = rec[:, 1]
        if key == "head":
            h = packed & 0xFFFF
            return torch.where(h == 0xFFFF, torch.full_like(h, -1), h).to(torch.int32)
        if key == "status":
            return ((packed >> 16) & 0xFF).to(torch.uint8)
        if key == "tstep":
            return (packed >> 32) & 0xFFFFFFFF
        raise KeyError(key)


# the per-slot arrays that are one row per slot whatever the env id and geometry: name -> (trailing shape, dtype).  A uniform engine
# allocates [B, ...] of each; a multi-class engine keeps ONE of each over all its slots and hands every class its rows.
PER_SLOT = dict(seed=((), torch.int32), episode=((), torch.int64), mt_state=((_lib.SEED_DEPTH, 2, 624), torch.int32),
                slot_rec=((2,), torch.int64), heuristic=((), torch.float64), reward=((), torch.float64),
                terminated=((), torch.uint8), invalid=((), torch.uint8), solved=((), torch.int8),
                final_cost=((), torch.float64), final_heur=((), torch.float64), final_len=((), torch.int32),
                counters=((2,), torch.int32))


def spare_queues(num_envs, device):
    """the five queues of the episode prefetch (ge_spares): a state byte and two slot lists per slot, a count per queue block"""
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)
    nb = _lib.queue_blocks(num_envs)
    return dict(state=z(num_envs, torch.uint8), swap_list=z(num_envs, torch.int32), swap_count=z(nb, torch.int32),
                refill_list=z(num_envs, torch.int32), refill_count=z(nb, torch.int32))


def slot_seeds(seed, num_envs, env_index_base, device):
    """the seeds ge_reset / ge_inject_state take, int32 [num_envs] on the device: an integer s gives slot i (global index g =
    env_index_base + i) the seed (s + g) mod 2^32; a sequence or tensor gives every slot its own"""
    if isinstance(seed, (int, np.integer)):
        s = (int(seed) + env_index_base + np.arange(num_envs, dtype=np.int64)) % (1 << 32)
    else:
        s = np.asarray(seed.cpu() if torch.is_tensor(seed) else seed, dtype=np.int64).reshape(num_envs)
        assert ((s >= 0) & (s < (1 << 32))).all(), "seeds must be in [0, 2**32) (np.random.seed requirement)"
    return torch.from_numpy(s.astype(np.uint32).view(np.int32)).to(device)


# GE_LOGITS_* of include/graphenvs.h: the storage types the policy head reads logits in (and writes their gradient in)
_LOGITS_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def policy_scale(temperature):
    """the float32 factor the engine multiplies every logit by: ``float(np.float32(1) / np.float32(temperature))``"""
    with np.errstate(all="ignore"):
        try:
            t = np.float32(temperature)
        except (TypeError, ValueError):
            raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}") from None
        if t.ndim != 0:
            raise ValueError(f"temperature must be one number, got {temperature!r}")
        scale = float(np.float32(1) / t)
    if not (np.isfinite(t) and t > 0 and np.isfinite(scale) and scale > 0):  # (a float32 1 / t that overflows or underflows is refused too)
        raise ValueError(f"temperature must be a finite number > 0 (and so must 1 / temperature in float32), got {temperature!r}")
    return scale


class _EvaluateActions(torch.autograd.Function):
    """evaluate_actions with a gradient for the logits: ge_policy_evaluate_as forward, ge_policy_backward_as backward (one launch
    each; the gradient has the logits' dtype).
    The outputs are fresh tensors -- a training step holds several evaluations alive; save_for_backward makes an in-place change of
    the logits, mask or actions before backward() torch's own error."""

    @staticmethod
    def forward(ctx, x, actions, mask, env, scale):
        logp, entropy = (torch.empty(env.num_envs, dtype=torch.float32, device=env.device) for _ in range(2))
        env._call("ge_policy_evaluate_as", x.data_ptr(), _LOGITS_DTYPES[x.dtype], scale, mask.data_ptr(), actions.data_ptr(), logp.data_ptr(),
                  entropy.data_ptr(), env._stream())
        ctx.env, ctx.scale = env, scale
        ctx.set_materialize_grads(False)  # (an output the loss does not use reaches backward as None, not as a tensor of zeros)
        ctx.save_for_backward(x, mask, actions)
        return logp, entropy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logp, grad_entropy):
        env = ctx.env
        if not env._h:
            raise RuntimeError("graphenvs_amd: backward through evaluate_actions() of a closed engine")
        x, mask, actions = ctx.saved_tensors
        # (an upstream gradient is often an expanded stride-0 view -- the one of a .mean() loss -- or absent: NULL stands for zeros)
        up = [None if g is None else g.to(device=env.device, dtype=torch.float32).contiguous() for g in (grad_logp, grad_entropy)]
        grad = torch.empty_like(x)  # (x is contiguous, the gradient has its dtype; the launch writes every element.  The locals outlive the enqueue below)
        env._call("ge_policy_backward_as", x.data_ptr(), _LOGITS_DTYPES[x.dtype], ctx.scale, mask.data_ptr(), actions.data_ptr(),
                  *(None if g is None else g.data_ptr() for g in up), grad.data_ptr(), env._stream())
        return grad, None, None, None, None


class EngineHandle:
    """What owns a ge_* handle: ``_L`` the library, ``_h`` the handle, ``device``, and the calls that are the same for a uniform
    and a multi-class engine.  A subclass sets those three, ``num_envs`` and ``_actions_scratch`` (int64, one entry per slot), and
    implements ``_policy_numel()`` and ``_after_step(extra)`` for the policy head."""
    _h = None
    _flat = None
    _policy = None

    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _call(self, name, *args):
        """ge_<name>(handle, *args), raising with the library's message unless it returns GE_OK"""
        _lib.check(self._L, getattr(self._L, name)(self._h, *args), name)

    def _quiesce(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def close(self):
        if self._h:
            self._quiesce()
            self._L.ge_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _vectorized(self, shape):
        """utils.vectorize_graph of every slot, back to back in one float32 buffer of `shape` (allocated at the first call)"""
        if self._flat is None:
            self._flat = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._call("ge_vectorize", self._flat.data_ptr(), self._stream())
        return self._flat

    def sample_random_actions(self, policy_seed=0, out=None):
        out = self._actions_scratch if out is None else out
        self._call("ge_sample_actions", int(policy_seed), out.data_ptr(), self._stream())
        return out

    # ------------------------------------------------------------------ masked categorical policy head (ge_policy_*)
    def _policy_input(self, v, what, dtypes):
        """`v` as a contiguous tensor of this engine's device with one element per (slot, action)"""
        if not torch.is_tensor(v):
            raise TypeError(f"{what} must be a torch tensor, got {type(v).__name__}")
        if v.dtype not in dtypes:
            raise TypeError(f"{what} must be {' or '.join(str(d) for d in dtypes)}, got {v.dtype}")
        if v.device.type != self.device.type or (self.device.index is not None and v.device.index != self.device.index):
            raise ValueError(f"{what} is on {v.device}, the engine on {self.device}")
        if v.numel() != self._policy_numel():
            raise ValueError(f"{what} has {v.numel()} elements, the engine's mask {self._policy_numel()} (one per slot and action)")
        return v.contiguous()

    def _policy_buffers(self):
        if self._policy is None:
            f = lambda dt: torch.empty(self.num_envs, dtype=dt, device=self.device)
            self._policy = dict(actions=f(torch.int64), logp=f(torch.float32), entropy=f(torch.float32),
                                eval_logp=f(torch.float32), eval_entropy=f(torch.float32))
        return self._policy

    def sample_actions(self, logits, policy_seed=0, greedy=False, temperature=1.0):
        """Masked categorical draw of every slot from the caller's logits, in one launch: ``(actions int64 [B], logp float32 [B],
        entropy float32 [B])`` -- what ``Categorical(logits=logits.masked_fill(~info['mask'], -inf))`` gives through sample(),
        log_prob() and entropy().  ``logits``: any float32 tensor on the engine's device with one element per (slot, action) in the
        layout of ``info['mask']`` (a multi-class engine: of ``mask_flat``): [B, A], [B * n] and [B * n, 1] are all accepted, a
        wrong element count, dtype or device raises.  The draw is a function of (policy_seed, global slot, the slot's transition
        count); ``greedy=True`` takes the valid action of largest logit.  A slot with no valid action and a frozen slot return
        -1, 0, 0.  The three tensors are allocated once per engine and overwritten by the next sample_actions() / step_policy():
        ``.clone()`` what a rollout buffer keeps, as with step().

        ``logits`` may also be bfloat16 or float16 (what a network under autocast emits): the kernel converts in registers, no
        ``.float()`` pass is needed.  ``temperature`` (a finite number > 0) divides the logits: the engine multiplies every element,
        as float32, by ``scale = float(np.float32(1) / np.float32(temperature))`` -- one float32 rounding -- and the result is
        bit for bit that of ``sample_actions(logits.float() * scale)``; 1.0 changes nothing."""
        x = self._policy_input(logits, "logits", tuple(_LOGITS_DTYPES))
        scale = policy_scale(temperature)
        o = self._policy_buffers()
        self._policy_keepalive = x
        self._call("ge_policy_sample_as", x.data_ptr(), _LOGITS_DTYPES[x.dtype], scale, int(policy_seed), int(bool(greedy)),
                   o["actions"].data_ptr(), o["logp"].data_ptr(), o["entropy"].data_ptr(), self._stream())
        return o["actions"], o["logp"], o["entropy"]

    def evaluate_actions(self, logits, actions, mask, temperature=1.0):
        """``(logp, entropy)`` of stored ``actions`` [B] under stored masks: the re-scoring of a PPO / A2C update.  ``mask``: bool or
        uint8, one element per logit -- what info['mask'] (``mask_flat``) held when the actions were drawn, cloned into the rollout
        buffer; the engine's live mask is not read.  On the logits, mask and actions of a sample_actions() call it returns that
        call's logp and entropy bit for bit.  An action of -1, out of range or masked out gives -inf.  The two tensors are
        allocated once per engine and overwritten by the next evaluate_actions().

        Differentiable in the logits: when ``logits.requires_grad`` and grad mode is on, the same values come back in fresh tensors
        with a ``grad_fn`` whose backward is one launch (ge_policy_backward, DESIGN.md 5: masked logits get a gradient of exactly
        0.0, a row whose action scored -inf drops its logp gradient, first order only).  sample_actions() and step_policy() carry no
        gradient: an on-policy update calls evaluate_actions() with the cloned mask and the drawn actions.

        ``logits`` float32, bfloat16 or float16 and ``temperature`` as in sample_actions().  The gradient has the logits' dtype and
        is taken with respect to the tensor passed in: with g the float32 gradient with respect to the scaled logit, an element is
        ``g * scale`` (one float32 multiply) rounded to the dtype to nearest even -- what autograd gives for
        ``evaluate_actions(logits.float() * scale, ...)``, bit for bit, without the cast and scale passes in either direction."""
        x = self._policy_input(logits, "logits", tuple(_LOGITS_DTYPES))
        scale = policy_scale(temperature)
        mk = self._policy_input(mask, "mask", (torch.bool, torch.uint8)).view(torch.uint8)
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions, dtype=np.int64))
        a = actions.to(device=self.device, dtype=torch.int64).contiguous()
        assert a.shape == (self.num_envs,)
        if x.requires_grad and torch.is_grad_enabled():
            return _EvaluateActions.apply(x, a, mk, self, scale)
        o = self._policy_buffers()
        self._evaluate_keepalive = (x, mk, a)
        self._call("ge_policy_evaluate_as", x.data_ptr(), _LOGITS_DTYPES[x.dtype], scale, mk.data_ptr(), a.data_ptr(), o["eval_logp"].data_ptr(),
                   o["eval_entropy"].data_ptr(), self._stream())
        return o["eval_logp"], o["eval_entropy"]

    def step_policy(self, logits, policy_seed=0, greedy=False, temperature=1.0):
        """sample_actions(logits, ...) and step() of the drawn actions in one call, nothing read back in between: returns what
        step() returns, with ``info['action']``, ``info['logp']`` and ``info['entropy']`` added (the tensors of sample_actions).
        ``logits`` float32, bfloat16 or float16 and ``temperature`` as in sample_actions()."""
        x = self._policy_input(logits, "logits", tuple(_LOGITS_DTYPES))
        scale = policy_scale(temperature)
        assert self._was_reset, "call reset() (or inject_state()) before step_policy()"
        o = self._policy_buffers()
        self._policy_keepalive = x
        self._call("ge_policy_step_as", x.data_ptr(), _LOGITS_DTYPES[x.dtype], scale, int(policy_seed), int(bool(greedy)),
                   o["actions"].data_ptr(), o["logp"].data_ptr(), o["entropy"].data_ptr(), self._stream())
        return self._after_step(dict(action=o["actions"], logp=o["logp"], entropy=o["entropy"]))

    def random_rollout(self, n_steps, policy_seed=0):
        self._call("ge_random_rollout", int(policy_seed), int(n_steps), self._actions_scratch.data_ptr(), self._stream())

    def timed_rollout(self, n_steps, policy_seed=0):
        """the rollout with a HIP-event pair around the policy, the step kernel and the autoreset launches of every step (profiling)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._call("ge_timed_rollout", int(policy_seed), int(n_steps), self._actions_scratch.data_ptr(), self._stream(),
                   C.byref(a), C.byref(b), C.byref(c))
        return dict(step_ms=a.value, reset_ms=b.value, policy_ms=c.value)


class VectorGraphEnv(EngineHandle, _VectorBase):
    """B independent envs of one id on one GPU.  One instance per process/GPU; no global state.  A subclass of
    gymnasium.vector.VectorEnv when gymnasium is installed (num_envs, single_*_space, *_space, metadata['autoreset_mode'])."""

    def __init__(self, env_id, num_envs, n_nodes, n_edges=-1, device="cuda", autoreset=True, obs_mode="pyg",
                 env_index_base=0, seed_stride=None, strict=False, _library=None, _views=None, node_id_base=0,
                 edge_row_stride=0, record_actions=False, copy_outputs=False, continue_streams=False, _defer_create=False, prefetch=None,
                 **kwargs):
        self.env_id = env_id
        self.kwargs = normalize_kwargs(env_id, n_nodes, n_edges, **kwargs)
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.obs_mode = obs_mode
        self.strict = strict
        self.copy_outputs = bool(copy_outputs)
        # reset(seed=None) like the reference (shortest_path.py:49-52): every slot draws its next graph from where its previous
        # reset left its `random` / `np.random` streams (5 KiB of saved generator state per slot, written by every reset).
        # Off: reset(seed=None) moves every slot to its next episode seed (seed + seed_stride), like an autoreset does.
        self.continue_streams = bool(continue_streams)
        # return_graph_obs (shortest_path.py:94-95 and siblings): info['graph_obs'] = per-slot (nodes, edges, edge_links) views
        self.return_graph_obs = bool(self.kwargs.get("return_graph_obs", False))
        # True / "same_step": a finished slot is regenerated inside the same step(); "next_step" (gymnasium's default mode): the
        # step that ends an episode returns its final observation and the NEXT step() regenerates the slot, ignoring its action;
        # False: finished slots freeze until reset()
        assert autoreset in (True, False, "same_step", "next_step"), autoreset
        self.autoreset_mode = 2 if autoreset == "next_step" else int(bool(autoreset))
        self.autoreset = bool(autoreset)
        self._L = engine_library(self.device, _library)
        kw = self.kwargs
        self.n, self.m = kw["n_nodes"], kw["n_edges"]
        self.seed_stride = int(seed_stride) if seed_stride is not None else self.num_envs
        self.env_index_base = int(env_index_base)
        self.cfg = make_config(env_id, self.num_envs, kw, self.autoreset_mode, self.env_index_base, self.seed_stride,
                               node_id_base, edge_row_stride)
        lay = _lib.GeLayout()
        _lib.check(self._L, self._L.ge_get_layout(C.byref(self.cfg), C.byref(lay)), "ge_get_layout")
        self.layout = lay
        self.F, self.Fe, self.A, self.W, self.E, self.obs_len = lay.F, lay.Fe, lay.A, lay.W, lay.E, int(lay.obs_len)
        B, n, E, W, A = self.num_envs, self.n, self.E, self.W, self.A
        AW = (A + 63) // 64
        edge_env = env_id in ("SteinerTree-v0", "MulticastRouting-v0")
        T = max(2, kw.get("n_dests", 0) + 1) if edge_env else max(2, kw.get("target_count", 0), 2 * kw.get("n_products", 0))
        self.T = T
        dev = self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        t = {k: z((B,) + shape, dt) for k, (shape, dt) in PER_SLOT.items()}
        t["x"] = z((B * n, self.F), torch.float32)
        t["edge_index"] = z((2, B * E), torch.int64)
        t["edge_attr"] = z((B * E, self.Fe), torch.float32)
        t["row_ptr"] = z((B, n + 1), torch.int32)
        t["colw"] = z((B * E,), torch.int16)
        t["scode"] = z((B * E,), torch.uint8)
        t["sw64"] = z((B * E,), torch.float64) if kw.get("spatial", False) else None
        t["adj_bits"] = z((B * n, W), torch.int64)
        t["node_rec"] = z((B * n, 2), torch.int64) if W == 1 else None
        t["rev_edge"] = z((B * E,), torch.int32) if edge_env else None
        t["terminals"] = z((B, T), torch.int32)
        t["node_bits"] = z((B, W), torch.int64)
        t["target_bits"] = z((B, W), torch.int64)
        t["aux_bits"] = z((B,), torch.int64) if (env_id == "DistributionCenter-v0" and W == 1) else None
        t["mask"] = z((B, A), torch.uint8)
        t["mask_bits"] = z((B, AW), torch.int64)
        t["reset_list"] = z((B,), torch.int32)
        t["reset_count"] = z((_lib.queue_blocks(B),), torch.int32)
        t["work_list"] = z((B,), torch.int32)
        t["work_count"] = z((4,), torch.int32)
        t["feat_scratch"] = z((B, lay.feat_parts, n), torch.float64) if lay.feat_parts > 1 else None
        t["node_aux"] = z((B, n), torch.int32) if env_id == "MulticastRouting-v0" and kw["parenting"] >= 3 else None
        dc = env_id == "DistributionCenter-v0"
        t["range_bits"] = z((B * n, W), torch.int64) if dc else None
        t["cover_bits"] = z((B, W), torch.int64) if dc else None
        # where the fused policy+step launches record the actions they drew (record_actions=True); off by default: 8 bytes
        # per slot and step less to write
        t["actions_out"] = z((B,), torch.int64) if record_actions else None
        t["stream_state"] = z((B, 2, _lib.STREAM_WORDS), torch.int32) if self.continue_streams else None
        t["eval_scratch"] = z((lay.eval_scratch_bytes,), torch.uint8) if lay.eval_scratch_bytes else None  # TSP is_eval_env: Christofides work space
        t["prune_scratch"] = z((lay.prune_scratch_words,), torch.int64) if lay.prune_scratch_words else None  # node sets of the residual-graph walks (registers up to 512 nodes)
        if _views:  # slabs shared with sibling engines of other geometries (RaggedVectorEnv)
            for k, v in _views.items():
                if t[k] is None:
                    continue
                assert v.dtype == t[k].dtype and v.numel() >= (t[k].numel() if k != "edge_index" else 0), k
                t[k] = v
        self.node_id_base = int(node_id_base)
        self.t = t = _Slabs((k, t[k]) for k in _lib.BUFFER_FIELDS)  # (in ge_buffers' order; a field without a line above is a KeyError)
        self.bufs = _lib.buffers(t)
        h = C.c_void_p()
        if not _defer_create:  # (a size class of a multi-class engine is created by RaggedVectorEnv, all classes at once)
            _lib.check(self._L, self._L.ge_create(C.byref(self.cfg), C.byref(self.bufs), C.byref(h)), "ge_create")
        self._h = h
        # episode prefetch (include/graphenvs.h, ge_attach_spares): every slot's NEXT episode is generated ahead of time into a spare
        # image, `prefetch` steps' worth of finished slots per launch, and moved in by one copy when the slot finishes.  Same outputs
        # with and without; it pays where few slots finish per step (long episodes, large graphs), where a regeneration in place
        # makes the whole step wait for the latency of a few slots.  None = the engine's choice for this env id and size, 0 = off.
        if prefetch is None:  # (the CPU sanitizer harness runs without it unless a test asks: it only doubles the work of a reset there)
            prefetch = self.default_prefetch(env_id, self.n, self.num_envs) if _library is None else 0
        self.prefetch = int(prefetch)
        if not self.autoreset or self.continue_streams:
            self.prefetch = 0
        self.spare = None
        if self.prefetch and not _defer_create:
            self._attach_spares()
        # static parts of the PyG view
        self._batch = torch.arange(B, device=dev, dtype=torch.int64).repeat_interleave(n)
        self._ptr = torch.arange(B + 1, device=dev, dtype=torch.int64) * n + int(node_id_base)
        self._truncated = torch.zeros(B, dtype=torch.bool, device=dev)
        self._actions_scratch = z((B,), torch.int64)
        self._was_reset = False
        self._streams = False  # stream_state holds the streams of a reset (continue_streams)
        self.single_action_space = _Space(n=(self.m if edge_env else n), mask_size=A)  # steiner_tree.py:43, multicast_routing.py:67
        self.single_observation_space = _Space(shape=(self.obs_len,), dtype=np.float32)
        if _GYM is not None and hasattr(_GYM, "spaces"):  # the reference's spaces (shortest_path.py:40-42), and their batched forms
            sp = _GYM.spaces
            self.single_action_space = sp.Discrete(self.m if edge_env else n)
            self.single_observation_space = sp.Box(low=-np.inf, high=np.inf, shape=(self.obs_len,), dtype=np.float32)
            self.action_space = sp.MultiDiscrete([self.m if edge_env else n] * B) if hasattr(sp, "MultiDiscrete") else None
            self.observation_space = sp.Box(low=-np.inf, high=np.inf, shape=(B, self.obs_len), dtype=np.float32)
            self.metadata = {"autoreset_mode": {0: "disabled", 1: "same_step", 2: "next_step"}[self.autoreset_mode]}

    @staticmethod
    def default_prefetch(env_id, n, num_envs):
        """refill period chosen when the caller does not say (0 = regenerate in place).  Prefetch pays when FEW slots finish per
        step -- a regeneration in place then costs the whole step the latency of those few -- and loses when thousands do (the
        reset kernels already fill the chip; the copy and the slots that finish twice inside a period are pure overhead).  The
        estimate: slots / a typical episode length under a random policy (measured, profiles/README.md round 3)."""
        length = {"ShortestPath-v0": 0.39 * n, "LongestPath-v0": 0.39 * n, "SteinerTree-v0": 0.8 * n, "MulticastRouting-v0": 0.5 * n,
                  "MaxIndependentSet-v0": 1.0 * n, "DensestSubgraph-v0": 0.36 * n, "DistributionCenter-v0": 6.0,
                  "PerishableProductDelivery-v0": 80.0 * n}.get(env_id)
        if length is None:  # TSP: every slot of a batch finishes in the same step -- one burst per episode, nothing to batch
            return 0
        per_step = num_envs / max(length, 1.0)
        if per_step >= 600:
            return 0
        # ~2 500 regenerations per refill: on BASELINE config 4 (~70 slots finish per step) the steady state gives 52 / 57 / 60 / 62.6 /
        # 58.6 / 56 M env-steps/s at periods 4 / 8 / 16 / 32 / 64 / 128 (bench.py --config c4 --prefetch P, value_200)
        # ... but never longer than about half an episode: a slot that finishes again before the refill takes the (throttled) path
        # in place, and with short episodes every refill would regenerate about every image anyway (DistributionCenter at 1 000
        # slots: 15 -> 3; ShortestPath n = 10 at 256 slots: 39 -> 2)
        period = min(128.0, max(4.0, 2560 / max(per_step, 1.0)), max(2.0, length / 2))
        return int(period)

    def _image_tensors(self, views=None):
        """a second set of the per-slot slabs (ge_spares.image); `views`: slabs given by the caller (multi-class engine)"""
        img = {}
        for k in _lib.IMAGE_FIELDS:
            live = dict.__getitem__(self.t, k)
            img[k] = None if live is None else (views[k] if views and k in views else torch.zeros_like(live))
        return img

    def _attach_spares(self):
        img, sp = self._image_tensors(), spare_queues(self.num_envs, self.device)
        self.spare = dict(image=img, **sp)
        self._call("ge_attach_spares", C.byref(_lib.spares(img, sp, self.prefetch)), None)

    # ------------------------------------------------------------------ views
    def graph(self):
        t = self.t
        return GraphBatch(x=t["x"], edge_index=t["edge_index"], edge_attr=t["edge_attr"], batch=self._batch,
                          ptr=self._ptr, num_graphs=self.num_envs)

    def flat_obs(self):
        """utils.vectorize_graph of every slot: float32 [B, obs_len] (utils.py:87-88)."""
        return self._vectorized((self.num_envs, self.obs_len))

    def _obs(self):
        return self.flat_obs() if self.obs_mode == "flat" else self.graph()

    @property
    def mask(self):
        return self.t["mask"].view(torch.bool)

    def graph_obs(self):
        """info['graph_obs'] of the reference (shortest_path.py:94-95: the live GraphInstance), batched: ``nodes`` [B, n, F],
        ``edges`` [B, E, Fe] as views of the observation slabs and ``edge_links`` [B, E, 2] local node ids."""
        t = self.t
        return SimpleNamespace(nodes=t["x"].view(self.num_envs, self.n, self.F),
                               edges=t["edge_attr"].view(self.num_envs, self.E, self.Fe), edge_links=self.edge_links())

    @staticmethod
    def _copied(out):
        def cp(v):
            if torch.is_tensor(v):
                return v.clone()
            if isinstance(v, dict):
                return {k: cp(x) for k, x in v.items()}
            if isinstance(v, (GraphBatch, SimpleNamespace)):
                return type(v)(**{k: cp(x) for k, x in v.__dict__.items()})
            return v
        return tuple(cp(v) for v in out)

    def _info(self, stepped):
        t = self.t
        info = {"mask": self.mask, "mask_bits": t["mask_bits"]}
        if self.return_graph_obs:
            info["graph_obs"] = self.graph_obs()
        if stepped:
            info.update(solved=t["solved"], solution_cost=t["final_cost"], heuristic_solution=t["final_heur"],
                        invalid_action=t["invalid"].view(torch.bool), episode_length=t["final_len"])
        return info

    # ------------------------------------------------------------------ gym surface
    def _seed_tensor(self, seed):
        if seed is None:
            if not self._was_reset:
                seed = 0
            else:  # next episode of every slot
                seed = (self.t["seed"].cpu().numpy().view(np.uint32).astype(np.int64) + self.seed_stride) % (1 << 32)
        return slot_seeds(seed, self.num_envs, self.env_index_base, self.device)

    def reset(self, seed=None, options=None):
        """reset(seed=s): slot i (global index g) runs the reference's reset(seed=(s+g) mod 2^32); a
        sequence/tensor gives every slot its own seed.  reset() without a seed: see ``continue_streams``."""
        if seed is None and self._streams:
            self._call("ge_reset_continue", self._stream())
        else:
            self._seeds_keepalive = seeds = self._seed_tensor(seed)
            self._call("ge_reset", seeds.data_ptr(), self._stream())
            self._was_reset = True
            self._streams = self.continue_streams
        out = (self._obs(), self._info(False))
        return self._copied(out) if self.copy_outputs else out

    def step(self, actions):
        """One transition of every slot.  The returned reward / terminated / info tensors (and the observation) ALIAS engine
        slabs that the next step() overwrites -- unlike a gymnasium VectorEnv, which returns fresh arrays: ``.clone()`` what a
        rollout buffer keeps across steps (or construct the env with ``copy_outputs=True``)."""
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions, dtype=np.int64))
        actions = actions.to(device=self.device, dtype=torch.int64).contiguous()
        assert actions.shape == (self.num_envs,)
        assert self._was_reset, "call reset() (or inject_state()) before step()"
        self._act_keepalive = actions
        self._call("ge_step", actions.data_ptr(), self._stream())
        return self._after_step()

    def _policy_numel(self):
        return self.num_envs * self.A

    def _after_step(self, extra=None):
        """what step() returns once the step is launched (`extra`: more entries of info)"""
        t = self.t
        if self.strict and bool(t["invalid"].any()):
            bad = torch.nonzero(t["invalid"]).flatten().tolist()
            raise AssertionError(f"invalid action in slots {bad[:8]} (the reference asserts here)")
        info = self._info(True)
        if extra:
            info.update(extra)
        out = (self._obs(), t["reward"], t["terminated"].view(torch.bool), self._truncated, info)
        return self._copied(out) if self.copy_outputs else out

    # ------------------------------------------------------------------ extras
    def timed_step_burst_raw_ms(self, k, policy_seed=0):
        """elapsed ms between one pair of HIP events around k back-to-back (sample+)step launches (k = 0: the bare
        event pair, i.e. the measurement overhead)."""
        ms = C.c_double()
        self._call("ge_timed_step_burst", int(policy_seed), int(k), self._actions_scratch.data_ptr(), self._stream(), C.byref(ms))
        return ms.value

    def timed_step_burst(self, k, policy_seed=0):
        """k back-to-back (sample+)step launches between one pair of HIP events, no autoreset in between; returns
        the average launch duration in microseconds."""
        return self.timed_step_burst_raw_ms(k, policy_seed) * 1e3 / k

    def launch_floor_us(self, k=5, reps=9):
        """what an EMPTY launch of the step kernel's shape takes (median of `reps` bursts of k), microseconds"""
        ms, vals = C.c_double(), []
        empty = sorted(self.timed_step_burst_raw_ms(0) for _ in range(reps))[reps // 2]
        for _ in range(reps):
            self._call("ge_timed_empty_burst", int(k), self._stream(), C.byref(ms))
            vals.append((ms.value - empty) * 1e3 / k)
        return sorted(vals)[reps // 2]

    def inject_state(self, links, wcode, x, terminals=None, seeds=None):
        """Parity path: load post-reset states produced elsewhere (links [B,E,2] local ids, wcode [B,E] in
        {3..10}, x [B,n,F], terminals [B,T]).  ``seeds`` [B] (optional): the seed each injected episode is taken to have;
        autoreset then continues with reset(seed + seed_stride), ... -- required on an engine with autoreset that was
        never reset()."""
        dev = self.device
        links_np, wcode_np = np.asarray(links), np.asarray(wcode)
        # the kernel indexes LDS rows with these: refuse what the reference could never produce
        assert links_np.min() >= 0 and links_np.max() < self.n, "edge_links must hold local node ids in [0, n_nodes)"
        assert wcode_np.min() >= 3 and wcode_np.max() <= 10, "weight codes are k with weight k/10.0, k in 3..10"
        # the graphs are undirected: the step kernels read the weight of u -> v from either end
        Bn = links_np.shape[0]
        wmat = np.zeros((Bn, self.n, self.n), dtype=np.uint8)
        bi = np.arange(Bn)[:, None]
        wmat[bi, links_np[..., 0], links_np[..., 1]] = wcode_np
        assert np.array_equal(wmat, wmat.transpose(0, 2, 1)), "edge weights must be symmetric (weight(u,v) == weight(v,u))"
        links = torch.as_tensor(links_np, dtype=torch.int64).to(dev).contiguous()
        wcode = torch.as_tensor(np.asarray(wcode), dtype=torch.uint8).to(dev).contiguous()
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev).contiguous()
        term = None
        if terminals is not None:
            term_np = np.asarray(terminals)
            assert term_np.min() >= -1 and term_np.max() < self.n, "terminals are local node ids (-1: unused tail)"
            term = torch.as_tensor(term_np, dtype=torch.int32).to(dev).contiguous()
            assert term.shape == (self.num_envs, self.T)
        assert links.shape == (self.num_envs, self.E, 2) and wcode.shape == (self.num_envs, self.E)
        assert x.shape == (self.num_envs, self.n, self.F)
        sd = None if seeds is None else slot_seeds(seeds, self.num_envs, 0, dev)
        self._inj_keepalive = (links, wcode, x, term, sd)
        self._call("ge_inject_state", links.data_ptr(), wcode.data_ptr(), x.data_ptr(), term.data_ptr() if term is not None else None,
                   sd.data_ptr() if sd is not None else None, self._stream())
        self._was_reset = True
        return self._obs(), self._info(False)

    def state_dict(self):
        """Snapshot of every engine slab: the whole state of the batch, generator states included."""
        self._quiesce()
        sd = {k: v.clone() for k, v in dict.items(self.t) if v is not None and k not in ("eval_scratch", "prune_scratch")}  # work space, not state
        if self.spare is not None:  # the images themselves are not state (they are regenerated); the marker says which invariant the generator ring obeys
            sd["_prefetch"] = torch.ones((), dtype=torch.int32)
        return sd

    def load_state_dict(self, sd):
        self._quiesce()
        # an engine with spares seeds its generator ring one episode later than one without: a snapshot of the former only restores
        # into an engine with spares (the other direction is fine)
        assert "_prefetch" not in sd or self.spare is not None, "snapshot of an engine with prefetch: restore into an engine with prefetch"
        for k, v in sd.items():
            if k != "_prefetch":
                dict.__getitem__(self.t, k).copy_(v)
        if self.spare is not None:
            self.spare["state"].zero_()  # every image is regenerated at the next opportunity
            # next-step autoreset: a slot that finished in the snapshot's last step waits for its regeneration (status 2), queued
            # either for the regeneration in place (reset_list, part of the snapshot) or -- it had a valid image -- for the swap
            # (swap_list, which is not: the images are gone).  Every such slot goes through the regeneration queue, in the layout the
            # step kernels write (a segment per QUEUE_BLOCK slots, slot order), and this engine's own swap queue is emptied.
            self.spare["swap_count"].zero_()
            B, QB = self.num_envs, _lib.QUEUE_BLOCK
            fin = (self.t["status"] == 2).to(torch.int32)
            pad = torch.zeros(_lib.queue_blocks(B) * QB, dtype=torch.int32, device=self.device)
            pad[:B] = fin
            blocks = pad.view(-1, QB)
            rank = torch.cumsum(blocks, dim=1) - blocks
            slot = torch.arange(pad.numel(), device=self.device, dtype=torch.int32).view(-1, QB)
            pos = (slot - slot % QB + rank)[blocks.bool()].to(torch.int64)
            dict.__getitem__(self.t, "reset_list")[pos] = slot[blocks.bool()]
            dict.__getitem__(self.t, "reset_count").copy_(blocks.sum(dim=1).to(torch.int32))
        self._call("ge_mark_restored")
        self._was_reset = True
        self._streams = self.continue_streams and "stream_state" in sd
        self._quiesce()

    def check_device_errors(self):
        """Raise if a kernel flagged an error it could not report otherwise (synchronises): bit 0 = a G(n, m) rejection loop
        hit its round cap (generator state never seeded or corrupted); the slot's status is 4 and it stays frozen."""
        flags = int(self.t["work_count"][1].item())
        if flags:
            raise RuntimeError(f"graphenvs_amd: device error flags {flags:#x} (bit 0: graph generation gave up -- unseeded generator state?)")

    def edge_links(self):
        """[B, E, 2] local node ids (GraphInstance.edge_links of every slot)."""
        assert self.cfg.edge_row_stride in (0, self.num_envs * self.E), "use RaggedVectorEnv.edge_links for shared slabs"
        ei = self.t["edge_index"].view(2, self.num_envs, self.E)
        off = (torch.arange(self.num_envs, device=self.device, dtype=torch.int64) * self.n + self.node_id_base).view(1, -1, 1)
        return (ei - off).permute(1, 2, 0).contiguous()


def make_vec(env_id, num_envs, shards=1, **kwargs):
    """``shards`` > 1: the batch as that many independent engines on their own HIP streams (graphenvs_amd.sharded.ShardedVectorEnv)"""
    if shards is not None and int(shards) > 1:
        from .sharded import ShardedVectorEnv
        return ShardedVectorEnv(env_id, num_envs, shards=int(shards), **kwargs)
    return VectorGraphEnv(env_id, num_envs, **kwargs)
