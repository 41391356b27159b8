"""Shapes and dtypes of every slab the host layer allocates, for a fixed list of small engines built on the kernels' CPU harness
(tests/emu, no GPU).  Run at a commit whose allocations are trusted, it writes tests/slab_layout.json; tests/test_slab_layout.py
builds the same engines and compares key for key, so that a host-side change cannot quietly hand a kernel a smaller slab.
usage: python tools/record_slab_layout.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "slab_layout.json")

# the kwargs an id needs to be constructed (tools/ragged_all_envs.py), MulticastRouting with the parenting that has a node_aux slab
IDS = {
    "ShortestPath-v0": {}, "LongestPath-v0": dict(parenting=2), "SteinerTree-v0": dict(n_dests=3), "TSP-v0": dict(parenting=1),
    "DensestSubgraph-v0": dict(parenting=1), "MaxIndependentSet-v0": {}, "MulticastRouting-v0": dict(parenting=4),
    "DistributionCenter-v0": dict(parenting=2), "PerishableProductDelivery-v0": dict(parenting=1),
}
OPTIONS = {"defaults": {}, "prefetch4": dict(prefetch=4), "record_actions": dict(record_actions=True),
           "continue_streams": dict(continue_streams=True)}
QUEUES = ("state", "swap_list", "swap_count", "refill_list", "refill_count")
RAGGED_SIZES = [(3, 10, 20), (2, 12, 24)]


def desc(v):
    return None if v is None else [list(v.shape), str(v.dtype)]


def descs(d):
    return {k: desc(v) for k, v in dict.items(d)}


def uniform(ge, emu, env_id, n, m, **kw):
    env = ge.VectorGraphEnv(env_id, 5, n, m, device="cpu", _library=emu, **kw)
    out = {"t": descs(env.t), "spare": None}
    if env.spare is not None:
        out["spare"] = dict(image=descs(env.spare["image"]), **{k: desc(env.spare[k]) for k in QUEUES})
    env.close()
    return out


def ragged(ge, emu, env_id, prefetch, **kw):
    env = ge.RaggedVectorEnv(env_id, RAGGED_SIZES, device="cpu", _library=emu, prefetch=prefetch, **kw)
    out = {k: desc(getattr(env, k)) for k in ("x", "edge_index", "edge_attr", "mask_flat")}
    out.update(g=descs(env.g), classes=[descs(c.t) for c in env.classes], offsets=[list(o) for o in env._offsets], spare=None)
    if env.spare is not None:
        out["spare"] = dict(images=[descs(i) for i in env.spare["images"]], shared=descs(env.spare["shared"]),
                            **{k: desc(env.spare[k]) for k in QUEUES})
    env.close()
    return out


def plan():
    """{case name: (builder, args, kwargs)}: per id the four options at (10, 20), the defaults at (70, 140) -- two adjacency words,
    where the one-word slabs go away --, a two-class RaggedVectorEnv without and with spares; and TSP's spatial / eval-only slabs"""
    cases = {}
    for env_id, kw in IDS.items():
        for name, opt in OPTIONS.items():
            cases[f"{env_id} n10 {name}"] = (uniform, (env_id, 10, 20), dict(opt, **kw))
        cases[f"{env_id} n70 defaults"] = (uniform, (env_id, 70, 140), kw)
        for prefetch in (0, 4):
            cases[f"{env_id} ragged prefetch{prefetch}"] = (ragged, (env_id, prefetch), kw)
    cases["TSP-v0 n10 spatial eval prefetch4"] = (uniform, ("TSP-v0", 10, 20), dict(parenting=2, spatial=True, is_eval_env=True, prefetch=4))
    return cases


def collect(ge, emu, name):
    fn, args, kw = plan()[name]
    return fn(ge, emu, *args, **kw)


def load_modules():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "emu")]
    import build_emu
    import graphenvs_amd as ge
    return ge, build_emu.load()


if __name__ == "__main__":
    mods = load_modules()
    cases = {name: collect(*mods, name) for name in plan()}
    with open(OUT, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in cases.items()) + "\n}\n")
    print(f"{len(cases)} cases -> {OUT}")
