"""CPU: the shape and dtype of every slab the host layer allocates -- the live slabs of uniform engines of all nine ids under each
option that adds or removes one, the spare images and queues, and the shared slabs, per-class views and offsets of multi-class
engines -- equal what tests/slab_layout.json recorded (tools/record_slab_layout.py, on the kernels' CPU harness).  A slab that comes
out smaller than the kernels were written for is an out-of-bounds write on the GPU; this fails first, without one."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_slab_layout as rec  # noqa: E402

with open(os.path.join(ROOT, "tests", "slab_layout.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def mods():
    return rec.load_modules()


def _same(got, want, where):
    """key for key, so that a failure names the slab"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (where, sorted(got or ()), sorted(want))
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list) and want and isinstance(want[0], dict):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    else:
        assert got == want, (where, got, want)


def test_the_plan_is_the_recorded_one():
    assert sorted(rec.plan()) == sorted(RECORDED)


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_slabs_have_the_recorded_shapes_and_dtypes(mods, name):
    got = json.loads(json.dumps(rec.collect(*mods, name)))  # (tuples -> lists, like the file)
    _same(got, RECORDED[name], name)
