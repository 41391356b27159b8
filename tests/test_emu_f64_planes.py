"""CPU harness (tests/emu): the level-3 path counts of the n <= 64 feature kernel's forward Brandes pull from bit planes
(GE_F64_PLANES) against a build of the same sources without them, and a sample of slots against the C oracle.  Bodies and shapes:
tests/f64_planes_check.py (tests/test_gpu_f64_planes.py runs them with 256 slots on the MI355X)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402
import f64_planes_check as pc  # noqa: E402
import seed_ring_check as rc  # noqa: E402

import graphenvs_amd as ge  # noqa: E402

# the harness runs a walk item's 256 lanes as fibers of one CPU thread: eight slots and four steps per shape here, 256 slots on the GPU
B, K = 8, 4
# what eight slots in four steps do not show (the seeds are fixed, so this is known, not chance): no episode of n64-m192, n64-m400,
# n40-m200 or n33-m70 ends, so their queue launch is compared on the GPU only -- here the reset's launch over all eight slots is; and no
# slot of n28-m32 is deeper than GE_F64_LV, so a non-empty list is compared on the GPU only
GPU_ONLY = {"n64-m192": dict(regen=False), "n64-m400": dict(regen=False), "n40-m200": dict(regen=False), "n33-m70": dict(regen=False),
            "n28-m32": dict(listed=False)}
# wave-round classes that the eight slots do not show (none: every class a shape is here for occurs among its eight slots)
GPU_ONLY_COVER = {}


@pytest.fixture(scope="module")
def libs():
    out = lambda name: os.path.join(os.path.dirname(build_emu.OUT), "libgraphenvs_emu_planes_%s.so" % name)
    return dict(product=build_emu.load(), **{name: build_emu.load(extra=flags, out=out(name)) for name, flags in pc.VARIANTS.items()})


@pytest.mark.parametrize("name,n,m,want,cover", pc.SHAPES, ids=[s[0] for s in pc.SHAPES])
def test_emulated_planes_leave_the_bytes_of_the_baseline(libs, name, n, m, want, cover):
    cover = tuple(c for c in cover if c not in GPU_ONLY_COVER.get(name, ()))
    st = pc.check_planes(rc.uniform(ge, "cpu", pc.SP, dict(n_nodes=n, n_edges=m), B), libs, pc.SP, K, range(B), cover)
    print(st)
    pc.expect(st, dict(want, **GPU_ONLY.get(name, {})), cover)


def test_emulated_planes_leave_the_bytes_of_the_baseline_in_a_two_class_engine(libs):
    """classes n = 24 and n = 64: the RAGGED instantiation of ge_k_features64"""
    cover = ("third",)
    st = pc.check_planes(rc.ragged(ge, "cpu", pc.SP, [(4, 24, 50), (4, 64, 192)], {}), libs, pc.SP, K, range(8), cover)
    print(st)
    pc.expect(st, dict(unlisted=True), cover)
