"""CPU harness (tests/emu): the shortcut of the n <= 64 feature kernel's forward Brandes pull (GE_F64_L2POP) against a build of the
same sources without it, and a sample of slots against the C oracle.  Bodies and shapes: tests/f64_shortcuts_check.py
(tests/test_gpu_f64_shortcuts.py runs them with 256 slots on the MI355X)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import build_emu  # noqa: E402
import f64_shortcuts_check as sc  # noqa: E402
import seed_ring_check as rc  # noqa: E402

import graphenvs_amd as ge  # noqa: E402

# the harness runs a walk item's 256 lanes as fibers of one CPU thread: eight slots and four steps per shape here, 256 slots on the GPU
B, K = 8, 4
# what eight slots in four steps do not show (the seeds are fixed, so this is known, not chance): no episode of n64-m192 or n33-m70
# ends, so their queue launch is compared on the GPU only -- here the reset's launch over all eight slots is; and no slot of n28-m32 is
# deeper than GE_F64_LV, so a non-empty list is compared on the GPU only
GPU_ONLY = {"n64-m192": dict(regen=False), "n33-m70": dict(regen=False), "n28-m32": dict(listed=False)}


@pytest.fixture(scope="module")
def libs():
    out = lambda name: os.path.join(os.path.dirname(build_emu.OUT), "libgraphenvs_emu_f64_%s.so" % name)
    return dict(product=build_emu.load(), **{name: build_emu.load(extra=flags, out=out(name)) for name, flags in sc.VARIANTS.items()})


@pytest.mark.parametrize("name,n,m,want", sc.SHAPES, ids=[s[0] for s in sc.SHAPES])
def test_emulated_shortcut_leaves_the_bytes_of_the_baseline(libs, name, n, m, want):
    st = sc.check_shortcuts(rc.uniform(ge, "cpu", sc.SP, dict(n_nodes=n, n_edges=m), B), libs, sc.SP, K, range(B))
    print(st)
    sc.expect(st, dict(want, **GPU_ONLY.get(name, {})))


def test_emulated_shortcut_leaves_the_bytes_of_the_baseline_in_a_two_class_engine(libs):
    """classes n = 24 and n = 64: the RAGGED instantiation of ge_k_features64"""
    st = sc.check_shortcuts(rc.ragged(ge, "cpu", sc.SP, [(4, 24, 50), (4, 64, 192)], {}), libs, sc.SP, K, range(8))
    print(st)
    sc.expect(st, dict(unlisted=True))
