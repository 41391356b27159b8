"""GPU (MI355X): the level-3 path counts of the n <= 64 feature kernel's forward Brandes pull from bit planes (GE_F64_PLANES)
against a -DGE_F64_PLANES=0 build of the same sources, and a sample of slots against the C oracle.  Bodies and shapes:
tests/f64_planes_check.py (tests/test_emu_f64_planes.py runs them on the CPU harness)."""
import ctypes
import os
import subprocess

import pytest

import f64_planes_check as pc
import seed_ring_check as rc

pytestmark = pytest.mark.gpu

B, K = 256, 4
SAMPLE = (0, 1, 63, 64, 127, 200, 255)


def _ge():
    import graphenvs_amd as ge
    return ge


@pytest.fixture(scope="module")
def libs():
    """the library of the same sources built with the switch off, beside the product; compiled when there is none of these sources"""
    from graphenvs_amd import _lib
    out = {name: os.path.join(os.path.dirname(_lib.LIB_PATH), "libgraphenvs_hip_planes_%s.so" % name) for name in pc.VARIANTS}
    for name, flags in pc.VARIANTS.items():
        if _lib.built_hash(out[name]) != _lib.source_hash():
            tmp = "%s.%d.tmp" % (out[name], os.getpid())
            subprocess.check_call(_lib.compile_command(tmp, flags), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            os.replace(tmp, out[name])
    return dict(product=None, **{name: _lib.bind(ctypes.CDLL(path)) for name, path in out.items()})  # None: the product (the switch defaults to 1)


@pytest.mark.parametrize("name,n,m,want,cover", pc.SHAPES, ids=[s[0] for s in pc.SHAPES])
def test_planes_leave_the_bytes_of_the_baseline(libs, name, n, m, want, cover):
    st = pc.check_planes(rc.uniform(_ge(), "cuda", pc.SP, dict(n_nodes=n, n_edges=m), B), libs, pc.SP, K, SAMPLE, cover)
    print(st)
    pc.expect(st, want, cover)


def test_planes_leave_the_bytes_of_the_baseline_in_a_two_class_engine(libs):
    """classes n = 24 and n = 64: the RAGGED instantiation of ge_k_features64"""
    cover = ("third",)
    st = pc.check_planes(rc.ragged(_ge(), "cuda", pc.SP, [(120, 24, 50), (136, 64, 192)], {}), libs, pc.SP, K, SAMPLE, cover)
    print(st)
    pc.expect(st, dict(unlisted=True), cover)
