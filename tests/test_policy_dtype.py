"""CPU: the policy head on bfloat16 / float16 logits with a temperature, compiled for the sanitizer harness (tests/emu) -- the bodies of
tests/policy_dtype_check.py at the harness's slot counts (70 / 20 / 3, the multi-class cases at an eighth), every case for both 16-bit
types and three temperatures; and the 16-bit conversions of ge_platform.h, walked over every word by a stand-alone program.  The
GPU runs the same bodies in tests/test_gpu_policy_dtype.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
import build_emu  # noqa: E402
import policy_dtype_check as dc  # noqa: E402
import policy_head_check as pc  # noqa: E402

import graphenvs_amd as ge  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return build_emu.load()


@pytest.fixture(scope="module")
def engines():
    """one engine per case for its six (dtype, temperature) entries (policy_dtype_check.check_engine)"""
    kept = {}
    yield kept
    for env in kept.values():
        env.close()


@pytest.mark.parametrize("T", dc.TEMPERATURES)
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("env_id,kw,B_gpu,B", dc.CASES)
def test_policy_dtype_rows(emu, engines, env_id, kw, B_gpu, B, dtype, T):
    # (a harness step of the three 2 048-action rows takes six seconds: one step between the two passes there, three elsewhere)
    dc.check_uniform(ge, "cpu", emu, env_id, kw, B, dtype, T, steps=1 if B == 3 else 3, shared=engines, key=(env_id, str(kw)))


def _shrunk(sizes):
    """the multi-class cases with an eighth of the slots: 9 / 17 / 13 -- classes still share waves and workgroups"""
    return [((e[0] + 7) // 8,) + tuple(e[1:]) for e in sizes]


@pytest.mark.parametrize("T", dc.TEMPERATURES)
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("env_id,sizes,prefetch", dc.RAGGED)
def test_policy_dtype_multi_class(emu, engines, env_id, sizes, prefetch, dtype, T):
    dc.check_ragged(ge, "cpu", emu, env_id, _shrunk(sizes), prefetch, dtype, T, shared=engines, key=(env_id, str(sizes)))


def test_step_policy_16bit_distribution_center(emu):
    """DistributionCenter, n <= 64: the coverage-range kernel sits between the policy and the step"""
    make = lambda: ge.VectorGraphEnv(pc._DC, 20, n_nodes=64, n_edges=192, seed_stride=pc.STRIDE, env_index_base=pc.BASE, device="cpu", _library=emu)
    dc.check_step_policy(ge, "cpu", make, torch.bfloat16, 0.7)


def test_step_policy_16bit_multi_class(emu):
    make = lambda: ge.RaggedVectorEnv(pc._SP, [(5, 12, 30), (9, 33, 80), (6, 70, 200)], seed_stride=pc.STRIDE, env_index_base=pc.BASE,
                                      device="cpu", _library=emu)
    dc.check_step_policy(ge, "cpu", make, torch.float16, 3.0)


def test_two_engines_over_the_halves_equal_one_bf16(emu):
    B, kw = 70, dict(n_nodes=12, n_edges=30, device="cpu", _library=emu)
    one = ge.VectorGraphEnv(pc._SP, B, **kw)
    halves = [ge.VectorGraphEnv(pc._SP, B // 2, env_index_base=k * (B // 2), seed_stride=B, **kw) for k in range(2)]
    dc.check_halves_equal_one(one, ge.MixedVectorEnv(halves), "cpu", torch.bfloat16, 0.7)


def test_policy_dtype_errors(emu):
    dc.check_errors(ge, "cpu", emu)


# ------------------------------------------------------------------------------------------ the conversions (no engine)
def _float32_samples(rng, n=1 << 20):
    """finite float32 values: random words, values around every 16-bit rounding boundary (the exact halfway cases and their float32
    neighbours) and the edges of both ranges"""
    words = rng.integers(0, 1 << 32, size=n - (1 << 18), dtype=np.uint64).astype(np.uint32)
    parts = [words.view(np.float32)]
    for dtype, count in ((torch.bfloat16, 1 << 16), (torch.float16, 1 << 16)):
        w = torch.from_numpy(rng.integers(0, 1 << 16, size=count, dtype=np.int64).astype(np.uint16).view(np.int16))
        lo = w.view(dtype).float().numpy()
        nxt = (w + 1).view(dtype).float().numpy()  # (the next word of the same sign: the neighbour away from zero)
        with np.errstate(all="ignore"):
            mid = ((lo.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)  # exact in float32: a halfway case
        parts += [mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf) * np.sign(mid))]
    edge = np.array([0.0, -0.0, 65504.0, 65519.996, 65520.0, 65536.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -14, 6.0975e-5,
                     3.3895314e38, 3.4028235e38, 1e-45, 1.1754944e-38], dtype=np.float32)
    parts += [edge, -edge]
    x = np.concatenate(parts).astype(np.float32)
    return x[np.isfinite(x)]


def test_conversion_helpers_equal_torch(tmp_path):
    exe = str(tmp_path / "policy_dtype_conv")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DGE_EMU", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(HERE, "emu"), "-I" + build_emu.CSRC, os.path.join(HERE, "policy_dtype_conv.cpp"), "-o", exe])
    x = _float32_samples(np.random.default_rng(16))
    assert len(x) >= 1_000_000
    x.tofile(str(tmp_path / "in_f32.bin"))
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.returncode, run.stderr[-2000:])
    lines = dict(l.split(" ", 1) for l in run.stdout.strip().splitlines())
    words = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)  # every word, as torch's int16
    order = words.numpy().view(np.uint16).astype(np.int64)
    for name, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        want_up = np.empty(65536, dtype=np.float32)
        want_up[order] = words.view(dtype).float().numpy()
        nan = np.isnan(want_up)
        assert int(nan.sum()) == {"bf16": 254, "f16": 2046}[name]
        up = np.fromfile(str(tmp_path / f"up_{name}.bin"), dtype=np.float32)
        assert np.array_equal(up.view(np.uint32)[~nan], want_up.view(np.uint32)[~nan]), name
        assert np.isnan(up[nan]).all()
        lost = [int(w) for w in lines[name].split("lost", 1)[1].split()]
        assert all(nan[w] for w in lost), (name, "a non-NaN word does not survive up-then-down", [w for w in lost if not nan[w]][:8])
        down = np.fromfile(str(tmp_path / f"down_{name}.bin"), dtype=np.uint16)
        want_down = torch.from_numpy(x).to(dtype).view(torch.int16).numpy().view(np.uint16)
        bad = np.flatnonzero(down != want_down)
        assert not len(bad), (name, len(bad), x[bad[:4]], down[bad[:4]], want_down[bad[:4]])
