"""Every row of tests/golden/gemm_f32_routes.json run once on the GPU: the launch counters rise as they were recorded on the commit
before the router became a pure function (see test_gemm_route_cpu.py), and C equals the double-buffered kernels' result
(w2v2_op_gemm_variant 0) on the same inputs bit for bit."""

import ctypes as C
import json
import os

import pytest

from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_f32_routes.json")
ROWS = [r for r in json.load(open(GOLDEN)) if r["recorded"] is not None]


@pytest.fixture(scope="module")
def env():
    import torch
    import wav2vec2
    import helpers as H
    torch.cuda.set_device(0)
    lib = N.load()
    model = wav2vec2.Wav2Vec2ForCTC(wav2vec2.Wav2Vec2Config(**H.TINY), input_shape=(1, 4000))      # any model: its profiler reads the family counter
    names = list(model.profile_read())
    return lib, torch, torch.device("cuda:0"), model, names.index("gemm_f32")


def counters(env):
    lib, _, _, model, fam = env
    c = (C.c_int64 * 4)()
    N.check(lib.w2v2_op_gemm_ring_launches(c))
    k = C.c_int64()
    N.check(lib.w2v2_profile_kernel_launches(model._handle, fam, C.byref(k)))
    return list(c), k.value


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row_reaches_the_recorded_kernels_with_the_double_buffers_bits(env, row):
    lib, torch, dev, _, _ = env
    g = torch.Generator(device=dev).manual_seed(0)
    M, N_, K, nb = row["M"], row["N"], row["K"], row["nbatch"]
    A = torch.randn((nb - 1) * row["strideA"] + (M - 1) * row["lda"] + K, generator=g, device=dev)
    B = torch.randn(K * N_, generator=g, device=dev)
    bias = torch.randn(N_, generator=g, device=dev) if row["bias"] else None
    res = torch.randn(nb * M * N_, generator=g, device=dev) if row["residual"] else None

    def run(variant, by_shape=False):
        out = torch.full((nb * M * N_,), float("nan"), device=dev)
        args = (N.ptr(A), row["lda"], row["strideA"], N.ptr(B), N_, N.ptr(out), N_, M * N_, N.ptr(bias), N.ptr(res), M, N_, K, nb, row["act"])
        if by_shape:
            N.check(lib.w2v2_op_gemm(*args, N.current_stream()))
        else:
            N.check(lib.w2v2_op_gemm_variant(*args, variant, N.current_stream()))
        torch.cuda.synchronize()
        return out

    ring0, launches0 = counters(env)
    out = run(row["variant"], by_shape=row["variant"] < 0)
    ring1, launches1 = counters(env)
    assert ([b - a for a, b in zip(ring0, ring1)], launches1 - launches0) == (row["recorded"]["ring"], row["recorded"]["launches"])
    ref = run(0)
    assert torch.isfinite(ref).all()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
