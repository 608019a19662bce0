"""The exact GELU of the fp32 GEMM epilogue (csrc/gemm_epilogue.h, csrc/common.h: gelu_erf_epi) and the ring kernels' compile-time
epilogue forms (csrc/gemm_f32_sw.hip).

1. The function: gelu_erf_epi against 0.5 x (1 + erff(x / sqrt 2)) with the library erff over all 2^32 float patterns.
2. The kernels: every ring instance and its edge path with bias + GELU or bias + residual, against a reference that does not run the
   new code: the act = 0 GEMM followed by an element-wise kernel that calls the library erff (w2v2_op_gelu_reference), or by torch's
   fp32 add of the residual.  Which instance a call reached is read from the launch counters (w2v2_op_gemm_ring_launches).
3. Host only: no ring instance spills or uses scratch."""

import ctypes as C
import os

import pytest

from wav2vec2 import _native as N


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


def ring_launches(lib):
    c = (C.c_int64 * 4)()
    N.check(lib.w2v2_op_gemm_ring_launches(c))
    return list(c)


def gemm(env, variant, A, lda, strideA, B, bias, res, M, N_, K, nb, act):
    lib, torch, dev = env
    out = torch.full((nb * M * N_,), float("nan"), device=dev)
    N.check(lib.w2v2_op_gemm_variant(N.ptr(A), lda, strideA, N.ptr(B), N_, N.ptr(out), N_, M * N_, N.ptr(bias), N.ptr(res),
                                     M, N_, K, nb, act, variant, N.current_stream()))
    torch.cuda.synchronize()
    return out


def check(env, M, N_, K, form, route, nb=1, lda=None, strideA=0, seed=0, use_bias=True):
    """form: "gelu" (bias + exact GELU; use_bias=False: the conv layers' bias-free form) or "res" (bias + residual).  route: launches per ring instance (256 x 128, 128 x 128, 64 x 64,
    64 x 64 quarters) that variants 1 and 2 must add; variant 0 (the double buffer) adds none."""
    lib, torch, dev = env
    g = torch.Generator(device=dev).manual_seed(seed)
    lda = lda or K
    n_a = (nb - 1) * strideA + (M - 1) * lda + K
    A = torch.randn(n_a, generator=g, device=dev)
    # a third of the rows x 0.3, a third x 2, a third x 8: outputs on both erf arms and in the saturated range
    third = (n_a + 2) // 3
    A[:third] *= 0.3
    A[third:2 * third] *= 2.0
    A[2 * third:] *= 8.0
    B = torch.randn(K, N_, generator=g, device=dev) * (1.0 / K ** 0.5)
    bias = torch.randn(N_, generator=g, device=dev) if use_bias else None
    lin = gemm(env, 0, A, lda, strideA, B, bias, None, M, N_, K, nb, 0)
    assert torch.isfinite(lin).all()
    if form == "gelu":
        assert (lin.abs() < 0.7).any() and ((lin.abs() > 2.0) & (lin.abs() < 5.0)).any() and (lin.abs() > 8.0).any()
        ref = torch.empty_like(lin)
        N.check(lib.w2v2_op_gelu_reference(N.ptr(lin), N.ptr(ref), lin.numel(), N.current_stream()))
        res, act = None, 1
    else:
        res = torch.randn(nb * M * N_, generator=g, device=dev)
        ref = lin + res
        act = 0
    torch.cuda.synchronize()
    for variant in (0, 1, 2):
        before = ring_launches(lib)
        out = gemm(env, variant, A, lda, strideA, B, bias, res, M, N_, K, nb, act)
        added = [b - a for a, b in zip(before, ring_launches(lib))]
        assert added == (list(route) if variant else [0, 0, 0, 0]), f"variant {variant}: ring launches {added}"
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"variant {variant}: differs from the reference"


@pytest.mark.gpu
def test_epilogue_gelu_is_the_library_gelu_on_every_float(env):
    """gelu_erf_epi (and gelu_erf_select) return gelu_erf's bits, library erff inside, for every one of the 2^32 float patterns."""
    lib, torch, dev = env
    mm = torch.full((2,), -1, dtype=torch.int64, device=dev)
    N.check(lib.w2v2_op_check_gelu_epilogue(N.ptr(mm), N.current_stream()))
    torch.cuda.synchronize()
    assert mm.tolist() == [0, 0]


@pytest.mark.gpu
def test_wide_ring_gelu_ragged_last_row_tile(env):
    """256 x 128: 12 x 128 = 1536 tiles, 40 padded rows of 3072 (<= 2.5 %)."""
    check(env, 3032, 16384, 32, "gelu", (1, 0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("K,route", [(96, (0, 1, 0, 0)), (48, (0, 0, 0, 0))])
def test_128_ring_gelu_ragged_m_and_n(env, K, route):
    """128 x 128: 24 x 16 = 384 tiles, partial last row and column tile.  K = 96 is six K tiles of 16: the fifth wraps the 4-stage ring.
    K = 48 is no multiple of the launcher's 32-wide K step, so no ring kernel takes it (the counters say so): the register-staged
    128 x 128 kernel runs the same shared epilogue on the same ragged tiles."""
    check(env, 3050, 2044, K, "gelu", route, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["res", "gelu"])
def test_split_route_main_and_quarter_launches(env, form):
    """576 tiles of 128 x 128 = 512 at 128 x 128 + 64 as 256 quarters of 64 x 64."""
    check(env, 12288, 768, 32, form, (0, 1, 0, 1), seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gelu", "res"])
def test_64_ring(env, form):
    check(env, 200, 192, 64, form, (0, 0, 1, 0), seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("use_bias", [True, False])
def test_64_ring_batched_overlapping_rows_gelu(env, use_bias):
    """conv-like: three samples, rows 64 elements apart read 96 (overlap), samples 1401 x 32 elements apart; with a bias, and without
    one as the base model's conv layers run it."""
    check(env, 700, 512, 96, "gelu", (0, 0, 1, 0), nb=3, lda=64, strideA=1401 * 32, seed=4, use_bias=use_bias)


def test_ring_kernels_have_no_scratch_and_no_spills():
    """Build gate, no GPU needed: with the epilogue form a template argument every gemm_f32_ring_kernel instance (the 256 x 128 one used
    to spill two VGPRs) reports ScratchSize 0 and no spilled registers.  The kernels' counted vmcnt waits rest on that."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "gsoc-wav2vec2_amd", "csrc", "gemm_f32_sw.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = [], None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            cur = {"name": line.split("Function Name:")[1].split("[")[0].strip()}
            kernels.append(cur)
        elif cur is not None:
            for key in ("ScratchSize [bytes/lane]:", "VGPRs Spill:", "SGPRs Spill:"):
                if key in line:
                    cur[key] = int(line.split(key)[1].split("[")[0].strip())
    ring = [k for k in kernels if "gemm_f32_ring_kernel" in k["name"]]
    assert len(ring) == 24, [k["name"] for k in kernels]      # 4 instances x 6 epilogue forms
    bad = [k for k in ring if k.get("ScratchSize [bytes/lane]:") != 0 or k.get("VGPRs Spill:") != 0 or k.get("SGPRs Spill:") != 0]
    assert not bad, bad
