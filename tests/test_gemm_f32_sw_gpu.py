"""The LDS-ring fp32 GEMM kernels (csrc/gemm_f32_sw.hip) against the double-buffered LDS-DMA kernels they replace: the
same k pairs in the same order, so every output must be bit-identical.  w2v2_op_gemm_variant pins the family for one call:
0 = double buffer, 1 = ring with one tile per block, 2 = ring with a persistent grid.  Every shape below routes to a ring
kernel under variants 1 and 2 (256 x 128 tiles where the launcher picks them, 128 x 128 otherwise)."""

import pytest

from wav2vec2 import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


def run(env, variant, A, lda, strideA, B, C, strideC, bias, res, M, N_, K, nb, act):
    lib, torch, _ = env
    C.fill_(float("nan"))
    N.check(lib.w2v2_op_gemm_variant(N.ptr(A), lda, strideA, N.ptr(B), N_, N.ptr(C), N_, strideC,
                                     N.ptr(bias) if bias is not None else None, N.ptr(res) if res is not None else None,
                                     M, N_, K, nb, act, variant, N.current_stream()))
    torch.cuda.synchronize()
    return C.clone()


def check(env, M, N_, K, act=0, use_bias=False, use_res=False, nb=1, lda=None, strideA=0, seed=0):
    """nb > 1: batched, sample z's A starts strideA elements after sample z - 1's (conv: lda = stride x C_in < K)."""
    _, torch, dev = env
    g = torch.Generator(device=dev).manual_seed(seed)
    lda = lda or K
    a_elems = (nb - 1) * strideA + (M - 1) * lda + K
    A = torch.randn(a_elems, generator=g, device=dev)
    B = torch.randn(K, N_, generator=g, device=dev) * (1.0 / K ** 0.5)
    bias = torch.randn(N_, generator=g, device=dev) if use_bias else None
    res = torch.randn(nb * M * N_, generator=g, device=dev) if use_res else None
    C = torch.empty(nb * M * N_, device=dev)
    ref = run(env, 0, A, lda, strideA, B, C, M * N_, bias, res, M, N_, K, nb, act)
    assert torch.isfinite(ref).all()
    # the reference kernel itself is the fp32 GEMM (spot check of one row block against fp64)
    a0 = torch.as_strided(A, (min(M, 64), K), (lda, 1)).double()
    want = a0 @ B.double() + (bias.double() if bias is not None else 0)
    if act == 0:
        if res is not None:
            want = want + res[: min(M, 64) * N_].view(-1, N_).double()
        assert torch.allclose(ref[: min(M, 64) * N_].view(-1, N_).double(), want, rtol=1e-4, atol=1e-4)
    for variant in (1, 2):
        out = run(env, variant, A, lda, strideA, B, C, M * N_, bias, res, M, N_, K, nb, act)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"variant {variant}: not bit-identical"


# forward shapes of the base model at B = 32 (24576 = 32 x 768 frames)
@pytest.mark.parametrize("M,N_,K,act,use_bias,use_res", [
    (24576, 2304, 768, 0, True, False),     # q|k|v (256 x 128)
    (24576, 3072, 768, 1, True, False),     # FFN up + exact GELU (256 x 128)
    (24576, 768, 3072, 0, True, True),      # FFN down + residual (128 x 128 main rows, 64 x 64 tail rows)
    (24576, 768, 768, 0, True, True),       # out-projection + residual
    (24576, 256, 768, 2, True, False),      # tanh GELU
])
def test_ring_dense_shapes_bit_identical(env, M, N_, K, act, use_bias, use_res):
    check(env, M, N_, K, act, use_bias, use_res)


def test_ring_m_and_n_edges(env):
    check(env, 50001, 516, 256, act=1, use_bias=True, use_res=True, seed=1)      # partial last row tile and column tile


@pytest.mark.parametrize("M,frames_in,nb", [
    (24599, 49199, 2),      # conv1 geometry (kernel 3, stride 2, 512 channels), two samples
    (12299, 24599, 8),      # conv2 geometry, eight samples: enough 256 x 128 tiles for the wide kernel
    (6149, 12299, 3),       # conv3 geometry: padded rows in the last tile of every sample
])
def test_ring_conv_overlapping_rows_batched(env, M, frames_in, nb):
    check(env, M, 512, 3 * 512, nb=nb, lda=2 * 512, strideA=frames_in * 512, seed=2)
