"""The 64 x 64 LDS-ring fp32 GEMM instance (csrc/gemm_f32_sw.hip) against the double-buffered 64 x 64 kernel it replaces on the
tail of a partly filled last round of 128 x 128 tiles, on the small problems (fewer than 384 tiles of 128 x 128) and on
their batched form.  Same k pairs in the same order, so every output must be bit-identical.  w2v2_op_gemm_variant pins the
family for one call: 0 = double buffer everywhere, 1 = ring with one tile per block, 2 = ring with a persistent grid.

The instance is BKT x NS = 32 x 3: K tiles of 32 through three ring stages.  The launcher takes the LDS-DMA kernels only for
K % 32 == 0, so K = 32 j is j K tiles, and j = 1 .. NS + 1 covers fewer K tiles than ring stages, exactly NS - 1, NS, and one
wrap of the ring.

The tail comes in two forms.  M or N not a multiple of 128: whole tile rows past the last full round go to the 64 x 64 kernel
(variant 0 does the same with the double-buffered kernels).  Both multiples of 128: variants 1 and 2 split the tile ORDER, the
first whole rounds at 128 x 128 and every later tile as four 64 x 64 quarters."""

import pytest

from wav2vec2 import _native as N

pytestmark = pytest.mark.gpu

BKT, NS = 32, 3
K_EDGES = [BKT * j for j in range(1, NS + 2)]


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


# fewer than 384 tiles of 128 x 128: one partial tile, one row / column short of a tile, one past it, several tiles
@pytest.mark.parametrize("K", K_EDGES)
@pytest.mark.parametrize("M,N_", [(1, 4), (63, 60), (65, 68), (200, 132)])
def test_small_problem_route_bit_identical(env, M, N_, K):
    for i, (act, use_bias, use_res) in enumerate([(0, False, False), (0, True, True), (1, True, False), (2, False, True), (2, True, True)]):
        check(env, M, N_, K, act, use_bias, use_res, seed=10 + i)


def test_long_k(env):
    """Three tiles of 64 x 64 at K = 3072: the launcher splits K eight ways for every variant (split-K keeps the double-buffered
    kernel for its slabs), so this case pins that route's result, not the ring."""
    check(env, 130, 64, 3072, use_bias=True, use_res=True, seed=3)


def test_long_k_on_the_ring(env):
    """K = 3072 on the small-problem route itself: 18 x 16 = 288 tiles of 64 x 64 are too many for split-K (more than 256) and
    9 x 8 = 72 tiles of 128 x 128 are fewer than 384; 96 K tiles wrap the three-stage ring 32 times.  And a batched pair, which
    split-K never takes."""
    check(env, 1100, 1024, 3072, act=1, use_bias=True, use_res=True, seed=7)
    check(env, 130, 64, 3072, use_bias=True, use_res=True, nb=2, strideA=130 * 3072, seed=8)


# 88 x 6 = 528 tiles of 128 x 128 = 512 + 16: the main rows are 10880 (85 row tiles), the tail 293 rows, its last 64-row tile partial
@pytest.mark.parametrize("K", [96, 3072])
def test_tail_route_bit_identical(env, K):
    check(env, 11173, 768, K, act=0, use_bias=True, use_res=True, seed=4)


def test_batched_overlapping_rows(env):
    """The conv1 remainder geometry (kernel 3, stride 2, 512 channels) with a short input: 23 rows per sample, three samples."""
    check(env, 23, 512, 3 * 512, nb=3, lda=2 * 512, strideA=47 * 512, seed=5)


# 88 x 6 = 528 tiles again, none partial: variants 1 and 2 cut the grouped tile order after 512 tiles (a cut inside a group of tile
# rows: the 16 last tiles are not whole rows) and run 64 quarter tiles; K below and above the ring depth
@pytest.mark.parametrize("K", [64, 512])
def test_tail_split_of_the_tile_order_bit_identical(env, K):
    check(env, 11264, 768, K, act=1, use_bias=True, use_res=True, seed=6)
