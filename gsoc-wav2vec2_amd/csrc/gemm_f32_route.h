// Which kernel(s) an fp32 GEMM reaches: a pure function of the problem, host only (no HIP, no pointers, no globals).
// launch_gemm_ex (gemm_f32.hip) executes the route; w2v2_op_gemm_f32_route shows it to CPU tests.  Every kernel named here sums
// an element's K products in the same order, so a route decides time, never bits.  The measurements behind the rules: DESIGN.md
// section 4.1 (route table) and section 8 (what was tried and dropped).
#pragma once

#include <stdint.h>

namespace w2v2 {

struct GemmF32Problem {
    int M, N, K, nbatch;
    int64_t lda, ldb, ldc, strideA, strideB;
    int act;                    // 0 none, 1 exact GELU, 2 tanh GELU
    bool has_bias, has_residual;
    bool ab_aligned;            // A and B are 16-byte aligned
    bool c_aligned;             // C, bias and residual are 16-byte aligned (null counts as aligned)
    int ring;                   // -1 by shape; 0 double buffer, 1 ring, 2 persistent ring (w2v2_op_gemm_variant)
};

enum GemmF32Kernel {
    GK_NONE = 0, GK_RING_256x128, GK_RING_128x128, GK_RING_64x64, GK_RING_64x64_QUARTERS,      // gemm_f32_ring_kernel, one launch counter each
    GK_DB_256x128x16, GK_DB_128x128x32, GK_DB_64x64x32,                           // gemm_f32_dma_kernel: LDS-DMA double buffer
    GK_STAGED_128x128,          // gemm_f32_kernel: register-staged, guarded scalar loads (shapes without 16-byte accesses)
};
enum GemmF32RouteKind {
    GR_ONE = 0,                 // kernel[0] over the whole problem
    GR_SPLIT_K,                 // kernel[0] over S slabs of K / S as batches, then the fold
    GR_ORDER_SPLIT,             // kernel[0] over the first main_tiles of the 128 x 128 tile order, kernel[1] the others as quarters
    GR_ROW_SPLIT,               // kernel[0] over the first main_rows rows, kernel[1] over the others
};
struct GemmF32Route {
    int kind = GR_ONE;
    int kernel[2] = {GK_NONE, GK_NONE};
    int S = 0, main_rows = 0;
    int64_t main_tiles = 0;
    bool persist = false;       // the ring kernels of this route run at most two blocks per CU, each looping over its tiles
};

constexpr int GEMM_F32_BK = 32;                         // K step of the double-buffered and staged kernels
constexpr int GEMM_F32_RING_DEFAULT = 2;                // by shape the ring kernels run persistent (59.9 vs 60.5 ms per forward)
constexpr int64_t GEMM_F32_RESIDENT = 512;              // 128 x 128 blocks resident at once: two per CU on 256 CUs
constexpr int64_t GEMM_F32_TAIL_DIV = 4;                // a last round at most a quarter full becomes a tail; half full is better left alone
constexpr int64_t GEMM_F32_SMALL_TILES = 384;           // fewer 128 x 128 tiles leave CUs idle over a long K loop: 64 x 64 tiles instead
constexpr int64_t GEMM_F32_WIDE_TILES = 1536;           // 256 x 128 tiles win only with at least three full rounds of them ...
constexpr int64_t GEMM_F32_WIDE_PAD = 40;               // ... and at most 1 / 40 = 2.5 % padded rows
constexpr int GEMM_F32_SPLITK_MIN_K = 1024;             // split-K (single utterances): a K loop long enough to cut,
constexpr int GEMM_F32_SPLITK_MIN_SLAB = 256;           // slabs of at least 256 k,
constexpr int64_t GEMM_F32_SPLITK_MAX_BLOCKS = 512;     // and no more 64 x 64 blocks than two per CU (so at most 256 tiles, at S = 2)

// the ring kernels' epilogue forms with an instance: plain, bias, bias + exact GELU, bias + residual, residual, exact GELU (the
// bias-free conv layers); -1: none
inline int gemm_f32_ring_form(bool has_bias, bool has_residual, int act) {
    if (act == 1) return has_residual ? -1 : has_bias ? 2 : 5;
    if (act != 0) return -1;
    return has_residual ? (has_bias ? 3 : 4) : (has_bias ? 1 : 0);
}
// a ring kernel (tile 0 = 256 x 128, 1 = 128 x 128, 2 = 64 x 64) can run this shape: 16-byte DMA pieces, and per-lane 32-bit byte
// offsets from the tile's row / column base
inline bool gemm_f32_ring_shape_ok(int tile, bool ab_aligned, int64_t lda, int64_t strideA, int64_t ldb, int64_t strideB, int M, int N, int K) {
    const int BM = tile == 0 ? 256 : tile == 1 ? 128 : 64, BKT = tile == 2 ? 32 : 16;
    const bool align = ab_aligned && lda % 4 == 0 && ldb % 4 == 0 && strideA % 4 == 0 && strideB % 4 == 0;
    return align && K % BKT == 0 && N % 4 == 0 && N >= 4 && (int64_t)BM * lda * 4 < (1ll << 31) && (int64_t)BKT * ldb * 4 < (1ll << 31) && M > 0;
}

inline GemmF32Route gemm_f32_route(const GemmF32Problem& p) {
    // THE ring rule, once: `rows` rows run on the ring kernel of a tile size if the epilogue form has an instance, the override allows
    // it, B is shared by the batches and the shape fits; otherwise on the double buffer of the same tile
    const int pref = gemm_f32_ring_form(p.has_bias, p.has_residual, p.act) < 0 ? 0 : p.ring >= 0 ? p.ring : GEMM_F32_RING_DEFAULT;
    auto ring_takes = [&](int tile, int rows) {
        return pref != 0 && p.strideB == 0 && gemm_f32_ring_shape_ok(tile, p.ab_aligned, p.lda, p.strideA, p.ldb, p.strideB, rows, p.N, p.K);
    };
    auto kernel_of = [&](int tile, int rows) { return (ring_takes(tile, rows) ? GK_RING_256x128 : GK_DB_256x128x16) + tile; };      // (enum order)
    GemmF32Route r;
    auto done = [&](int kind, int k0, int k1 = GK_NONE) {
        r.kind = kind; r.kernel[0] = k0; r.kernel[1] = k1;
        r.persist = pref == 2 && (k0 <= GK_RING_64x64_QUARTERS || (k1 != GK_NONE && k1 <= GK_RING_64x64_QUARTERS));
        return r;
    };
    // shapes without 16-byte global accesses (no GEMM of the models): the register-staged kernel with guarded loads
    const bool fast = p.K % GEMM_F32_BK == 0 && p.N % 4 == 0 && p.lda % 4 == 0 && p.ldb % 4 == 0 && p.strideA % 4 == 0 && p.strideB % 4 == 0 && p.ab_aligned;
    if (!fast) return done(GR_ONE, GK_STAGED_128x128);
    // split-K (serving, B = 1): a handful of tiles each walking a long K loop alone; the most slabs that fit fill the chip, and the fold
    // applies the epilogue the slabs skipped.  The slabs keep the double buffer.
    if (p.nbatch == 1 && p.strideB == 0 && p.K >= GEMM_F32_SPLITK_MIN_K && p.ldc % 4 == 0 && p.c_aligned) {
        const int64_t tiles64 = (int64_t)((p.M + 63) / 64) * ((p.N + 63) / 64);
        for (r.S = 8; r.S >= 2; r.S >>= 1)
            if (p.K % (r.S * GEMM_F32_BK) == 0 && p.K / r.S >= GEMM_F32_SPLITK_MIN_SLAB && tiles64 * r.S <= GEMM_F32_SPLITK_MAX_BLOCKS)
                return done(GR_SPLIT_K, GK_DB_64x64x32);
        r.S = 0;
    }
    // small problems (batch 1-4 of the transformer GEMMs, lm_head, conv rows of a short input): 4 x the blocks at 64 x 64
    const int64_t tn = (p.N + 127) / 128, tiles128 = (int64_t)((p.M + 127) / 128) * tn * p.nbatch;
    if (tiles128 < GEMM_F32_SMALL_TILES) return done(GR_ONE, kernel_of(2, p.M));
    // tail fill: the last, partial round of 128 x 128 tiles would leave most CUs idle for a whole tile time; run it as 64 x 64 tiles
    const int64_t rem = tiles128 % GEMM_F32_RESIDENT;
    if (p.nbatch == 1 && tiles128 > GEMM_F32_RESIDENT && rem != 0 && GEMM_F32_TAIL_DIV * rem <= GEMM_F32_RESIDENT) {
        // no partial tile: the ring kernels cut the tile ORDER (whole rounds, then 4 rem <= 512 quarters: 102 us where whole rows take 142)
        if (p.M % 128 == 0 && p.N % 128 == 0 && ring_takes(1, p.M) && ring_takes(2, p.M)) {
            r.main_tiles = tiles128 - rem;
            return done(GR_ORDER_SPLIT, GK_RING_128x128, GK_RING_64x64_QUARTERS);
        }
        // other shapes, and the double buffer, cut at a tile row
        r.main_rows = (int)((tiles128 - rem) / tn) * 128;
        if (r.main_rows > 0 && r.main_rows < p.M) return done(GR_ROW_SPLIT, kernel_of(1, r.main_rows), kernel_of(2, p.M - r.main_rows));
        r.main_rows = 0;
    }
    // wide tiles for the well-filled shapes: 25 % less LDS-DMA per flop; they lose where their tile count quantises or rows are padded
    const int64_t tm256 = (p.M + 255) / 256, tiles256 = tm256 * (p.N / 128) * p.nbatch;
    if (p.N % 128 == 0 && tiles256 >= GEMM_F32_WIDE_TILES && (tm256 * 256 - p.M) * GEMM_F32_WIDE_PAD <= p.M) return done(GR_ONE, kernel_of(0, p.M));
    // default: 128 x 128, 8 waves, two blocks per CU
    return done(GR_ONE, kernel_of(1, p.M));
}

}  // namespace w2v2
