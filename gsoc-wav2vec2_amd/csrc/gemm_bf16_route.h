// Which kernel a bf16 GEMM reaches: a pure function of the problem, host only (no HIP, no pointers, no globals).
// launch_gemm_bf16_x (gemm_bf16.hip) executes the route; w2v2_op_gemm_bf16_route shows it to CPU tests.  Every kernel named here
// rounds the operands the same way and sums an element's K products in the same order, so a route decides time, never bits.  The
// measurements behind the rules: DESIGN.md section 4.1 (route table, constants) and section 8 (what was tried and dropped).
#pragma once

#include <stdint.h>

namespace w2v2 {

enum GemmOperand { GO_ABSENT = 0, GO_PRESENT = 1, GO_ALIGNED = 2 };      // ALIGNED: present and on a 16-byte boundary

struct GemmBf16Problem {
    int M, N, K, nbatch;
    int64_t lda, ldb, strideA, strideB;
    int64_t ldb16;                      // row stride of B16 as the launcher resolved it (GemmShadows::ldb16, 0 -> K)
    int A, B, A16, B16, B16p;           // GemmOperand each: the fp32 operands and their shadows
    bool C, C16;                        // outputs asked for
    // GemmShadows fields that steer (kseg does not: its contract in the launcher allows it on fp32 operands only, where the
    // weight-gradient form has one kernel)
    bool transA;
    int zmod;
    bool colsum, overlapA;
    int64_t validK;
    int kextra;
    bool b_zero_row;
    int force_kernel;
};

enum GemmBf16Kernel {
    GB_NONE = 0,
    GB_F32_GUARDED,         // gemm_bf16_kernel<0, 128, 128, 2, 2, 2>: fp32 operands, scalar guarded loads (any shape)
    GB_F32_VEC,             // <1, ...>: fp32 operands, 16-byte loads
    GB_A_SHADOW,            // <2, ...>: A from its shadow, B fp32
    GB_B_SHADOW,            // <3, ...>: B from its shadow, A fp32
    GB_DMA_128x128,         // <5, 128, 128, 2, 4, 2>: both shadows by LDS-DMA, 8 waves
    GB_DMA_128x64,          // <5, 128, 64, 2, 2, 2>: ... narrow outputs
    GB_AT_F32_128x128,      // <7, 128, 128, 2, 2, 2>: fp32 A transposed in memory (weight gradient)
    GB_AT_F32_128x64,       // <7, 128, 64, 2, 2, 2>
    GB_TR_128x128,          // gemm_bf16_tr_kernel<2, 4, 2>: weight gradient from both shadows, transposing LDS reads
    GB_SW_128x256,          // launch_gemm_bf16_sw: software-pipelined 128 x 256 tiles (gemm_bf16_sw.hip)
    GB_SWTR_128x256,        // launch_gemm_bf16_swtr: its weight-gradient form
    GB_KERNELS              // (one launch counter per value: w2v2_op_gemm_bf16_launches)
};
enum GemmBf16Refusal {
    GBR_NONE = 0,
    GBR_KEXTRA_ON_TR,       // uneven slabs on a shape only the 128 x 128 transposing kernel takes
    GBR_VALIDK,             // validK outside the LDS-DMA weight-gradient form
    GBR_KEXTRA_ZERO_ROW,    // kextra / b_zero_row outside it
    GBR_AT_F32,             // the transposed-fp32 preconditions
    GBR_SHADOW_ONLY,        // an operand given only as a shadow that cannot be streamed
};
inline const char* gemm_bf16_refusal_text(int refusal) {
    switch (refusal) {
        case GBR_KEXTRA_ON_TR: return "gemm_bf16: uneven slabs (kextra) are a feature of the 128 x 256 transposed kernel";
        case GBR_VALIDK: return "gemm_bf16: validK needs the LDS-DMA weight-gradient form (both shadows, whole 128 x 128 tiles)";
        case GBR_KEXTRA_ZERO_ROW: return "gemm_bf16: uneven slabs (kextra) / the zero row behind B need the LDS-DMA weight-gradient form";
        case GBR_AT_F32: return "gemm_bf16: transposed A needs fp32 A and B, K % 64 == 0, M % 4 == 0 and 16-byte alignment";
        case GBR_SHADOW_ONLY: return "gemm_bf16: a shadow-only operand needs K % 64 == 0 and 16-byte alignment";
        default: return "";
    }
}
struct GemmBf16Route {
    int kernel = GB_NONE;
    int refusal = GBR_NONE;             // != 0: no kernel runs this call, the launcher returns gemm_bf16_refusal_text
    int krag = 0;                       // GB_SWTR_128x256: rows that exist in the ragged last K tile (0 = whole)
    int64_t krows = 0;                  // rows of the K dimension over all batches: K nbatch (+ 64 kextra in the weight-gradient forms)
    int a_bytes = 4, b_bytes = 4;       // bytes per element the kernel reads of A and B (what the profiler is charged)
};

constexpr int GEMM_BF16_BK = 64;                            // K tile of every kernel here: one 128-byte LDS row of bf16
constexpr int GEMM_BF16_NARROW_N = 64;                      // N <= 64 (grouped conv: 48 | 64 columns): 128 x 64 tiles waste no half tile
constexpr int GEMM_BF16_SW_MIN_K = 192;                     // the 128 x 256 pipeline has three K tiles in flight
constexpr int64_t GEMM_BF16_SW_MIN_TILES = 256;             // 128 x 256 tiles that fill half of the chip's 512 block slots
constexpr int64_t GEMM_BF16_SW_MIN_WEIGHT = 768 * 768;      // N K of a single-batch GEMM: smaller weights are faster on 128 x 128 ...
constexpr int GEMM_BF16_SW_BATCHED = 2;                     // ... "or a batch": from two batches on (the conv layers) any weight qualifies

// The shape part of "this GEMM streams the bf16 shadow of A": whole 64-wide K tiles, and rows / batch strides that keep every
// 16-byte piece aligned.  The router adds the run-time part (a shadow was passed, its pointer is 16-byte aligned); the forward
// plan asks this before the launch to decide which tensors need no fp32 copy.
inline bool gemm_bf16_streams_a16(int K, int64_t lda, int64_t strideA) { return K % GEMM_BF16_BK == 0 && lda % 8 == 0 && strideA % 8 == 0; }
// 128 x 256 software-pipelined form (gemm_bf16_sw.hip).  Shapes: both operands as aligned bf16 shadows, whole 256-column tiles (B's
// per-lane offsets are shared by its four items), K a multiple of 64 with at least 3 K tiles, any M.
inline bool gemm_bf16_sw_ok(int M, int N, int K, int64_t lda, int64_t ldb16, int64_t strideA) {
    return M >= 1 && N >= 256 && N % 256 == 0 && K % 64 == 0 && K >= GEMM_BF16_SW_MIN_K && lda % 8 == 0 && ldb16 % 8 == 0 && strideA % 8 == 0 &&
           128 * lda < (1 << 29) && 256 * ldb16 < (1 << 29);
}
// Its weight-gradient form: C_z (M, N) = A16_z^T B16_z with A16 (K, M) rows lda apart and B16 (K, N) rows ldb apart, K rows per batch.
inline bool gemm_bf16_swtr_ok(int M, int N, int K, int64_t lda, int64_t ldb, int64_t strideA, int64_t strideB) {
    return M >= 128 && M % 128 == 0 && N >= 256 && N % 256 == 0 && K % 64 == 0 && K >= GEMM_BF16_SW_MIN_K && lda % 8 == 0 && ldb % 8 == 0 &&
           strideA % 8 == 0 && strideB % 8 == 0 && 64 * lda < (1 << 29) && 64 * ldb < (1 << 29);
}

inline GemmBf16Route gemm_bf16_route(const GemmBf16Problem& p) {
    GemmBf16Route r;
    r.krows = (int64_t)p.K * p.nbatch;
    auto run = [&](int kernel, int a_bytes, int b_bytes) { r.kernel = kernel; r.a_bytes = a_bytes; r.b_bytes = b_bytes; return r; };
    auto refuse = [&](int why) { r.refusal = why; return r; };
    const bool kfast = p.K % GEMM_BF16_BK == 0, narrow = p.N <= GEMM_BF16_NARROW_N;
    // an operand can be read 16 bytes at a time: as fp32 (4 elements), as a shadow (8 elements)
    const bool a32 = p.A == GO_ALIGNED && p.lda % 4 == 0 && p.strideA % 4 == 0;
    const bool b32 = p.B == GO_ALIGNED && p.N % 4 == 0 && p.ldb % 4 == 0 && p.strideB % 4 == 0;

    if (p.transA) {      // ---- weight-gradient form  C = A^T B,  A (K, M) and B (K, N) as they lie in memory ----
        // both shadows, whole 128 x 128 tiles, 16-byte aligned rows: LDS-DMA (the fp32 operands are not touched and may be absent)
        if (kfast && p.C && p.A16 == GO_ALIGNED && p.B16p == GO_ALIGNED && !p.colsum && !p.overlapA && p.M % 128 == 0 && p.N % 128 == 0 &&
            p.lda % 8 == 0 && p.ldb % 8 == 0 && p.strideA % 8 == 0 && p.strideB % 8 == 0) {
            r.krows += (int64_t)GEMM_BF16_BK * p.kextra;
            // 128 x 256 tiles where the shape allows them and every row exists, or rows are missing only from the last K tile and the
            // caller promises a zero row behind B (the ragged form); any other ragged row count stays on the transposing-read kernel,
            // which reads rows past validK as zero
            const bool whole = p.validK == 0 || p.validK == r.krows;
            if (!whole && p.b_zero_row && p.validK > r.krows - GEMM_BF16_BK && p.validK < r.krows) r.krag = (int)(p.validK - (r.krows - GEMM_BF16_BK));
            if (p.force_kernel != 1 && (whole || r.krag > 0) && gemm_bf16_swtr_ok(p.M, p.N, p.K, p.lda, p.ldb, p.strideA, p.strideB))
                return run(GB_SWTR_128x256, 2, 2);
            r.krag = 0;
            if (p.kextra != 0) return refuse(GBR_KEXTRA_ON_TR);
            return run(GB_TR_128x128, 2, 2);
        }
        // fp32 operands, A transposed on its way through the registers; contracts exactly K nbatch rows
        if (p.validK != 0) return refuse(GBR_VALIDK);
        if (p.kextra != 0 || p.b_zero_row) return refuse(GBR_KEXTRA_ZERO_ROW);
        if (!(a32 && b32 && kfast && p.M % 4 == 0 && (p.lda >= p.M || p.overlapA))) return refuse(GBR_AT_F32);
        return run(narrow ? GB_AT_F32_128x64 : GB_AT_F32_128x128, 4, 4);
    }

    // ---- forward form  C = A B,  by where the operands can come from ----
    const bool a16 = p.A16 == GO_ALIGNED && gemm_bf16_streams_a16(p.K, p.lda, p.strideA);
    const bool b16 = p.B16 == GO_ALIGNED && kfast && p.strideB == 0 && p.ldb16 % 8 == 0;
    if (a16 && b16) {
        // enough 128 x 256 tiles to fill the chip and a weight large enough (or a batch): the software-pipelined kernel.  force_kernel
        // overrides the size rules, never the shape (1 = never, 2 = whenever the operands allow it); the two-level batch stays here.
        const int64_t tiles = (int64_t)((p.M + 127) / 128) * (p.N / 256) * p.nbatch;
        const bool by_size = tiles >= GEMM_BF16_SW_MIN_TILES && ((int64_t)p.N * p.K >= GEMM_BF16_SW_MIN_WEIGHT || p.nbatch >= GEMM_BF16_SW_BATCHED);
        if (p.zmod == 0 && p.force_kernel != 1 && gemm_bf16_sw_ok(p.M, p.N, p.K, p.lda, p.ldb16, p.strideA) && (p.force_kernel == 2 || by_size))
            return run(GB_SW_128x256, 2, 2);
        return run(narrow ? GB_DMA_128x64 : GB_DMA_128x128, 2, 2);
    }
    if (a16 && b32) return run(GB_A_SHADOW, 2, 4);
    if (b16 && a32) return run(GB_B_SHADOW, 4, 2);
    if (kfast && a32 && b32) return run(GB_F32_VEC, 4, 4);
    if (p.A == GO_ABSENT || p.B == GO_ABSENT) return refuse(GBR_SHADOW_ONLY);
    return run(GB_F32_GUARDED, 4, 4);
}

}  // namespace w2v2
