// How a weight gradient dW (Kin, Nout) = A^T dY over M = B T rows is cut into split-K slabs, which kernels contract them, where the
// result goes and how the bias gradient is made: a pure function of the problem, host only (no HIP, no pointers, no globals).
// launch_weight_grad (w2v2_train.hip) executes a plan; w2v2_op_weight_grad_plan shows it to CPU tests; the scratch sizes of the training
// step (wg_max_slabs, WG_MAX_SLABS) come from the same constants.  Every form sums fp32 slabs in slab order, so a plan decides time and
// launches, and which bits only through the cut.  The measurements behind the constants: DESIGN.md section 5.2 (plan table) and
// section 8 (what was tried).
#pragma once

#include <stdint.h>

#include "gemm_bf16_route.h"

namespace w2v2 {

struct WgProblem {
    int M, Kin, Nout;                   // rows contracted (B T), dW is (Kin, Nout)
    int precision;                      // the calling thread's mode (gemm_get_precision), as the caller read it
    bool A, dY, A16, dY16;              // operands present: fp32 A (M, Kin) / dY (M, Nout) and their bf16 shadows
    bool dy16_zero_row;                 // the caller keeps row M of dY16 all-zero
    bool want_dW, want_db;
    bool unpack;                        // the fold scatters the packed q|k|v matrix: even one slab goes through it
    int64_t shared_slab_floats;         // the training step's shared slab scratch: the slab count follows it whichever scratch is used
    int64_t site_slab_floats;           // the site's own slab scratch, 0 = none (the shared one is in use)
    int64_t cs_floats;                  // scratch for the per-slab column sums of dY
    int dw_blocks, dw_uneven;           // W2V2_DW_BLOCKS, W2V2_DW_UNEVEN as the caller read them (weight_grad_knobs)
};

enum WgForm {
    WG_BIAS_ONLY = 0,       // no dW wanted
    WG_UNEVEN_128x256,      // both shadows on the 128 x 256 transposed kernel: any slab count, the first kextra slabs one K tile longer
    WG_RAGGED_128x128,      // both shadows on the transposing-read kernel: rows past validK read as zero, the last slab merely short
    WG_DIV_SHADOWS,         // divisor rule, both shadows; leftover rows on launch_dw_tail_bf16
    WG_DIV_F32_REG,         // divisor rule, fp32 operands transposed in registers by the bf16 kernel; leftover rows through a transposed copy
    WG_DIV_F32_COPY,        // divisor rule, a transposed copy of A and the fp32 GEMM for slabs and leftover rows
    WG_FORMS
};
enum WgTail { WG_TAIL_NONE = 0, WG_TAIL_SHADOW, WG_TAIL_COPY };
enum WgDst { WG_TO_NONE = 0, WG_TO_DW, WG_TO_SLABS };
enum WgBias { WG_BIAS_NONE = 0, WG_BIAS_FUSED, WG_BIAS_PASS };      // FUSED: column sums ride in the GEMM; PASS: a column-sum pass over fp32 dY
enum WgRefusal { WGR_NONE = 0, WGR_FP32_OPERANDS, WGR_SLAB_SCRATCH, WGR_BIAS_NEEDS_DY };
inline const char* weight_grad_refusal_text(int refusal) {
    switch (refusal) {
        case WGR_FP32_OPERANDS: return "weight_grad: the fp32 operands are needed here (no bf16 shadows / shapes not whole 128-tiles)";
        case WGR_SLAB_SCRATCH: return "weight_grad: slab scratch too small";
        case WGR_BIAS_NEEDS_DY: return "weight_grad: the bias gradient needs the fp32 dY";
        default: return "";
    }
}

struct WgPlan {
    int refusal = WGR_NONE;             // != 0: nothing is launched, the executor returns weight_grad_refusal_text
    int form = WG_BIAS_ONLY;
    int kernel = GB_NONE;               // GemmBf16Kernel of the slab GEMM (GB_NONE: the fp32 GEMM, or no slab GEMM at all)
    int kq = 0;                         // K granularity of the slab kernel
    int cap = 0;                        // most slabs the block slots and the scratch allow
    int S = 0, Kp = 0;                  // S slabs of Kp rows on the slab kernel (S = 0: fewer than kq rows)
    int kextra = 0;                     // GemmShadows::kextra
    int64_t validK = 0;                 // GemmShadows::validK
    bool b_zero_row = false;            // GemmShadows::b_zero_row
    int Mq = 0, R = 0;                  // rows [0, Mq) on the slab kernel, leftover rows [Mq, M) on the tail
    int tail = WG_TAIL_NONE;
    int nslabs = 0;                     // S + (R ? 1 : 0)
    int dst = WG_TO_NONE;               // where the GEMMs write
    bool fold = false;                  // a fold sums nslabs slabs into dW (or the three unpacked kernels)
    int bias = WG_BIAS_NONE;
};

constexpr int WG_KQ_BF16 = 64, WG_KQ_F32 = 32;      // K tile of the bf16 kernels / of the fp32 one: slabs are whole multiples
constexpr int WG_BLOCKS_BF16 = 512;                 // tiles x slabs: one block per resident slot for the bf16 kernels (W2V2_DW_BLOCKS) ...
constexpr int WG_BLOCKS_F32 = 2048;                 // ... about four for the fp32 one, to balance its long tiles
constexpr int WG_MAX_S = 32;                        // each slab costs a fold pass
constexpr int WG_MAX_SLABS = WG_MAX_S + 1;          // ... plus the leftover-row slab: what the shared scratch holds of the widest kernel
constexpr int WG_GIVE_AWAY = 16;                    // divisor rule: up to 15 units go to the leftover slab for a better divisor
constexpr int WG_UNEVEN_MIN_TILES = 3;              // K tiles per slab of the 128 x 256 kernel: its pipeline depth (GEMM_BF16_SW_MIN_K)
constexpr int WG_TILE = 128;
static_assert(WG_UNEVEN_MIN_TILES * WG_KQ_BF16 == GEMM_BF16_SW_MIN_K && WG_KQ_BF16 == GEMM_BF16_BK, "the uneven form feeds the 128 x 256 kernel");

// Slabs a site's own scratch is sized for (+ 1 for the fold's partial scratch behind them): no plan of a (Kin, Nout) gradient has
// more.  tiles >= Kin Nout / 128^2 and tiles S <= WG_BLOCKS_F32 (the larger of the two block limits; wide tiles count double against
// the smaller one), S <= WG_MAX_S, plus the leftover-row slab.
inline int64_t wg_max_slabs(int64_t Kin, int64_t Nout) {
    const int64_t elems = Kin * Nout, s = ((int64_t)WG_BLOCKS_F32 * WG_TILE * WG_TILE + elems - 1) / elems;
    return (s < WG_MAX_S ? s : WG_MAX_S) + 1;
}

// `rows` rows as S slabs on the 128 x 256 kernel: every slab Kp rows, the first kextra one K tile more, the last K tile short when
// validK != 0 (which needs the zero row behind dY16).  w2v2_op_weight_grad_bf16 checks its arguments against this.
struct WgUneven {
    int Kp, kextra;
    int64_t validK;
};
inline WgUneven wg_uneven_slabs(int64_t rows, int S) {
    const int64_t units_all = (rows + WG_KQ_BF16 - 1) / WG_KQ_BF16;
    return WgUneven{(int)(units_all / S * WG_KQ_BF16), (int)(units_all % S), rows % WG_KQ_BF16 ? rows : 0};
}

inline WgPlan weight_grad_plan(const WgProblem& q) {
    WgPlan p;
    auto refuse = [&](int why) { p.refusal = why; return p; };
    const int M = q.M, Kin = q.Kin, Nout = q.Nout;
    const int64_t elems = (int64_t)Kin * Nout;
    // ---- the bias gradient, unless the divisor form below lets it ride along: a column-sum pass over the fp32 dY
    auto finish = [&]() {
        if (q.want_db && p.bias != WG_BIAS_FUSED) {
            if (!q.dY) return refuse(WGR_BIAS_NEEDS_DY);
            p.bias = WG_BIAS_PASS;
        }
        return p;
    };
    if (!q.want_dW) return finish();
    // ---- the kernel family.  Mode bf16 stages A^T from A directly (the bf16 GEMM's B path transposes in registers anyway); fp32
    // goes through a transposed copy.  Both shadows and whole 128 x 128 tiles: the transposing-read kernels, which touch no fp32 operand
    const bool direct = q.precision == 1 && Kin % 4 == 0 && Nout % 4 == 0;
    const bool tr_form = direct && q.A16 && q.dY16 && Kin % WG_TILE == 0 && Nout % WG_TILE == 0;
    const int kq = p.kq = direct ? WG_KQ_BF16 : WG_KQ_F32;
    // ... whole rows (or a short last K tile made up from the zero row) and whole 256-column tiles: 128 x 256 tiles, half as many
    const bool wide_tiles = tr_form && Nout % 256 == 0 && (M % kq == 0 || (q.dy16_zero_row && M > kq));
    // ---- most slabs worth having: tiles x slabs within the block limit, and cap + 2 slabs within the shared scratch (whichever scratch
    // is in use, so that S does not depend on the site); a site's own scratch is sized by wg_max_slabs and holds them all
    const int64_t tiles = (int64_t)((Kin + WG_TILE - 1) / WG_TILE) * (wide_tiles ? Nout / 256 : (Nout + WG_TILE - 1) / WG_TILE);
    const int64_t max_blocks = direct ? q.dw_blocks : WG_BLOCKS_F32;
    int cap = WG_MAX_S;
    while (cap > 1 && (tiles * cap > max_blocks || (int64_t)(cap + 2) * elems > q.shared_slab_floats)) --cap;
    while (cap > 1 && q.site_slab_floats > 0 && (int64_t)(cap + 1) * elems > q.site_slab_floats) --cap;
    p.cap = cap;
    if (!tr_form && !(q.A && q.dY)) return refuse(WGR_FP32_OPERANDS);
    const int64_t units_all = ((int64_t)M + kq - 1) / kq;      // (the last unit may be short)

    // ---- 1. uneven slabs on the 128 x 256 kernel: ANY slab count works there, so take as many as the block slots hold
    const int S_uneven = (int)(cap < units_all / WG_UNEVEN_MIN_TILES ? cap : units_all / WG_UNEVEN_MIN_TILES);
    if (wide_tiles && q.dw_uneven != 0 && S_uneven >= 1) {
        const WgUneven u = wg_uneven_slabs(M, S_uneven);
        p.form = WG_UNEVEN_128x256; p.kernel = GB_SWTR_128x256;
        p.S = S_uneven; p.Kp = u.Kp; p.kextra = u.kextra; p.validK = u.validK; p.b_zero_row = u.validK != 0;
        p.Mq = M;
    }
    // ---- 2. a ragged row count on the transposing-read kernel: S slabs of ceil(units / S) K tiles, none empty, the last one short
    else if (tr_form && M % kq != 0) {
        int S = (int)(units_all < cap ? units_all : cap);
        int64_t per = (units_all + S - 1) / S;
        while (S > 1 && (int64_t)(S - 1) * per >= units_all) { --S; per = (units_all + S - 1) / S; }
        p.form = WG_RAGGED_128x128; p.kernel = GB_TR_128x128;
        p.S = S; p.Kp = (int)(per * kq); p.validK = M;
        p.Mq = M;
    }
    // ---- 3. the divisor rule: S equal slabs of whole units, S the largest divisor <= cap of the unit count; a unit count without a
    // useful divisor (a prime, say) gives up to 15 units to the leftover slab until one appears
    else {
        const int64_t units0 = M / kq;
        int64_t units = units0;
        int S = units0 > 0 ? 1 : 0;
        for (int drop = 0; drop < WG_GIVE_AWAY && units0 - drop > 0; ++drop) {
            const int64_t u = units0 - drop;
            int d = 1;
            for (int cand = cap; cand >= 2; --cand)
                if (u % cand == 0) { d = cand; break; }
            if (d > S) { S = d; units = u; }
            if (2 * d >= cap) break;      // good enough: stop giving rows away
        }
        p.S = S; p.Mq = (int)(units * kq); p.R = M - p.Mq;
        p.Kp = S ? p.Mq / S : 0;
        p.form = tr_form ? WG_DIV_SHADOWS : direct ? WG_DIV_F32_REG : WG_DIV_F32_COPY;
        if (S && tr_form)
            p.kernel = gemm_bf16_swtr_ok(Kin, Nout, p.Kp, Kin, Nout, (int64_t)p.Kp * Kin, (int64_t)p.Kp * Nout) ? GB_SWTR_128x256 : GB_TR_128x128;
        else if (S && direct)
            p.kernel = Nout <= GEMM_BF16_NARROW_N ? GB_AT_F32_128x64 : GB_AT_F32_128x128;
        if (p.R) p.tail = tr_form ? WG_TAIL_SHADOW : WG_TAIL_COPY;
    }
    p.nslabs = p.S + (p.R ? 1 : 0);
    // ---- where the GEMMs write: one slab goes straight to dW, more (or the unpacking fold) through the slabs and a fold, whose
    // one-chunk partial scratch lives behind them
    p.fold = p.nslabs > 1 || q.unpack;
    p.dst = p.fold ? WG_TO_SLABS : WG_TO_DW;
    if (p.fold && (int64_t)(p.nslabs + 1) * elems > (q.site_slab_floats > 0 ? q.site_slab_floats : q.shared_slab_floats)) return refuse(WGR_SLAB_SCRATCH);
    // ---- the fp32 operands in registers: the kernel's row-tile-0 blocks sum the dY columns they stage anyway, one row per slab (the
    // leftover rows add one), then one small fold.  The shadow kernels have no fp32 dY in registers (db sums the UNROUNDED dY)
    if (p.form == WG_DIV_F32_REG && p.S && q.want_db && (int64_t)(p.nslabs + 1) * Nout <= q.cs_floats) p.bias = WG_BIAS_FUSED;
    return finish();
}

}  // namespace w2v2
