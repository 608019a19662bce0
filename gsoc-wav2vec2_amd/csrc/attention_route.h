// Which attention kernel a problem reaches: a pure function of the problem, host only (no HIP, no pointers, no globals).
// launch_attention_routed / _train_routed / _bwd_routed (attention.hip) execute the route; the forward plan, the training plan, the
// packed stream's tile table and the packed ops ask it instead of restating its conditions; w2v2_op_attention_route shows it to CPU
// tests.  Unlike a GEMM route this one decides bits as well as time: the three families round differently (DESIGN.md section 4.2,
// route table; section 8, what was tried and dropped).
#pragma once

namespace w2v2 {

enum AttnPass { AP_INFER = 0, AP_TRAIN = 1, AP_BWD = 2 };      // inference forward, training forward (dropout, lse saved), backward

struct AttnProblem {
    int pass;                   // AttnPass
    int precision;              // W2V2_PRECISION_*: 0 fp32, 1 bf16, 2 bf16x3, 3 f16x2
    int B, T, H, heads;         // packed: B = 1 and T = the stream's frames (neither steers a packed route)
    bool packed;                // inference only: one block of queries per entry of a tile table, keys of the tile's utterance
    bool split_allowed;         // W2V2_SPLIT_ATTN, read by the caller (attention_split_allowed)
    bool io_aligned;            // qkv and ctx on 16-byte boundaries (a plan, which has no pointers yet, passes true)
    // the forms of the output the caller wants (backward: of dqkv): a form the family cannot write is a refusal
    bool want_f32, want_b16, want_planes;
};

enum AttnFamily { AF_NONE = 0, AF_F32, AF_SPLIT, AF_BF16 };
enum AttnKernel {
    AK_NONE = 0,
    AK_F32_D32_W4, AK_F32_D32_W8, AK_F32_D32_W12,       // attention_kernel<DH, NW>: fp32 inference, dense
    AK_F32_D64_W4, AK_F32_D64_W8, AK_F32_D64_W12,
    AK_F32_D128_W4, AK_F32_D128_W8,
    AK_F32_PACKED_D32, AK_F32_PACKED_D64, AK_F32_PACKED_D128,       // attention_kernel<DH, 8, false, true>
    AK_F32_TRAIN_D32_W4, AK_F32_TRAIN_D64_W4, AK_F32_TRAIN_D64_W12, // attention_kernel<DH, NW, true>
    AK_F32_BWD_D32, AK_F32_BWD_D64,                     // attn_dvec_kernel, attention_bwd_dq_kernel, attention_bwd_dkv_kernel <DH>
    AK_SPLIT_BF16X3, AK_SPLIT_F16X2,                    // attention_split_kernel<FMT>
    AK_SPLIT_PACKED_BF16X3, AK_SPLIT_PACKED_F16X2,      // attention_split_kernel<FMT, true>
    AK_BF16, AK_BF16_PACKED, AK_BF16_TRAIN,             // attention_bf16_pipe_kernel<TRAIN, DROP, SEG>
    AK_BF16_BWD,                                        // attention_bf16_bwd_dq_kernel, attention_bf16_bwd_dkv_kernel <BITS>
    AK_KERNELS                                          // (one launch counter per value: w2v2_op_attention_launches)
};
enum AttnRefusal {
    ATR_NONE = 0,
    ATR_HEAD_SIZE,          // no kernel of the pass has this head size
    ATR_SHADOW,             // a bf16 shadow output wanted from a family other than bf16
    ATR_PLANES,             // a plane output wanted from a family other than split
};

struct AttnRoute {
    AttnProblem p;                      // the problem this route answers (the launchers take their sizes from it)
    int kernel = AK_NONE;
    int refusal = ATR_NONE;             // != 0: no kernel runs, the launcher returns attention_refusal_text
    int family = AF_NONE;
    int fmt = -1;                       // split family: the plane format, 0 = three bf16 terms (PF_BF16X3), 1 = two fp16 terms (PF_F16X2)
    int dh = 0;                         // head size
    int waves = 0, rows = 0;            // waves per block; queries per block = 32 waves = the height of a packed tile
    bool lse_log2 = false;              // training: the saved lse is -(m C2 + log2 l), not the natural one
    bool writes_b16 = false, writes_planes = false;       // what the family can write besides fp32
};

constexpr int ATTN_WAVE_ROWS = 32;                  // queries (backward, dK / dV: keys) a wave owns, every kernel
constexpr int ATTN_CUS = 256;                       // the cost model's chip
constexpr int ATTN_F32_PACKED_WAVES = 8;            // the tile table is built before the launch: one height for every stream
constexpr int ATTN_F32_BWD_WAVES = 4;
constexpr int ATTN_F32_TRAIN_LONG_T = 384;          // from here on a head-size-64 training forward fills whole 12-wave blocks
constexpr int ATTN_SPLIT_WAVES = 8;
constexpr int ATTN_BF16_WAVES = 4;
constexpr int ATTN_BF16_DH = 64, ATTN_SPLIT_DH = 64;
constexpr int ATTN_MIN_PACKED_ROWS = ATTN_BF16_WAVES * ATTN_WAVE_ROWS;      // the lowest packed tile of any route: sizes tile tables

// The message of a refusal, as the launcher of the pass worded it before there was a route (a head size goes into its %d).
inline const char* attention_refusal_text(const AttnRoute& r) {
    const int pass = r.p.pass;
    switch (r.refusal) {
        case ATR_HEAD_SIZE:
            return pass == AP_BWD     ? "attention_bwd: head size %d unsupported (32, 64)"
                   : pass == AP_TRAIN ? "attention_train: head size %d unsupported (32, 64)"
                   : r.p.packed       ? "attention_packed: head size %d unsupported (32, 64, 128)"
                                      : "attention: head size %d unsupported (32, 64, 128)";
        case ATR_SHADOW:
            return pass == AP_BWD     ? "attention_bwd: a bf16 shadow of dqkv is only written by the bf16 kernels (head size 64, precision mode 1)"
                   : pass == AP_TRAIN ? "attention_train: a bf16 shadow output needs the bf16 kernel (precision 1, head size 64)"
                                      : "attention: a bf16 shadow output needs the bf16 kernel (precision 1, head size 64)";
        case ATR_PLANES: return "attention: a plane output needs the split kernel (precision modes 2 / 3, head size 64)";
        default: return "";
    }
}

// fp32 inference, dense: the waves per block that fill the CUs in the fewest rounds.  Waves stay a multiple of 4 (one per SIMD).
// Measured at T = 768, B = 32, 12 heads: 4 waves (2 blocks per CU) 95 TF, 8 waves 93, 12 waves (3 per SIMD) 105.
inline int attention_f32_waves(int dh, int B, int T, int heads) {
    const int cand[3] = {12, 8, 4};
    int best = 4;
    long long best_cost = -1;
    for (int i = 0; i < 3; ++i) {
        const int nw = cand[i];
        if (dh == 128 && nw == 12) continue;                  // 241 VGPRs: 3 waves per SIMD would spill
        const int bpc = (dh != 128 && nw == 4) ? 2 : 1;       // blocks per CU the VGPR / LDS budget admits
        const long long nblk = (long long)((T + nw * ATTN_WAVE_ROWS - 1) / (nw * ATTN_WAVE_ROWS)) * heads * B;
        const long long rounds = (nblk + ATTN_CUS * bpc - 1) / (ATTN_CUS * bpc);
        const long long cost = rounds * nw * bpc * (nw == 12 ? 9 : 10);   // 3 waves per SIMD run ~10 % better
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = nw; }
    }
    return best;
}

inline AttnRoute attention_route(const AttnProblem& p) {
    AttnRoute r;
    r.p = p;
    r.dh = p.heads > 0 ? p.H / p.heads : 0;
    const int dh = r.dh;
    const bool packed = p.pass == AP_INFER && p.packed;
    auto run = [&](int family, int kernel, int waves) {
        r.family = family; r.kernel = kernel; r.waves = waves; r.rows = waves * ATTN_WAVE_ROWS;
        return r;
    };
    auto refuse = [&](int why) { r.refusal = why; return r; };

    // precision mode 1, head size 64: the bf16 matrix pipe, every pass.  Whatever the caller holds of q | k | v: the kernel reads the
    // bf16 shadow and makes one from the fp32 tensor where none came.
    if (p.precision == 1 && dh == ATTN_BF16_DH) {
        r.writes_b16 = true;
        r.lse_log2 = p.pass != AP_INFER;
        if (p.want_planes) return refuse(ATR_PLANES);
        return run(AF_BF16, p.pass == AP_BWD ? AK_BF16_BWD : p.pass == AP_TRAIN ? AK_BF16_TRAIN : packed ? AK_BF16_PACKED : AK_BF16, ATTN_BF16_WAVES);
    }
    if (p.want_b16) return refuse(ATR_SHADOW);
    // precision modes 2 / 3, head size 64, inference: fp32-grade results from the bf16 / fp16 matrix pipe, 16-byte accesses throughout
    if (p.pass == AP_INFER && p.precision >= 2 && p.split_allowed && dh == ATTN_SPLIT_DH && p.H % 4 == 0 && p.io_aligned) {
        r.writes_planes = true;
        r.fmt = p.precision == 3 ? 1 : 0;
        return run(AF_SPLIT, (packed ? AK_SPLIT_PACKED_BF16X3 : AK_SPLIT_BF16X3) + r.fmt, ATTN_SPLIT_WAVES);
    }
    if (p.want_planes) return refuse(ATR_PLANES);
    // fp32 on the fp32 matrix pipe
    const int d = dh == 32 ? 0 : dh == 64 ? 1 : (dh == 128 && p.pass == AP_INFER) ? 2 : -1;
    if (d < 0) return refuse(ATR_HEAD_SIZE);
    if (p.pass == AP_BWD) return run(AF_F32, AK_F32_BWD_D32 + d, ATTN_F32_BWD_WAVES);
    if (p.pass == AP_TRAIN) {      // 12 waves per block (3 per SIMD) when the sequence is long enough to fill whole blocks
        const bool w12 = dh == 64 && p.T >= ATTN_F32_TRAIN_LONG_T;
        return run(AF_F32, d == 0 ? AK_F32_TRAIN_D32_W4 : w12 ? AK_F32_TRAIN_D64_W12 : AK_F32_TRAIN_D64_W4, w12 ? 12 : 4);
    }
    if (packed) return run(AF_F32, AK_F32_PACKED_D32 + d, ATTN_F32_PACKED_WAVES);
    const int nw = attention_f32_waves(dh, p.B, p.T, p.heads);
    return run(AF_F32, (d == 0 ? AK_F32_D32_W4 : d == 1 ? AK_F32_D64_W4 : AK_F32_D128_W4) + (nw == 12 ? 2 : nw == 8 ? 1 : 0), nw);
}

}  // namespace w2v2
