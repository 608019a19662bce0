// Shared host/device helpers for the gfx950 Wav2Vec2 path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <initializer_list>
#include <type_traits>

#include <string>

#include "../../include/w2v2.h"
#include "gemm_bf16_route.h"
#include "attention_route.h"

namespace w2v2 {

// ---- error plumbing (no exceptions across the C ABI) ----------------------
void set_error(const char* fmt, ...);

#define W2V2_HIP_CHECK(expr)                                                            \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            ::w2v2::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                              __FILE__, __LINE__);                                      \
            return W2V2_EHIP;                                                           \
        }                                                                               \
    } while (0)

#define W2V2_REQUIRE(cond, ...)                \
    do {                                       \
        if (!(cond)) {                         \
            ::w2v2::set_error(__VA_ARGS__);    \
            return W2V2_EINVAL;                \
        }                                      \
    } while (0)

// A kernel's dynamic LDS limit, raised once per kernel (the call is idempotent; the flag is atomic so that concurrent host threads
// agree on it).  `bytes` is a constant of the kernel.
template <auto Kernel>
int set_dynamic_lds(size_t bytes) {
    static std::atomic<bool> done{false};
    if (!done) {
        W2V2_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        done = true;
    }
    return W2V2_OK;
}

// ---- tuning knobs -----------------------------------------------------------
// The shipping library has NO environment reads: every knob is its measured default, folded at compile time.  The tools-only
// build (`python build.py --tuning` -> lib/libw2v2_tuning.so, -DW2V2_TUNING) reads the same names from the environment for
// the sweeps and timing ablations recorded under profiles/; tests and bench.py never load it.
#ifdef W2V2_TUNING
int tune_int(const char* name, int dflt);      // getenv + atoi, read on every call (w2v2_api.hip)
#else
constexpr int tune_int(const char*, int dflt) { return dflt; }
#endif

// ---- tile order of the large-tile GEMM kernels inside an XCD's run of tiles (round 6) ----
// Every GEMM kernel hands each XCD (blockIdx % 8) one contiguous run of the linear tile order, so that tiles in flight together on
// an XCD share operand panels in ITS L2 (4 MB).  With the linear order row-major (N fastest), the ~64 tiles an XCD has in flight are
// 64 / tiles_n rows x ALL tiles_n columns: on the wide shapes (N = 3072 / 4096: 12 - 32 column tiles) that is 2 - 5 row panels of A
// beside the WHOLE of B, streamed through L2 again for every such set -- PMC (profiles/hbm_traffic_configs.json, round 5): the bf16
// q|k|v / FFN-up kernels of the large model fetched 577 MB per launch for 57 MB of operands, the fp32 256 x 128 instances 960 MB.
// Grouped order: the run walks groups of `gm` tile rows, column-major inside a group; gm is the number of A row panels
// (BM x K elements each) that fit a 3.25-MB share of the L2, so a group's A panels stay resident while B streams past them ONCE per
// group instead of once per 64 tiles; the tiles in flight form a gm x (64 / gm) patch.  gm = 0 keeps the linear order (narrow N, the
// weight-gradient form with its own shorter-dimension-fastest rule).  Bijective for any tile count (the last group is shorter).
__device__ __forceinline__ void grouped_tile(int t, int tiles_m, int tiles_n, int gm, int& tm, int& tn) {
    const int per = gm * tiles_n, grp = t / per, first = grp * gm;
    const int rows = min(gm, tiles_m - first), tl = t - grp * per;
    tn = tl / rows;
    tm = first + (tl - tn * rows);
}
// host side: group height for a launch (0 = linear order).  a_panel_bytes = BM x K x element size; inflight = tiles an XCD runs at once
inline int tile_group_rows(int tiles_m, int tiles_n, int64_t a_panel_bytes, int inflight) {
    const int forced = tune_int("W2V2_TILE_GROUP", -1);
    if (forced >= 0) return forced > tiles_m ? tiles_m : forced;
    if (tiles_m < tiles_n || tiles_n < 6) return 0;      // narrow outputs: inflight / tiles_n rows x all columns is already the patch
    int64_t gm = (int64_t)3407872 / (a_panel_bytes > 0 ? a_panel_bytes : 1);      // 3.25 MB of the 4-MB L2 for the resident A panels
    const int need = (inflight + tiles_n - 1) / tiles_n;      // never fewer rows than the linear order has in flight
    if (gm < need) gm = need;
    if (gm < 2) gm = 2;
    // an XCD's run covers tiles_m / 8 rows: split them into equal groups no taller than that (B streams past once per group)
    const int rows_xcd = (tiles_m + 7) / 8;
    if (gm < rows_xcd) {
        const int ngroups = (int)((rows_xcd + gm - 1) / gm);
        gm = (rows_xcd + ngroups - 1) / ngroups;
    }
    return (int)(gm > tiles_m ? tiles_m : gm);
}

// ---- kernel families (one row each in profiles/ and in the roofline) ------
enum Family {
    FAM_CONV0_STATS = 0,   // conv0 recompute + per-(sample,channel) sum/sumsq   (HBM: wave read)
    FAM_CONV0_APPLY,       // conv0 recompute + GroupNorm + GELU + single write  (HBM: 100.76 MB/utt write)
    FAM_GEMM,              // fp32 MFMA GEMM / implicit-GEMM conv / Dense        (MFMA f32)
    FAM_GEMM_BF16,         // same contractions, bf16 operands / fp32 accumulate (MFMA bf16; precision mode 1)
    FAM_GEMM_SPLIT,        // same contractions, fp32 operands as 3 bf16 terms each, 6 MFMA products (precision mode 2)
    FAM_LAYERNORM,         // row LayerNorm (+GELU)                              (HBM)
    FAM_POSCONV,           // grouped positional conv, MFMA 16x16x4 f32          (MFMA f32)
    FAM_ATTENTION,         // fused QK^T-softmax-PV, MFMA 32x32x2 f32            (MFMA f32)
    FAM_CTC,               // CTC alpha/beta                                     (latency)
    FAM_MISC,              // frame lengths, weight-norm regroup, packing, spec-augment, residual adds, transposes
    // training-step-only families (train_kernels.hip, shadow.hip): HBM-bound element-wise passes and reductions
    FAM_DROPOUT,           // dropout forward / backward (+ GELU / GELU', + fused column sums)   (HBM / VALU)
    FAM_REDUCE,            // column sums: bias gradients, weight-gradient slab folds            (HBM)
    FAM_LN_BWD,            // LayerNorm backward (+ its partial-sum fold)                        (HBM)
    FAM_OPTIMIZER,         // Adam (one launch over a chunk table) + the weight-shadow refresh   (HBM)
    FAM_COUNT
};
const char* family_name(int f);

// plane formats of the pre-split GEMM operands (gemm_split_sw.hip): three bf16 planes, x = p0 + p1 + p2 exactly (precision mode
// bf16x3), or two fp16 planes of x S (precision mode f16x2; helpers further down)
enum PlaneFmt { PF_BF16X3 = 0, PF_F16X2 = 1 };
constexpr int plane_count(int fmt) { return fmt == PF_F16X2 ? 2 : 3; }
// where a producing kernel leaves the planes of its output for the consumer GEMM (same element layout as the fp32 output; null p = none)
struct PlaneOut {
    uint16_t* p = nullptr;
    int64_t plane = 0;         // elements between planes
    int fmt = PF_BF16X3;
    int* range_flag = nullptr; // f16x2: sticky overflow flag in device memory
};

// Kernel launches actually enqueued, per family (an op-level call may enqueue several kernels: main + tail tiles, a partial
// and a final reduction ...).  Every launch in csrc/ goes through W2V2_LAUNCH; the family is the innermost live ProfScope's
// (FAM_MISC outside any).  Process-wide counters, cleared by profiler_reset; read by w2v2_profile_kernel_launches.
extern thread_local int tl_launch_family;
void note_kernel_launch();
int64_t kernel_launches(int family);
#define W2V2_LAUNCH(...)                  \
    do {                                  \
        ::w2v2::note_kernel_launch();     \
        hipLaunchKernelGGL(__VA_ARGS__);  \
    } while (0)

// A launch record sink.  When `enabled`, every launch wrapper brackets its
// kernel with an event pair on the launch stream and logs algorithmic
// flops/bytes; reading synchronises the events.
struct Profiler;
Profiler* profiler_create();
void profiler_destroy(Profiler*);
void profiler_enable(Profiler*, bool on);
void profiler_set_mask(Profiler*, unsigned family_mask);   // bit f = record family f; 0 = all
void profiler_set_stride(Profiler*, int stride);           // every stride-th launch of a family gets the event pair
int64_t profiler_seen(const Profiler*, int family);        // launches since the last reset, sampled or not
int64_t profiler_kernel_launches(const Profiler*, int family);      // kernels enqueued (process-wide counter) since THIS profiler's last reset
bool profiler_enabled(const Profiler*);
void profiler_reset(Profiler*);
// returns a token (>=0) to pass to profiler_end, or -1 when disabled
int profiler_begin(Profiler*, int family, double flops, double bytes, hipStream_t s);
void profiler_end(Profiler*, int token, hipStream_t s);
int profiler_read(Profiler*, int family, int64_t* launches, double* ms, double* flops, double* bytes);

// (a scope opened inside another one -- a launcher with its own scope called from a launcher that has one -- neither brackets its
//  kernels again nor re-labels their launches: time and launch counts stay with the OUTER family, nothing is counted twice)
extern thread_local int tl_prof_depth;
struct ProfScope {
    Profiler* p;
    int tok;
    hipStream_t s;
    int outer_family;
    ProfScope(Profiler* p_, int family, double flops, double bytes, hipStream_t s_)
        : p(p_), tok((p_ && tl_prof_depth == 0) ? profiler_begin(p_, family, flops, bytes, s_) : -1), s(s_), outer_family(tl_launch_family) {
        if (tl_prof_depth++ == 0) tl_launch_family = family;
    }
    ~ProfScope() {
        if (--tl_prof_depth == 0) tl_launch_family = outer_family;
        if (tok >= 0) profiler_end(p, tok, s);
    }
};

// The profiler of the model whose training step is running on this thread: the training-only kernels (train_kernels.hip,
// shadow.hip) take no Profiler argument; their launchers read it from here (null outside w2v2_train_* / w2v2_adam_step).
extern thread_local Profiler* tl_step_prof;
struct StepProfScope {
    Profiler* outer;
    explicit StepProfScope(Profiler* p) : outer(tl_step_prof) { tl_step_prof = p; }
    ~StepProfScope() { tl_step_prof = outer; }
};

// ---- operator launchers (defined one per .hip file) ------------------------
// All return 0 / negative W2V2_E*; `prof` may be null.
int launch_gemm(Profiler* prof, const float* A, int64_t lda, int64_t strideA, const float* B,
                int64_t ldb, float* C, int64_t ldc, int64_t strideC, const float* bias,
                const float* residual, int M, int N, int K, int nbatch, int act, hipStream_t s);

// fp32 GEMM on the LDS-ring kernels (gemm_f32_sw.hip): tile 0 = 256 x 128, 1 = 128 x 128, 2 = 64 x 64; persist: at most two blocks per CU,
// each looping over its tiles.  launch_gemm routes to them (gemm_f32_route.h); gemm_f32_ring_ok says whether a shape fits.
void gemm_f32_force_ring(int route);      // this thread's next launch_gemm calls: 0 double buffer | 1 ring | 2 persistent ring, -1 = by shape
void gemm_f32_ring_launches(int64_t* counts /* [4]: 256 x 128, 128 x 128, 64 x 64, 64 x 64 quarters */);      // launches so far, this process
bool gemm_f32_ring_ok(int tile, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, int64_t strideB,
                      int M, int N, int K);
int launch_gemm_f32_ring(int tile, bool persist, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb,
                         int64_t strideB, float* C, int64_t ldc, int64_t strideC, const float* bias, const float* residual, int M,
                         int N, int K, int nbatch, int act, hipStream_t s);
// ... split at main_tiles of the 128 x 128 tile order: those at 128 x 128, the rest as 64 x 64 quarters (M % 128 == 0, N % 128 == 0)
int launch_gemm_f32_ring_split(bool persist, int64_t main_tiles, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                               int64_t ldc, const float* bias, const float* residual, int M, int N, int K, int act, hipStream_t s);

// precision mode 1: operands rounded to bf16 on the way into LDS, fp32 accumulate (gemm_bf16.hip)
int launch_gemm_bf16(Profiler* prof, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb,
                     int64_t strideB, float* C, int64_t ldc, int64_t strideC, const float* bias,
                     const float* residual, int M, int N, int K, int nbatch, int act, hipStream_t s);
// fp32 GEMM as six bf16 MFMA products per fp32 product (gemm_split.hip, precision mode 2): A fp32 (M, K) rows lda apart,
// the weight pre-split by launch_split_weight into three bf16 planes stored as the kernel's LDS images (3 N K elements).
bool gemm_split_supported(const float* A, int64_t lda, int64_t strideA, int M, int N, int K);
int launch_split_weight(const float* w, uint16_t* planes, int K, int N, hipStream_t s);
int launch_gemm_split(Profiler* prof, const float* A, int64_t lda, int64_t strideA, const uint16_t* planes, float* C, int64_t ldc,
                      int64_t strideC, const float* bias, const float* residual, int M, int N, int K, int nbatch, int act,
                      hipStream_t s);

// ... and with BOTH operands pre-split (gemm_split_sw.hip), in plane format `fmt` (PlaneFmt below: three bf16 planes = precision mode
// bf16x3, two fp16 planes = precision mode f16x2): the activation as row-major planes `planeA` elements apart (written by its
// producer; launch_split_planes is the unfused form), the weight as that kernel's LDS images (launch_split_weight_sw: plane_count x N x K
// elements; the f16x2 format also needs two scratch words, whose second is the `out_scale` the GEMM reads); the result as fp32 (C,
// + residual) or as the planes of (acc + bias -> act) for the next GEMM (C16, planeC).  range_flag: sticky overflow flag of f16x2.
bool gemm_split_sw_ok(const uint16_t* A16, int64_t planeA, int64_t lda, int64_t strideA, int M, int N, int K);
int launch_split_weight_sw(const float* w, uint16_t* img, int K, int N, int fmt, void* scratch, hipStream_t s);
int launch_split_planes(const float* x, uint16_t* planes, int64_t plane, int64_t n, int fmt, int* range_flag, hipStream_t s);
int launch_gemm_split_sw(Profiler* prof, int fmt, const uint16_t* A16, int64_t planeA, int64_t lda, int64_t strideA, const uint16_t* Bimg,
                         const float* out_scale, float* C, uint16_t* C16, int64_t planeC, int64_t ldc, int64_t strideC, const float* bias,
                         const float* residual, int M, int N, int K, int nbatch, int act, int* range_flag, hipStream_t s);

// selftest.hip: counts the float patterns on which erf_select / tanh_select differ from the device library's erff / tanhf
int launch_check_select_forms(unsigned long long* mismatches_dev /* [2] */, hipStream_t s);
// ... and those on which gelu_erf_epi (the fp32 GEMM epilogue) / gelu_erf_select differ from gelu_erf; y = gelu_erf(x) element-wise
int launch_check_gelu_epilogue(unsigned long long* mismatches_dev /* [2] */, hipStream_t s);
int launch_gelu_reference(const float* x, float* y, int64_t n, hipStream_t s);

// Optional bf16 shadows of the operands (precision mode 1).  A shadow holds nearest-even bf16 roundings of the fp32
// tensor -- exactly what the kernel would round to itself -- so using one changes speed, never results.
//   A16: same shape / strides (in elements) as A;   B16: B TRANSPOSED, [N][K] with row stride ldb16 (0 = K);
//   C16: bf16 copy of the output for the consumer GEMM (C itself may then be null: the fp32 store is skipped).
struct GemmShadows {
    const uint16_t* A16 = nullptr;
    const uint16_t* B16 = nullptr;
    uint16_t* C16 = nullptr;
    int64_t ldb16 = 0;
    // A is stored TRANSPOSED: element (m, k) at A[k * lda + m] (fp32).  The weight-gradient GEMM dW = X^T dY passes the
    // activation X itself this way, so no transposed copy of X is made in precision mode 1.
    bool transA = false;
    // two-level batch z = zo * zmod + zi for a grouped conv run as one GEMM launch: A(16) advances with z (strideA), B16 and
    // bias with zi (strideB16, strideBias), C / residual with zo * strideC2 + zi * strideC.  zmod = 0: plain batch.
    int zmod = 0;
    int64_t strideB16 = 0, strideC2 = 0, strideBias = 0;
    int64_t strideB2 = 0;        // fp32 B with a two-level batch: B advances with zo * strideB2 + zi * strideB
    bool overlapA = false;       // transposed A whose rows overlap (lda < M): the packed positional-conv input
    // SRC 7 (fp32 transposed A) only: the K dimension is a concatenation of segments of `kseg` rows (a multiple of 64) that lie segA (A) /
    // segB (B) elements apart -- the positional-conv kernel gradient contracts over the frames of SEVERAL samples in one accumulator
    // (segment = sample) instead of writing one slab per sample.  kseg = 0: contiguous K.
    int kseg = 0;
    int64_t segA = 0, segB = 0;
    // transposed-A form only: also write the column sums of B over each batch's K rows to colsum[z * strideCS + n]
    // (dW = X^T dY has the bias gradient 1^T dY for free: dY is in registers while it is staged)
    float* colsum = nullptr;
    int64_t strideCS = 0;
    // transposed-A form with BOTH operands from bf16 shadows in their natural row-major layouts: A16 = bf16 copy of the
    // (K, M) activation (same lda / strideA as A), B16p = bf16 copy of the (K, N) gradient (same ldb / strideB as B).  Both then
    // stream into LDS by DMA as they lie in memory ([k][m] and [k][n] rows) and the k-contiguous MFMA fragments come out of the
    // transposing LDS read ds_read_b64_tr_b16 (gemm_bf16.hip: gemm_bf16_tr_kernel).  No column sums in this form (they are sums
    // of the UNROUNDED gradient): `colsum` must be null.
    const uint16_t* B16p = nullptr;
    // (that form only) the K dimension really has validK rows over all batches, K * nbatch >= validK > K * (nbatch - 1): rows past
    // it are read as zero.  0 = K * nbatch.  Lets dW = X^T dY run over B T = 23984 rows (T = 1499) without a leftover-row pass.
    int64_t validK = 0;
    // transposed-A shadow form on the 128 x 256 kernel: the first `kextra` batches (slabs) own one K tile (64 rows) more than K says
    // and every slab starts where the previous one ends -- K dimension = 64 (nbatch K / 64 + kextra) rows, strideA / strideB = K rows.
    // Lets the rows be cut into ANY number of slabs (7 x 72 tiles = 504 of the 512 block slots instead of 6 x 72 = 432).
    int kextra = 0;
    // ... and when validK ends inside the last K tile of the last slab, that kernel takes the ragged form too IF the caller keeps the
    // row of B16p just past the end (row validK) all-zero: the missing rows are then read from there (and from A's last row).
    bool b_zero_row = false;
    int force_kernel = 0;        // forward form with both shadows: 0 = by shape, 1 = the 128 x 128 kernel, 2 = the 128 x 256 software-pipelined one
};
// 128 x 256 software-pipelined form, two 4-wave blocks per CU (gemm_bf16_sw.hip): same arithmetic, identical bits.  Which shapes they
// take (gemm_bf16_sw_ok, gemm_bf16_swtr_ok) and which stream A's shadow (gemm_bf16_streams_a16): gemm_bf16_route.h
int launch_gemm_bf16_sw(const uint16_t* A16, int64_t lda, int64_t strideA, const uint16_t* B16, int64_t ldb16, float* C, uint16_t* C16,
                        int64_t ldc, int64_t strideC, const float* bias, const float* residual, int M, int N, int K, int nbatch, int act,
                        hipStream_t s);
int launch_gemm_bf16_swtr(const uint16_t* A16, int64_t lda, int64_t strideA, const uint16_t* B16, int64_t ldb, int64_t strideB, float* C,
                          int64_t ldc, int64_t strideC, int M, int N, int K, int nbatch, hipStream_t s, int kextra = 0, int krag = 0);
void gemm_bf16_launches(int64_t* counts /* [GB_KERNELS], by GemmBf16Kernel */);      // launch_gemm_bf16_x's launches so far, this process
int launch_gemm_bf16_x(Profiler* prof, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb,
                       int64_t strideB, float* C, int64_t ldc, int64_t strideC, const float* bias,
                       const float* residual, int M, int N, int K, int nbatch, int act, const GemmShadows& x,
                       hipStream_t s);
// launch_gemm / launch_gemm_ex route to launch_gemm_bf16 while the calling thread's precision is 1.  The
// API entry points set it from the model for the duration of one call (PrecisionScope).
void gemm_set_precision(int mode);
int gemm_get_precision();
struct PrecisionScope {
    int prev;
    explicit PrecisionScope(int mode) : prev(gemm_get_precision()) { gemm_set_precision(mode); }
    ~PrecisionScope() { gemm_set_precision(prev); }
};
int launch_gemm_ex(Profiler* prof, const float* A, int64_t lda, int64_t strideA, const float* B,
                   int64_t ldb, int64_t strideB, float* C, int64_t ldc, int64_t strideC, const float* bias,
                   const float* residual, int M, int N, int K, int nbatch, int act, hipStream_t s);

int launch_layer_norm(Profiler* prof, const float* x, float* y, const float* gamma,
                      const float* beta, int64_t rows, int C, float eps, int act, hipStream_t s);

int launch_layer_norm_x(Profiler* prof, const float* x, float* y, const float* gamma, const float* beta, int64_t rows,
                        int C, float eps, int act, uint16_t* y16 /* optional bf16 shadow of y */, hipStream_t s,
                        const PlaneOut* planes = nullptr /* optional planes of y (precision modes bf16x3 / f16x2; C % 4 == 0) */);

// ---- packed variable-length forward (w2v2_forward_packed) --------------------------------------------------------------
// The utterances sit back to back in one stream.  Utterance i starts at stream sample s0, a multiple of the alignment unit
// (a multiple of the conv stack's total stride and of conv0's stride x its stats chunk), so its frames at every conv layer
// start at s0 / (that layer's cumulative stride) and its conv0 rows at a chunk boundary.  Its span, [s0, next s0), holds its
// samples and then zeros.
struct PackSeg {
    int64_t s0, len, src0;        // first stream sample, samples, offset in the caller's dense concatenation
    int32_t f0, nf, out0, keep0;  // first stream frame, frames (w2v2_num_frames(len)), first row of the caller's output, first of
                                  // the utterance's frames that goes there (w2v2_forward_windows; the rows up to the next out0)
};
// one tile of an utterance's frames: rows [t0, t0 + tile rows) of the nf frames that start at stream frame f0
struct SegTile {
    int32_t f0, nf, t0, pad;
};
// index of the span that holds stream sample `pos` (spans tile the stream; segs sorted by s0)
__device__ __forceinline__ int pack_seg_of_sample(const PackSeg* segs, int n, int64_t pos) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].s0 <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

int64_t conv0_ws_floats(int B, int64_t L, int K, int stride, int C);
int conv0_chunk_frames();     // conv0 rows per statistics chunk
// group-norm conv0 over a packed stream of L samples: statistics per utterance over exactly its rows (no padding, no
// neighbour), applied with that utterance's scale and shift.  ws: conv0_ws_floats(1, L, ...); scale_shift: (nseg, 2, C).
int launch_conv0_packed(Profiler* prof, const float* wave, const float* kernel, const float* bias, const float* gamma,
                        const float* beta, float* out, float* ws, float* scale_shift, int64_t L, int K, int stride, int C,
                        float eps, int act, const PackSeg* segs, int nseg, hipStream_t s,
                        const PlaneOut* planes = nullptr /* optional planes of out (K = 10, stride 5, C % 4 == 0; out may then be null) */,
                        double* gram_ws = nullptr /* conv0_gram_ws_doubles(): statistics in the dense pass's form, as each utterance alone */,
                        int max_seg_frames = 0 /* with gram_ws: conv0 rows of the longest utterance */,
                        uint16_t* out16 = nullptr /* optional bf16 shadow of out, as launch_conv0_x writes it (out may then be null) */);
int64_t conv0_gram_ws_doubles(int64_t L, int stride, int nseg);
int launch_conv0(Profiler* prof, const float* wave, const float* kernel, const float* bias,
                 const float* gamma, const float* beta, float* out, float* ws, int B, int64_t L,
                 int K, int stride, int C, float eps, int norm_mode, int act, hipStream_t s);

int launch_conv0_x(Profiler* prof, const float* wave, const float* kernel, const float* bias,
                   const float* gamma, const float* beta, float* out, uint16_t* out16 /* optional bf16 shadow */, float* ws,
                   int B, int64_t L, int K, int stride, int C, float eps, int norm_mode, int act, hipStream_t s,
                   const PlaneOut* planes = nullptr /* optional planes of the output (the K = 10, stride 5, C % 4 == 0 kernel only) */);
// fp32 -> bf16 (nearest even): plain copy, and [K][N] -> [N][K] transpose (GEMM weight shadows)
int launch_to_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t s);
// one 64 x 64 tile of one weight for the single-launch shadow refresh (shadow.hip): w (K, N) fp32 -> wt (N, K) bf16 and / or
// plain (K, N) bf16 (either may be null)
struct ShadowJob {
    const float* w;
    uint16_t* wt;
    uint16_t* plain;
    int K, N, k0, n0;
};
int launch_weight_shadows_multi(const ShadowJob* jobs_dev, int njobs, hipStream_t s);
int launch_transpose_to_bf16(const float* w, uint16_t* wt, int K, int N, hipStream_t s);
int launch_transpose_to_bf16_batched(const float* w, uint16_t* wt, int K, int N, int nbatch, hipStream_t s);   // nbatch dense (K, N) matrices

int launch_weight_norm_regroup(Profiler* prof, const float* wv, const float* wg, float* out, int K,
                               int cg, int H, int groups, hipStream_t s);
int launch_pos_conv(Profiler* prof, const float* x, const float* wg, const float* bias,
                    const int32_t* frame_len, float* y, int B, int T, int H, int K, int groups,
                    int act, hipStream_t s);

// precision mode 1: the grouped positional conv as one batched bf16 GEMM (posconv.hip)
int64_t pos_conv_bf16_pack_elems(int B, int T, int H, int K);
int launch_pos_conv_weight_shadow(const float* wg, uint16_t* w16, int K, int cg, int groups, hipStream_t s);
int launch_pos_conv_bf16(Profiler* prof, const float* x, const uint16_t* w16, const float* bias, const int32_t* frame_len,
                         float* y, float* pre_act, uint16_t* pack16, float* xz_ws, int B, int T, int H, int K, int groups,
                         int act, int pad_left, int add_residual, hipStream_t s);

// kernel gradient of the positional conv as a batched transposed-A GEMM (precision mode 1, T % 64 == 0):
//   dwg (groups, K, cg, og) = sum over samples and frames; pack32: (B, G, 64 ceil(T/64)+K-1, cg) fp32 scratch, slabs: B * K*cg*H fp32 scratch
int pos_conv_dw_bf16_slabs(int B, int H, int K, int groups);      // the slab count S (1, 2 or 4) launch_pos_conv_dw_bf16 picks
void pos_conv_dw_bf16_ws_floats(int B, int T, int H, int K, int groups, int64_t sizes[4], int* S_out);   // pack32, slabs, red_ws, dc_pad
int launch_pos_conv_dw_bf16(Profiler* prof, const float* xz, const float* dc, float* dwg, float* pack32, float* slabs, float* red_ws,
                            int B, int T, int H, int K, int groups, hipStream_t s, float* dc_pad = nullptr /* (B, 64 ceil(T/64), H): T % 64 != 0 */);

// packed forward, fp32: the positional conv over tiles of 128 frames (pos_conv_packed_rows()), each utterance zero-padded at its
// own edges; attention over tiles of AttnRoute::rows queries, keys restricted to the tile's utterance.  x / y and
// qkv / ctx are (frames, H) / (frames, 3H) stream buffers.
int pos_conv_packed_rows();
int launch_pos_conv_packed(Profiler* prof, const float* x, const float* wg, const float* bias, float* y, const SegTile* tiles,
                           int ntiles, int64_t frames, int H, int K, int groups, int act, hipStream_t s);
// packed forward, precision mode 1 (posconv.hip, attention_bf16.hip): segment forms of launch_pos_conv_bf16 (pad_left = K / 2,
// residual on; rows of y no utterance owns are zeroed) and of launch_attention_fwd_bf16 over a table of
// 128-query tiles; each utterance's output is bit for bit what the dense launcher gives it alone
int launch_pos_conv_bf16_packed(Profiler* prof, const float* x, const uint16_t* w16, const float* bias, float* y, const PackSeg* segs,
                                int nseg, int64_t frames, int H, int K, int groups, int act, hipStream_t s);
int launch_attention_bf16_packed(const float* qkv, const uint16_t* qkv16, float* ctx, uint16_t* ctx16, const SegTile* tiles, int ntiles,
                                 int64_t frames, double sum_nf2, int H, int heads, hipStream_t s);
// packed.hip: caller's samples (from src0 on, per utterance) -> aligned stream (gaps zeroed); stream rows -> caller's rows.
// stats: null (a copy), or launch_pack_stats' (nseg, 2) fp64 (mean, sqrt(var + eps)): (x - mean) / that, formed in fp64
int launch_pack_scatter(const float* src, float* stream, int64_t L, const PackSeg* segs, int nseg, hipStream_t s,
                        const double* stats = nullptr);
int launch_pack_stats(const float* src, const PackSeg* segs, int nseg, double eps, double* stats, hipStream_t s);
int launch_pack_gather(const float* stream_rows, float* out, int64_t out_rows, int width, const PackSeg* segs, int nseg,
                       hipStream_t s);
// zero the stream rows no utterance owns -- [f0 + nf, next f0) behind each, [f0 + nf, frames) behind the last -- of an fp32
// (frames, width) buffer (x, may be null), of its planes (pl, may be null) and of its bf16 shadow (x16, may be null): what the
// segment kernels never write stays defined
int launch_pack_zero_gaps(float* x, const PlaneOut* pl, int64_t frames, int width, const PackSeg* segs, int nseg, hipStream_t s,
                          uint16_t* x16 = nullptr);

// grow-only device scratch per (purpose, stream), owned by the library (shadow.hip)
enum ScratchSlot { SCRATCH_SPLITK = 0, SCRATCH_CTC = 1, SCRATCH_QKV16 = 2, SCRATCH_DCTX16 = 3, SCRATCH_ALIGN = 4, SCRATCH_BEAM = 5, SCRATCH_WINDOWS = 6,
                   SCRATCH_CUTS = 7, SCRATCH_RESAMPLE = 8, SCRATCH_EDIT = 9, SCRATCH_ALIGN_LONG = 10, SCRATCH_SCORE = 11, SCRATCH_SPOT = 12, SCRATCH_SCORE_GRAD = 13,
                   SCRATCH_SCORE_STAR = 14, SCRATCH_SCORE_GRAD_STAR = 15, SCRATCH_POS_PACKED = 16, SCRATCH_AUGMENT = 17, SCRATCH_SLOTS = 18 };
int stream_scratch(int slot, hipStream_t s, size_t bytes, void** out);
int stream_scratch_release();       // frees the calling device's scratch buffers and staged-upload buffers
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }      // the parts of a workspace begin at multiples of 256 bytes
// pinned staging of a small host table on its way to the device (shadow.hip): grow-only, and the previous upload out of it has
// completed before it is rewritten.  One per owner, who serialises its users: a model; a device's entry of a library-wide map, under that map's lock.
struct PinnedStage {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;     // recorded behind the last upload out of p
};
int pinned_stage_begin(PinnedStage& st, size_t bytes, size_t min_bytes);             // waits for the previous upload; st.p then holds >= bytes (a new buffer: >= min_bytes)
int pinned_stage_upload(PinnedStage& st, void* dst, size_t bytes, hipStream_t s);    // dst <- st.p[0, bytes) on s
void pinned_stage_free(PinnedStage& st);
// A family's host tables on their way into its workspace (shadow.hip), through a library-owned pinned buffer per (slot, device)
// (a new one: >= min_bytes).  Waits (host-side) for the slot's previous upload on this device only: one lock per slot.
// staged_fill: fill(stage) writes `bytes` bytes in place, which are then uploaded to dst on s.
// staged_upload: the blocks, in ascending order of offset and not overlapping, go to their byte offsets, the gaps between them
// are zeroed, and [0, end of the last block) is uploaded.
int staged_fill_raw(int slot, hipStream_t s, void* dst, size_t bytes, size_t min_bytes, void (*fill)(void* stage, void* ctx), void* ctx);
template <class F>
int staged_fill(int slot, hipStream_t s, void* dst, size_t bytes, size_t min_bytes, F&& fill) {
    return staged_fill_raw(slot, s, dst, bytes, min_bytes, [](void* stage, void* ctx) { (*static_cast<std::remove_reference_t<F>*>(ctx))(stage); },
                           const_cast<void*>(static_cast<const void*>(&fill)));
}
struct StageBlock {
    const void* src;
    size_t bytes, offset;
};
int staged_upload(int slot, hipStream_t s, void* dst, std::initializer_list<StageBlock> blocks, size_t min_bytes);
// one layer's q | k | v projections <-> the packed (H, 3H) kernel and (3H) bias (shadow.hip); unpack skips null targets
int launch_qkv_pack(float* packed_w, float* packed_b, const float* const w[3], const float* const b[3], int H, hipStream_t s);
int launch_qkv_pack_layers(float* const* packed_w, float* const* packed_b, const float* const* w, const float* const* b, int layers, int H, hipStream_t s);
int launch_qkv_unpack(const float* packed_w, const float* packed_b, float* const w[3], float* const b[3], int H, hipStream_t s);
// ---- attention: attention_route (attention_route.h) decides, these execute ----
static_assert(PF_BF16X3 == 0 && PF_F16X2 == 1, "AttnRoute::fmt is a PlaneFmt");
bool attention_split_allowed();      // W2V2_SPLIT_ATTN (tools/nll_drift_probe.py separates the attention from the GEMMs): its one reader
// the problem of a caller that has no pointers yet (a plan) or whose buffers are 16-byte aligned by construction
inline AttnProblem attention_problem(int pass, int precision, int B, int T, int H, int heads, bool packed, bool want_f32 = true, bool want_b16 = false,
                                     bool want_planes = false, bool io_aligned = true) {
    return AttnProblem{pass, precision, B, T, H, heads, packed, attention_split_allowed(), io_aligned, want_f32, want_b16, want_planes};
}
struct AttnTrain;
// What a routed launch reads and writes.  A form the route's family does not use may be null; qkv16 is optional everywhere (the bf16
// kernels round qkv into scratch without it), and with ctx16 the fp32 ctx may be null.
struct AttnIO {
    const float* qkv = nullptr;
    const uint16_t* qkv16 = nullptr;
    const int32_t* frame_len = nullptr;      // dense: (B) valid frames, or null
    const SegTile* tiles = nullptr;          // packed: one entry per AttnRoute::rows queries of an utterance, utterance by utterance
    int ntiles = 0;
    int64_t frames = 0;                      // ... the stream's frames and the sum of squared utterance frames (sizes the profile)
    double sum_nf2 = 0.0;
    float* ctx = nullptr;                    // (backward: the forward's output, read)
    uint16_t* ctx16 = nullptr;
    const PlaneOut* planes = nullptr;        // split family: planes of ctx and / or the f16x2 range flag
    const AttnTrain* train = nullptr;        // training forward and backward
    // backward: dctx (B, T, H) in, dqkv (B, T, 3H) out, each as fp32 and / or bf16; dvec_ws (B, heads, T) scratch; colpart: see launch_attention_bwd_bf16
    const float* dctx = nullptr;
    const uint16_t* dctx16 = nullptr;
    float* dqkv = nullptr;
    uint16_t* dqkv16 = nullptr;
    float *dvec_ws = nullptr, *colpart = nullptr;
};
int launch_attention_routed(Profiler* prof, const AttnRoute& route, const AttnIO& io, hipStream_t s);            // AP_INFER, dense or packed
int launch_attention_train_routed(Profiler* prof, const AttnRoute& route, const AttnIO& io, hipStream_t s);      // AP_TRAIN
int launch_attention_bwd_routed(Profiler* prof, const AttnRoute& route, const AttnIO& io, hipStream_t s);        // AP_BWD
void attention_launches(int64_t* counts);      // AK_KERNELS launch counts of the three launchers above
// The op-level forms: the problem comes from the calling thread's precision (gemm_get_precision) and the pointers' alignment.
int launch_attention(Profiler* prof, const float* qkv, const int32_t* frame_len, float* ctx, int B,
                     int T, int H, int heads, hipStream_t s);
// qkv16: optional bf16 shadow of qkv (precision mode 1 with head size 64 reads ONLY it; qkv may then be null.  Without it that
// kernel rounds qkv into scratch first).  ctx may be null when ctx16 is given.
int launch_attention_x(Profiler* prof, const float* qkv, const uint16_t* qkv16, const int32_t* frame_len, float* ctx, int B, int T, int H,
                       int heads, uint16_t* ctx16 /* optional bf16 shadow of ctx (bf16 kernel only) */, hipStream_t s,
                       const PlaneOut* planes = nullptr /* optional planes of ctx (split kernel only: precision modes 2 / 3, head size 64) */);
// The kernels' own launchers (their files keep the kernels in anonymous namespaces): they check their operands and launch.
int launch_attention_split(const float* qkv, const int32_t* frame_len, float* ctx, int B, int T, int H, int heads, hipStream_t s,
                           const PlaneOut* planes = nullptr /* optional planes of ctx; ctx itself may then be null */,
                           int fmt = PF_BF16X3 /* PF_F16X2: two fp16 terms / three products per contraction (precision mode 3) */,
                           int* range_flag = nullptr /* f16x2: sticky flag for q / k / v beyond fp16's scaled range */);
// packed forward, precision modes 2 / 3: the split kernel over the same 256-query tile table as the fp32 segment kernel, keys and
// values restricted to the tile's utterance; each utterance's ctx (and planes) bit-identical to launch_attention_split on it alone
int launch_attention_split_packed(const float* qkv, float* ctx, const SegTile* tiles, int ntiles, int64_t frames, int H, int heads, hipStream_t s,
                                  const PlaneOut* planes, int fmt, int* range_flag);

int launch_frame_lengths(Profiler* prof, const int32_t* mask, int32_t* frame_len, int B, int64_t L,
                         const int32_t* ks, const int32_t* ss, int nl, hipStream_t s);

int launch_ctc(Profiler* prof, const float* logits, int B, int T, int V, const int32_t* labels,
               int U, const int32_t* label_len, const int32_t* logit_len, int blank, float* nll,
               float* grad, hipStream_t s);
// ... with the reference's conventions evaluated on the device (losses.py:29-45): label_len null = count of labels != blank,
// logit_len null = uniform_len frames for every row, the gradient / grad_div (division_factor), loss_sum (optional device
// scalar) = sum_b nll[b] / grad_div.  One call, no host-side tensor arithmetic around it.
int launch_ctc_x(Profiler* prof, const float* logits, int B, int T, int V, const int32_t* labels, int U, const int32_t* label_len,
                 const int32_t* logit_len, int uniform_len, int blank, float grad_div, float* nll, float* grad, float* loss_sum, hipStream_t s);
// CTC forced alignment (align.hip; w2v2_ctc_align): utterance i = logits rows [row0_i, row0_i + frames_i), labels
// [label0_i, label0_i + nlabels_i); per-frame outputs back to back, one score per utterance
int launch_ctc_align(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                     const int64_t* label0, const int32_t* nlabels, int blank, int32_t* token, int32_t* label_index,
                     float* frame_logp, double* score, hipStream_t s);
// ... with the star, the wildcard label V (w2v2_ctc_align_star; the definition in align.hip): star_score <= 0
int launch_ctc_align_star(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                          const int64_t* label0, const int32_t* nlabels, int blank, float star_score, int32_t* token,
                          int32_t* label_index, float* frame_logp, double* score, hipStream_t s);
// ... of whole recordings (align_long.hip; w2v2_ctc_align_long): the same addressing and outputs, any label count; the plane of
// frames x states runs as tiles of panel_frames steps x strip_pairs state pairs (0 = the defaults), one launch per anti-diagonal.
// ctc_align_long_workspace: the bytes of scratch such a call needs (host only; a negative W2V2_E* for bad shapes).  star: the
// label V is the star with that star_score (w2v2_ctc_align_long_star), and the workspace holds xs_t as well
int launch_ctc_align_long(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                          const int64_t* label0, const int32_t* nlabels, int blank, int32_t* token, int32_t* label_index,
                          float* frame_logp, double* score, int strip_pairs, int panel_frames, int64_t max_workspace_bytes,
                          hipStream_t s, bool star = false, float star_score = 0.f);
int64_t ctc_align_long_workspace(int n, const int32_t* frames, const int32_t* nlabels, int strip_pairs, int panel_frames,
                                 bool star = false);
// exact CTC scoring (score.hip, with the definitions; w2v2_ctc_score, w2v2_ctc_score_star): the same addressing of the logits; pair
// j = utterance utt_of[j] against labels [label0_j, label0_j + nlabels_j); one fp64 log-probability per pair, in the caller's
// order.  star: label V is the wildcard, star_score <= 0 its penalty per frame
int launch_ctc_score(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                     const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, bool star, float star_score,
                     double* logp, hipStream_t s);
// its gradient (w2v2_ctc_score_grad, w2v2_ctc_score_grad_star): grad rows, addressed like the logits, = sum_j coef_j d logp_j /
// d logits over each utterance's pairs; utterances in groups whose workspace fits max_workspace_bytes (0: 8 GiB).
// ctc_score_grad_workspace: the bytes of one pass over the whole call (host only; a negative W2V2_E* for bad shapes); with the star
// it also holds the star's emission and the top token of every frame
int launch_ctc_score_grad(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                          const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, bool star, float star_score,
                          const double* coef, double* logp, float* grad, int64_t max_workspace_bytes, hipStream_t s);
int64_t ctc_score_grad_workspace(int n, const int32_t* frames, int m, const int32_t* utt_of, const int32_t* nlabels, int V, bool star);
// CTC phrase search (spot.hip; w2v2_ctc_spot): the same addressing and pairs; per pair max_hits slots of (score, begin, end), the
// true count, and optionally z_t and c_t of every frame from trace0_j on (-1: none)
int launch_ctc_spot(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                    const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, int delim,
                    const double* min_score, int max_hits, double* hit_score, int32_t* hit_begin, int32_t* hit_end, int32_t* count,
                    double* trace_score, int32_t* trace_begin, const int64_t* trace0, hipStream_t s);
// CTC prefix beam search (beam.hip; w2v2_ctc_beam_search): the same addressing of the logits; per utterance nbest rows of max_len
// labels, their lengths (-1: no such hypothesis), score (CTC log-probability over the kept paths) and total (score + LM)
int launch_ctc_beam_search(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank, int beam_width,
                           int nbest, const float* lm_table, int lm_order, float lm_alpha, float lm_beta, int max_len,
                           int32_t* labels_out, int32_t* length, double* score, double* total, hipStream_t s);
// pause cuts of CTC logits (segment.hip; w2v2_ctc_pause_cuts): the same addressing of the logits; per utterance max_cuts slots of
// cuts and pause lengths (-1 behind the last) and the true count
int launch_ctc_pause_cuts(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank, int delim,
                          float margin, int min_pause, int max_cuts, int32_t* cut, int32_t* pause, int32_t* count, hipStream_t s);
// polyphase resampling (resample.hip; w2v2_resample): segment i = in[in0_i, in0_i + in_len_i) through filters[filter_of_i] to
// out[out0_i, ...); resample_design / resample_length are host code
int launch_resample(const float* in, int n, const int64_t* in0, const int64_t* in_len, const int32_t* filter_of,
                    const w2v2_resample_filter* filters, int n_filters, float* out, const int64_t* out0, hipStream_t s);
int resample_design(int rate_in, int rate_out, int zeros, double rolloff, double beta, int32_t* L, int32_t* M, int32_t* K, int32_t* lead,
                    float* table, int64_t table_capacity);
int64_t resample_length(int64_t len, int L, int M);
// waveform augmentation (augment.hip; w2v2_fir, w2v2_mix): segment i = in[in0_i, in0_i + len_i) convolved with its own taps, or with a
// wrapped stretch of noise added at a gain from the two powers, to out[out0_i, + len_i); gain (n floats) may be null
int launch_fir(const float* in, int n, const int64_t* in0, const int64_t* len, const float* taps, const int64_t* taps0, const int32_t* ntaps,
               const int32_t* delay, float* out, const int64_t* out0, int match_power, float* gain, hipStream_t s);
int launch_mix(const float* in, int n, const int64_t* in0, const int64_t* len, const float* noise, const int64_t* noise0,
               const int64_t* noise_len, const int64_t* offset, const double* scale, float* out, const int64_t* out0, float* gain,
               hipStream_t s);
// edit distance and its breakdown (edit.hip; w2v2_edit_distance): pair p = tokens[hyp0_p, + hyp_len_p) against tokens[ref0_p, + ref_len_p);
// out (n_pairs, 4) = distance, substitutions, deletions, insertions
int launch_edit_distance(const int32_t* tokens, int64_t n_tokens, int n_pairs, const int64_t* hyp0, const int32_t* hyp_len,
                         const int64_t* ref0, const int32_t* ref_len, int32_t* out, hipStream_t s);
// the same search with a word n-gram model and a lexicon in place of the table (w2v2_ctc_beam_search_words)
int launch_ctc_beam_search_words(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank,
                                 int beam_width, int nbest, const w2v2_word_lm* lm, int delim, float lm_alpha, float lm_beta,
                                 float unk_penalty, int score_eos, int max_len, int32_t* labels_out, int32_t* length, double* score,
                                 double* total, hipStream_t s);
// either search with a phrase bias (w2v2_ctc_beam_search_biased): the character form when word_lm is null, else the word form
int launch_ctc_beam_search_biased(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank,
                                  int beam_width, int nbest, const float* lm_table, int lm_order, const w2v2_word_lm* word_lm, int delim,
                                  float lm_alpha, float lm_beta, float unk_penalty, int score_eos, const w2v2_ctc_bias* bias, int max_len,
                                  int32_t* labels_out, int32_t* length, double* score, double* total, hipStream_t s);
// any of the four forms, resumable (w2v2_ctc_beam_search_stream): stream i goes on behind its frames_done_i frames from its state slab,
// its trie in nodes[node0_i, node0_i + node_cap_i); labels_out may be null (the call then only advances the state)
int64_t ctc_beam_stream_state_bytes();
int launch_ctc_beam_search_stream(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int64_t* frames_done,
                                  int blank, int beam_width, int nbest, const float* lm_table, int lm_order, const w2v2_word_lm* word_lm,
                                  int delim, float lm_alpha, float lm_beta, float unk_penalty, int score_eos, const w2v2_ctc_bias* bias,
                                  void* state, uint64_t* nodes, const int64_t* node0, const int64_t* node_cap, int max_len,
                                  int32_t* labels_out, int32_t* length, double* score, double* total, int32_t* stable_len, hipStream_t s);

// ---- device helpers ---------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ float gelu_erf(float x) {
    // tf.nn.gelu(approximate=False): 0.5 x (1 + erf(x / sqrt(2)))
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
// The device library's erff (ROCm 7.2 ocml, __ocml_erf_f32) without its branch: the |x| < 1 polynomial and the 1 - exp(-q(|x|))
// form are BOTH evaluated -- the same operations in the same order as the library's two arms -- and the result selected, so every
// input gives the library's bits (tools/erf_exhaustive.hip compares all 2^32 patterns on the GPU; tests/test_ops_gpu.py runs it).
// In a wave of 64 GELU inputs both arms execute anyway; what the select form removes is the control flow, which around 128
// accumulator registers makes the allocator spill (gemm_split_sw.hip: 570 bytes of scratch per lane with the branch, 0 without).
__device__ __forceinline__ float erf_select(float x) {
    const float ax = fabsf(x), t = x * x;
    float p = __builtin_fmaf(t, -0x1.268bc2p-11f, 0x1.420828p-8f);
    p = __builtin_fmaf(t, p, -0x1.b5937p-6f);
    p = __builtin_fmaf(t, p, 0x1.ce077cp-4f);
    p = __builtin_fmaf(t, p, -0x1.81266p-2f);
    p = __builtin_fmaf(t, p, 0x1.06ebap-3f);
    const float small = __builtin_fmaf(ax, p, ax);
    float q = __builtin_fmaf(ax, 0x1.1d3156p-16f, -0x1.8d129p-12f);
    q = __builtin_fmaf(ax, q, 0x1.f9a6d2p-9f);
    q = __builtin_fmaf(ax, q, -0x1.8c3164p-6f);
    q = __builtin_fmaf(ax, q, 0x1.b4e9c8p-4f);
    q = __builtin_fmaf(ax, q, 0x1.4515fap-1f);
    q = __builtin_fmaf(ax, q, 0x1.078e5p-3f);
    q = __builtin_fmaf(ax, q, ax);
    const float large = 1.0f - expf(-q);
    return copysignf(ax < 1.0f ? small : large, x);
}
// ... and the library's tanhf the same way (|x| < 0.625: odd polynomial; else 1 - 2 / (exp(2 |x|) + 1))
__device__ __forceinline__ float tanh_select(float x) {
    const float ax = fabsf(x), t = x * x;
    float p = __builtin_fmaf(t, -0x1.758e7ap-8f, 0x1.521192p-6f);
    p = __builtin_fmaf(t, p, -0x1.b8389cp-5f);
    p = __builtin_fmaf(t, p, 0x1.110704p-3f);
    p = __builtin_fmaf(t, p, -0x1.555532p-2f);
    const float small = __builtin_fmaf(t, ax * p, ax);
    const float large = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(expf(ax * 2.0f) + 1.0f), 1.0f);
    return copysignf(ax < 0.625f ? small : large, x);
}
__device__ __forceinline__ float gelu_tanh_select(float x) {     // == gelu_tanh(x), bit for bit
    const float c = 0.79788456080286535588f;  // sqrt(2/pi)
    return 0.5f * x * (1.0f + tanh_select(c * (x + 0.044715f * x * x * x)));
}
__device__ __forceinline__ float gelu_erf_select(float x) {      // == gelu_erf(x), bit for bit
    return 0.5f * x * (1.0f + erf_select(x * 0.70710678118654752440f));
}
// gelu_erf for the fp32 GEMM epilogue (gemm_epilogue.h): gelu_erf_select with the library expf of the 1 - exp(-q) arm written out
// (the compiler's own expansion: -q log2(e) in two terms, v_exp_f32 of the fraction, v_ldexp_f32 by the integer part) WITHOUT its two
// range selects.  The overflow select (q < -88.7 -> inf) cannot fire on a selected arm: q >= 1 wherever |z| >= 1.  The underflow select
// (q > 103.3 -> 0) is what keeps a huge or infinite z from producing inf - inf; clamping |z| to 4 in front of the q chain does the same
// with one v_min_f32: q(4) = 18.1 and 1 - exp(-q) rounds to 1 from q = 17.33 on, which is the library's value for every |z| >= 4.
// A NaN passes the clamp as 4, and the final 0.5 x (...) is NaN all the same.  Bit for bit gelu_erf over all 2^32 patterns:
// selftest.hip (w2v2_op_check_gelu_epilogue), tests/test_gemm_gelu_epilogue_gpu.py.
__device__ __forceinline__ float gelu_erf_epi(float x) {
    const float z = x * 0.70710678118654752440f, az = fabsf(z), t = z * z;
    float p = __builtin_fmaf(t, -0x1.268bc2p-11f, 0x1.420828p-8f);
    p = __builtin_fmaf(t, p, -0x1.b5937p-6f);
    p = __builtin_fmaf(t, p, 0x1.ce077cp-4f);
    p = __builtin_fmaf(t, p, -0x1.81266p-2f);
    p = __builtin_fmaf(t, p, 0x1.06ebap-3f);
    const float small = __builtin_fmaf(az, p, az);
    const float ac = __builtin_fminf(az, 4.0f);
    float q = __builtin_fmaf(ac, 0x1.1d3156p-16f, -0x1.8d129p-12f);
    q = __builtin_fmaf(ac, q, 0x1.f9a6d2p-9f);
    q = __builtin_fmaf(ac, q, -0x1.8c3164p-6f);
    q = __builtin_fmaf(ac, q, 0x1.b4e9c8p-4f);
    q = __builtin_fmaf(ac, q, 0x1.4515fap-1f);
    q = __builtin_fmaf(ac, q, 0x1.078e5p-3f);
    q = __builtin_fmaf(ac, q, ac);
    const float ph = q * -0x1.715476p+0f;                                        // exp(-q) = 2^(ph + pl)
    const float pl = __builtin_fmaf(q, -0x1.4ae0bep-26f, __builtin_fmaf(q, -0x1.715476p+0f, -ph));
    const float e = __builtin_rintf(ph);
    const float large = 1.0f - __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f((ph - e) + pl), (int)e);
    return 0.5f * x * (1.0f + copysignf(az < 1.0f ? small : large, z));
}
__device__ __forceinline__ float gelu_tanh(float x) {
    const float c = 0.79788456080286535588f;  // sqrt(2/pi)
    return 0.5f * x * (1.0f + tanhf(c * (x + 0.044715f * x * x * x)));
}
// exact GELU 0.5 x (1 + erf(x / sqrt 2)) with erf from Abramowitz-Stegun 7.1.26: |erf error| < 1.5e-7 absolute, ~14 VALU
// ops against ~35 for erff.  Used by the bf16 kernel only (FAST_GELU): its error is a smooth, i.e. BIASED, function of x,
// and through 19 GELU layers that bias moved the fp32 CTC loss of the 246000-sample fixture from 5e-3 to 1.7e-2 off the
// fp64 reference (logits 7.4e-5 -> 8.1e-5) -- invisible next to bf16 rounding, not acceptable for the fp32 path.
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);
    const float erf_abs = fmaf(-p * t, e, 1.0f);             // erf(|x| / sqrt 2)
    return 0.5f * x + 0.5f * fabsf(x) * erf_abs;             // 0.5 x (1 + sign(x) erf(|x| / sqrt 2))
}

// gelu_erf_fast on two values at once (v_pk_mul_f32 / v_pk_fma_f32 where the ISA has packed forms; rcp and exp2 stay scalar)
using f32x2_t = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f32x2_t gelu_erf_fast2(f32x2_t x) {
    const f32x2_t ax = {fabsf(x[0]), fabsf(x[1])};
    const f32x2_t z = ax * f32x2_t{0.70710678118654752440f, 0.70710678118654752440f};
    const f32x2_t d = __builtin_elementwise_fma(f32x2_t{0.3275911f, 0.3275911f}, z, f32x2_t{1.0f, 1.0f});
    const f32x2_t t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    f32x2_t q = __builtin_elementwise_fma(f32x2_t{1.061405429f, 1.061405429f}, t, f32x2_t{-1.453152027f, -1.453152027f});
    q = __builtin_elementwise_fma(q, t, f32x2_t{1.421413741f, 1.421413741f});
    q = __builtin_elementwise_fma(q, t, f32x2_t{-0.284496736f, -0.284496736f});
    q = __builtin_elementwise_fma(q, t, f32x2_t{0.254829592f, 0.254829592f});
    const f32x2_t zz = z * z * f32x2_t{-1.44269504088896340736f, -1.44269504088896340736f};
    const f32x2_t e = {__builtin_amdgcn_exp2f(zz[0]), __builtin_amdgcn_exp2f(zz[1])};
    const f32x2_t erf_abs = __builtin_elementwise_fma(-(q * t), e, f32x2_t{1.0f, 1.0f});
    const f32x2_t half = {0.5f, 0.5f};
    return __builtin_elementwise_fma(half * ax, erf_abs, half * x);
}

// act: 0 none, 1 exact GELU (erff), 2 tanh GELU, 3 exact GELU through gelu_erf_fast (element-wise kernels in precision mode 1)
__device__ __forceinline__ float apply_act(float x, int act) {
    return act == 1 ? gelu_erf(x) : (act == 2 ? gelu_tanh(x) : (act == 3 ? gelu_erf_fast(x) : x));
}
// two fp32 -> one dword of two bf16, nearest even (gfx950 v_cvt_pk_bf16_f32; no builtin in ROCm 7.2)
__device__ __forceinline__ unsigned pack_bf16_rne(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// exact three-term bf16 split of fp32 values (precision mode bf16x3): x = p0 + p1 + p2 with p0 = bf16(x), p1 = bf16(x - p0),
// p2 = x - p0 - p1 -- both subtractions are exact in fp32 and the last remainder fits bf16's 8 significant bits.
// Four values -> one dword pair per plane (element 0 in the low half of dword 0).
using f32x4_t = __attribute__((ext_vector_type(4))) float;
using u32x2_t = __attribute__((ext_vector_type(2))) unsigned;
__device__ __forceinline__ void split3_pack4(const f32x4_t& x, u32x2_t& p0, u32x2_t& p1, u32x2_t& p2) {
    p0[0] = pack_bf16_rne(x[0], x[1]);
    p0[1] = pack_bf16_rne(x[2], x[3]);
    f32x4_t r;
    r[0] = x[0] - __uint_as_float(p0[0] << 16);
    r[1] = x[1] - __uint_as_float(p0[0] & 0xffff0000u);
    r[2] = x[2] - __uint_as_float(p0[1] << 16);
    r[3] = x[3] - __uint_as_float(p0[1] & 0xffff0000u);
    p1[0] = pack_bf16_rne(r[0], r[1]);
    p1[1] = pack_bf16_rne(r[2], r[3]);
    r[0] -= __uint_as_float(p1[0] << 16);
    r[1] -= __uint_as_float(p1[0] & 0xffff0000u);
    r[2] -= __uint_as_float(p1[1] << 16);
    r[3] -= __uint_as_float(p1[1] & 0xffff0000u);
    p2[0] = pack_bf16_rne(r[0], r[1]);
    p2[1] = pack_bf16_rne(r[2], r[3]);
}
// one value -> its three bf16 bit patterns
__device__ __forceinline__ void split3_one(float x, uint16_t& p0, uint16_t& p1, uint16_t& p2) {
    const unsigned h0 = pack_bf16_rne(x, 0.f) & 0xffffu;
    const float r1 = x - __uint_as_float(h0 << 16);
    const unsigned h1 = pack_bf16_rne(r1, 0.f) & 0xffffu;
    const float r2 = r1 - __uint_as_float(h1 << 16);
    p0 = (uint16_t)h0;
    p1 = (uint16_t)h1;
    p2 = (uint16_t)(pack_bf16_rne(r2, 0.f) & 0xffffu);
}
// ---- precision mode f16x2: fp32 values as TWO fp16 terms of x S (S a power of two): h0 = fp16(x S), h1 = fp16(x S - h0); the
// subtraction is exact and h0 + h1 carries 22 significant bits of x S (fp16 keeps its subnormals on gfx950, in the conversion and in
// the MFMA -- tools/mfma_power_probe.hip -- so below |x S| = 2^-3 the error is absolute, <= 2^-25).  A product keeps a0 b0 + a0 b1 +
// a1 b0: three MFMA products instead of bf16x3's six, at an error of ~2^-22 per product, which after K >= 64 products is below what
// the fp32 accumulation itself commits (gemm_split_sw.hip).  |x S| > 65504 saturates; the producers report it (`ovf`).
constexpr float F16X2_ACT_SCALE = 16.0f;       // activations: full precision for 2^-7 <= |x| < 4094
constexpr float F16X2_MAX = 65504.0f;
using h2_t = __attribute__((ext_vector_type(2))) _Float16;
__device__ __forceinline__ unsigned pack_f16_rne(float lo, float hi) {
    const h2_t v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void split2h_pack4(const f32x4_t& x, float s, u32x2_t& p0, u32x2_t& p1, bool& ovf) {
    f32x4_t y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float t = x[i] * s;
        ovf |= !(fabsf(t) <= F16X2_MAX);
        y[i] = __builtin_amdgcn_fmed3f(t, -F16X2_MAX, F16X2_MAX);
    }
    const h2_t a = {(_Float16)y[0], (_Float16)y[1]}, b = {(_Float16)y[2], (_Float16)y[3]};
    p0[0] = __builtin_bit_cast(unsigned, a);
    p0[1] = __builtin_bit_cast(unsigned, b);
    p1[0] = pack_f16_rne(y[0] - (float)a[0], y[1] - (float)a[1]);
    p1[1] = pack_f16_rne(y[2] - (float)b[0], y[3] - (float)b[1]);
}
__device__ __forceinline__ void split2h_one(float x, float s, uint16_t& p0, uint16_t& p1, bool& ovf) {
    const float t = x * s;
    ovf |= !(fabsf(t) <= F16X2_MAX);
    const float y = __builtin_amdgcn_fmed3f(t, -F16X2_MAX, F16X2_MAX);
    const _Float16 h = (_Float16)y;
    p0 = __builtin_bit_cast(uint16_t, h);
    p1 = __builtin_bit_cast(uint16_t, (_Float16)(y - (float)h));
}
// four values -> their planes at p, p + plane, (p + 2 plane); `ovf` only moves in the fp16 format
__device__ __forceinline__ void store_planes4(uint16_t* __restrict__ p, int64_t plane, int fmt, const f32x4_t& v, bool& ovf) {
    u32x2_t p0, p1, p2;
    if (fmt == PF_F16X2) {
        split2h_pack4(v, F16X2_ACT_SCALE, p0, p1, ovf);
        *reinterpret_cast<u32x2_t*>(p) = p0;
        *reinterpret_cast<u32x2_t*>(p + plane) = p1;
    } else {
        split3_pack4(v, p0, p1, p2);
        *reinterpret_cast<u32x2_t*>(p) = p0;
        *reinterpret_cast<u32x2_t*>(p + plane) = p1;
        *reinterpret_cast<u32x2_t*>(p + 2 * plane) = p2;
    }
}
// a producer's end: lanes that saw a saturated value set the sticky flag (range_flag: int in device memory, may be null)
__device__ __forceinline__ void report_overflow(int* range_flag, bool ovf) {
    if (range_flag && ovf) atomicOr(range_flag, 1);      // (exceptional: no need to elect one lane)
}
// wave64 all-reduce sum via DPP/shuffles
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
#endif

}  // namespace w2v2
