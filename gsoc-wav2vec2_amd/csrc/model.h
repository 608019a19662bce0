// Model state and the forward plan shared by the C ABI (w2v2_api.hip), the inference forward (forward.hip) and training
// (w2v2_train.hip).
#pragma once

#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

struct Param {
    std::string name;
    std::vector<int64_t> shape;
    int64_t numel = 0;
    float* dev = nullptr;
    bool set = false;
};
struct Act {
    float* ptr;
    int64_t shape[3];
};

struct w2v2_model {
    w2v2_config cfg;
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;
    // derived tensors (w2v2_finalize)
    float* pos_wg = nullptr;                 // (groups, K, cg, og)
    std::vector<float*> qkv_w, qkv_b;        // per layer (H, 3H), (3H)
    bool finalized = false;
    int precision = 0;                       // 0 fp32 MFMA, 1 bf16 operands / fp32 accumulate (w2v2_set_precision)
    bool opt_shadows = true, opt_keep_acts = false;      // w2v2_set_option
    // activation workspace
    int ws_B = 0;
    int64_t ws_L = 0;
    std::vector<void*> allocs;
    std::map<std::string, Act> acts;
    std::vector<std::string> acts_skipped;   // stage outputs the LAST forward wrote only as bf16 (precision mode 1): no fp32 copy to read back
    std::vector<float*> conv;                // conv stack outputs
    std::vector<int> conv_T;
    float *conv0_ws = nullptr, *ln512 = nullptr, *proj = nullptr, *posout = nullptr;
    std::vector<float*> hs;                  // hidden states: encoder_in, layer0..N-1
    float *qkv = nullptr, *ctx = nullptr, *t0 = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr,
          *ffn = nullptr, *enc_out = nullptr;
    int32_t* frame_len = nullptr;
    // packed variable-length forward (w2v2_forward_packed): stream buffers allocated with a B = 1 workspace of ws_L samples
    int64_t pk_L = 0;                        // ws_L the stream buffers were sized for (0: none)
    int pk_seg_cap = 0, pk_tile_cap = 0;
    float *pk_wave = nullptr, *pk_scale = nullptr, *pk_out = nullptr;   // stream samples, conv0 scale / shift per utterance, head output
    void* pk_tab = nullptr;                  // device tables: PackSeg[pk_seg_cap] | SegTile[pk_tile_cap]
    double* pk_gram = nullptr;               // Gram partials of conv0's GroupNorm statistics per window (w2v2_forward_windows)
    double* pk_stats = nullptr;              // (pk_seg_cap, 2) mean, sqrt(var + eps) per window (w2v2_forward_windows, normalize)
    w2v2::PinnedStage pk_stage;              // pinned staging of the tables (outlives the workspace)
    // bf16 shadows (precision mode 1, inference forward; forward.hip::w2v2_ensure_shadows).  Weight shadows are the
    // GEMM kernels transposed to (N, K); activation shadows are written by the producing kernels.
    bool sh_ready = false, w16_valid = false;
    std::unordered_map<const float*, uint16_t*> w16;      // (N, K): forward GEMMs
    std::unordered_map<const float*, uint16_t*> w16p;     // plain (K, N) bf16 copy = the (N, K) shadow of W^T: dX GEMMs
    std::vector<void*> sh_allocs, w16_allocs;
    w2v2::ShadowJob* shadow_jobs = nullptr;               // device table of the single-launch weight-shadow refresh
    int shadow_njobs = 0;
    bool shadow_jobs_train = false;                       // the table includes the plain copies (built after training state existed)
    std::vector<uint16_t*> conv16, hs16;
    uint16_t *qkv16 = nullptr;                            // q|k|v as the bf16 attention kernels read it (the fp32 copy is then not written)
    uint16_t *ln512_16 = nullptr, *ctx16 = nullptr, *t0_16 = nullptr, *t2_16 = nullptr, *ffn16 = nullptr, *enc16 = nullptr;
    // bf16 positional conv (precision mode 1; posconv.hip): kernel shadow (groups, og, K cg), pack scratch (B, G, T+K-1, cg)
    uint16_t *pos_w16 = nullptr, *pos_pack16 = nullptr;
    bool pos16_valid = false;
    // precision mode 2 (gemm_split.hip): three (N, K) bf16 planes per GEMM weight, built on first use, rebuilt after finalize
    struct SplitPlanes { uint16_t* p = nullptr; int64_t elems = 0; uint64_t epoch = 0; };
    std::unordered_map<const float*, SplitPlanes> w48;     // keyed by the fp32 matrix (a variable, or a transposed copy)
    uint64_t w48_epoch = 1;                                 // bumped whenever the variables change: entries re-split lazily
    // precision modes 2 / 3 on the plane-fed GEMM (gemm_split_sw.hip; forward.hip::w2v2_ensure_planes): the planes of every GEMM
    // operand, written by its producer (three bf16 planes or two fp16 planes per element: PlaneFmt), and the weights as that kernel's
    // LDS images, built on first use and re-split lazily after the variables change (w48_epoch).  Stream order lets one buffer serve
    // every layer: attention input | ctx | FFN input | FFN hidden.
    struct PlaneBuf { uint16_t* p = nullptr; int64_t plane = 0; };
    bool opt_planes = true;                                  // W2V2_OPT_SPLIT_PLANES
    bool opt_wgrad_stream = false;                           // W2V2_OPT_WGRAD_STREAM
    bool opt_defer_folds = true;                             // W2V2_OPT_DEFER_FOLDS
    bool opt_bf16_packed = false;                            // W2V2_OPT_BF16_PACKED
    int pl_fmt = -1, pl_B = 0;
    int64_t pl_L = 0;
    std::vector<void*> pl_allocs;
    std::vector<PlaneBuf> conv48;                            // conv-stack outputs 0 .. NC-2
    PlaneBuf ln512_48, attn_in48, ctx48, ffn_in48, ffn48;
    int* range_flag = nullptr;                               // sticky fp16 saturation flag (device)
    struct SplitImages { uint16_t* img = nullptr; float* scale_ws = nullptr; int64_t elems = 0; uint64_t epoch = 0; };
    std::unordered_map<const float*, SplitImages> wimg[2];   // [PlaneFmt], keyed by the fp32 matrix
    w2v2::Profiler* prof = nullptr;
    struct TrainState* train = nullptr;      // owned by w2v2_train.hip (null until the first training call)
    struct Comm* comm = nullptr;             // owned by comm.hip: the native RCCL communicator (null until w2v2_comm_init)

    float* P(const std::string& n) const {
        auto it = index.find(n);
        return it == index.end() ? nullptr : params[it->second].dev;
    }
};


// ---- the forward plan (forward.hip; the table of every tensor's forms is in DESIGN.md, "The forward plan") ------------------------
// where a producer leaves the planes of its output; converts to the launchers' optional `const PlaneOut*` (null = none)
struct PlaneDst {
    w2v2::PlaneOut o;
    bool on = false;
    operator const w2v2::PlaneOut*() const { return on ? &o : nullptr; }
};

struct ForwardPlan {
    using PlaneBuf = w2v2_model::PlaneBuf;
    // The forms a tensor can be stored in.  Which of them a forward writes is decided ONCE, in w2v2_plan_forward, before the first
    // launch: producers take their destinations and consumers their sources from the same field, through the helpers below.
    enum Form : unsigned { F32 = 1, B16 = 2 /* nearest-even bf16 shadow (precision mode bf16) */, PLANES = 4 /* operand planes (bf16x3 / f16x2) */ };
    // sizes and modes
    int B = 0, T = 0, NC = 0;
    int64_t L = 0, BT = 0;
    std::vector<int> conv_T;                 // frames per conv layer for THIS input (a packed stream runs in a larger workspace)
    bool sh = false, attn16 = false;         // precision mode bf16 with shadows; ... and the bf16 attention kernels (q|k|v, ctx as bf16)
    bool pm = false;                         // precision modes bf16x3 / f16x2 with operand planes
    int fmt = w2v2::PF_BF16X3;
    bool keep = false;                       // W2V2_OPT_KEEP_ACTIVATIONS
    bool layer_mode = false, prenorm = false;
    int act = 1, act_ew = 1;                 // GELU form of the GEMM epilogues / of the element-wise kernels
    bool fused = false;                      // conv0's kernel writes the planes of its output itself
    w2v2::AttnRoute attn;                    // the attention kernel of this forward (attention_route.h), dense or packed
    bool split_attn = false;                 // ... is the split kernel
    bool ctx_fused = false;                  // ... and writes ctx's planes itself
    bool ctx16_only = false, ffn_sh_only = false;      // mode bf16: ctx / the FFN hidden exist only as bf16 (both ignore `keep`)
    bool pos16 = false;                      // the bf16 positional conv (needs w2v2_ensure_pos16)
    // plane-fed GEMM call sites: cp[i] = conv layer i's GEMM (1 .. NC-1) streams the planes of conv output i - 1
    std::vector<char> cp;
    bool p_proj = false, p_qkv = false, p_out = false, p_f1 = false, p_f2 = false, any_planes = false;
    // forms written in this forward, per tensor.  conv[i] is the value behind LN + GELU in LayerNorm mode; conv0_kernel / attn_kernel
    // are the forms those two kernels write themselves (the planes of conv[0] / ctx are otherwise split off the fp32 copy behind them)
    std::vector<unsigned> conv;
    unsigned conv0_kernel = F32, ln512 = F32, proj = F32, hidden = F32, attn_in = F32, qkv = F32, ctx = F32, attn_kernel = F32,
             ffn_in = F32, ffn = F32, head_in = F32;

    // the GEMM behind conv layer i writes conv[i] itself, or (LayerNorm mode) the fp32 input of the LN + GELU pass that does
    unsigned conv_gemm_out(int i) const { return layer_mode ? (unsigned)F32 : conv[i]; }
    // a producer's destinations / a consumer's sources: the buffer when the form is written in this forward, else null
    static float* f32(unsigned forms, float* p) { return (forms & F32) ? p : nullptr; }
    static uint16_t* b16(unsigned forms, uint16_t* p) { return (forms & B16) ? p : nullptr; }
    static uint16_t* b16(unsigned forms, const std::vector<uint16_t*>& v, int i) { return (forms & B16) ? v[i] : nullptr; }
    static const PlaneBuf* planes(unsigned forms, const PlaneBuf& b) { return (forms & PLANES) ? &b : nullptr; }
    static const PlaneBuf* planes(unsigned forms, const std::vector<PlaneBuf>& v, int i) { return (forms & PLANES) ? &v[i] : nullptr; }
    PlaneDst plane_out(const PlaneBuf* b, int* range_flag) const {
        PlaneDst d;
        if (b) { d.o.p = b->p; d.o.plane = b->plane; d.o.fmt = fmt; d.o.range_flag = range_flag; d.on = true; }
        return d;
    }
};
struct PackedPlan;      // forward.hip: the tables of a packed stream

// ---- the training plan (w2v2_train.hip::plan_train; DESIGN.md, "The training plan") -------------------------------------------------
// What a training forward decided, once, before its first launch.  The forward runs from it, the workspace is built for it, and the
// backward takes every mode-dependent decision from the copy TrainState keeps -- never from the model's settings at backward time.
struct TrainPlan {
    int precision = 0;                       // the mode and the shadow option the forward ran with: the backward refuses any other
    bool opt_shadows = false;
    int B = 0, T = 0;
    int64_t BT = 0;
    bool sh = false, attn16 = false;         // mode bf16 with shadows; ... and the bf16 attention kernels (q|k|v kept as bf16 only)
    // kept as bf16 only (no fp32 copy written): dropout(GELU(u)); u (in the first half of its buffer); the attention output; prenorm: a, t2
    bool ffn16_only = false, u16_only = false, ctx16_only = false, ln16_only = false;
    bool lean_ws = true;                     // the fp32 buffers of the above are not even allocated (tools-only knob W2V2_LEAN_WS)
    bool prenorm = false;
    int act = 1, act_ew = 1;                 // GELU form of the GEMM epilogues / of the element-wise kernels
    int u_round = 0;                         // the element-wise kernels round an fp32 u to bf16 on the way in (mode bf16)
    bool lse_log2 = false;                   // the attention forward saved lse2 = -(m C2 + log2 l) (bf16 kernels), not the natural lse
    w2v2::AttnRoute attn, attn_bwd;          // the attention kernels of the step (attention_route.h): attn16 and lse_log2 are read off them
};

// implemented in w2v2_api.hip
int w2v2_ensure_workspace(w2v2_model* m, int B, int64_t L);
int w2v2_ws_alloc(w2v2_model* m, float** out, int64_t floats);           // a buffer that lives as long as the workspace
void w2v2_free_planes(w2v2_model* m);
// implemented in forward.hip
// conv-stack output i (behind LN + GELU in LayerNorm mode) is written only as bf16: shadows on, no `keep`, and layer i + 1's GEMM streams the shadow
bool w2v2_conv_bf16_only(const w2v2_model* m, int i, bool sh);
// the plan of a forward over (B, L) in the model's precision mode and options; `planes` false (training) keeps every GEMM off the plane-fed route.
// Needs the workspace (w2v2_ensure_workspace) in place.
ForwardPlan w2v2_plan_forward(const w2v2_model* m, int B, int64_t L, bool planes, bool packed);
// conv0, conv 1 .. NC-1, the projection LayerNorm and the projection GEMM (-> m->proj) as the plan says; sets m->acts_skipped.  pk: the packed stream, or null
int w2v2_forward_frontend(w2v2_model* m, const ForwardPlan& plan, const float* wave, const PackedPlan* pk, hipStream_t s);
int w2v2_ensure_shadows(w2v2_model* m, int B, int T, hipStream_t s);      // allocate activation shadows, (re)build weight shadows
bool w2v2_pos_conv_bf16_ok(const w2v2_model* m);                          // precision 1 and a supported group shape
int w2v2_ensure_pos16(w2v2_model* m, int B, int T, hipStream_t s);        // kernel shadow + pack scratch
// precision mode 2: the LDS-image bf16 planes of the (K, N) fp32 matrix `W` (built / refreshed on demand; gemm_split.hip)
int w2v2_split_planes(w2v2_model* m, const float* W, int K, int N, hipStream_t s, const uint16_t** planes);
// whether GEMM (M, N, K) x nbatch with this A should take the split kernel in the model's current precision mode
bool w2v2_use_split_gemm(const w2v2_model* m, const float* A, int64_t lda, int64_t strideA, int64_t ldb, int M, int N, int K, int nbatch);
// a GEMM that is not plane-fed, on the mode's route (six-product split / fp32 / bf16 with shadows when `sh`); null = form not written
int w2v2_gemm_route(w2v2_model* m, bool sh, hipStream_t s, const float* A, const uint16_t* A16, int64_t lda, int64_t strideA, const float* Bw,
                    int64_t ldb, float* Cc, uint16_t* C16, int64_t ldc, int64_t strideC, const float* bias, const float* res, int M, int N, int K,
                    int nbatch, int act_);
// precision modes 2 / 3 with W2V2_OPT_SPLIT_PLANES: the plane buffers of a (B, L) forward in the mode's format; the LDS images (and,
// f16x2, the accumulator scale) of the (K, N) fp32 matrix W
int w2v2_ensure_planes(w2v2_model* m, int B, int64_t L, int fmt);
int w2v2_split_images(w2v2_model* m, const float* W, int K, int N, int fmt, hipStream_t s, const uint16_t** img, const float** out_scale);
// implemented in w2v2_train.hip
void w2v2_train_destroy(w2v2_model* m);
void w2v2_train_invalidate(w2v2_model* m);
// the contiguous runs of TRAINABLE slots (offset, numel; 16-byte aligned slots merge) inside gradient bucket k, and the flat buffer
int w2v2_train_trainable_runs(w2v2_model* m, int k, std::vector<std::pair<int64_t, int64_t>>* runs, float** grads);
// implemented in comm.hip
void w2v2_comm_free(w2v2_model* m);
