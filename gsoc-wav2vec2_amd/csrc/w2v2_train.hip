// Training step of the CTC fine-tuning path: training-mode forward, backward, Adam.
//
// What the reference does inside Keras' train_step (src/main.py:136-259):
//   forward with training=True  -- dropout at every Dropout layer, spec-augment on the projected
//     features (modeling.py:193-199), StochasticDepth on the FFN branch (encoder.py:130);
//   CTC loss / global batch (losses.py:45, main.py:198-200);
//   gradients of every trainable variable -- stage 2 freezes the 7 conv layers (main.py:234-237),
//     stage 1 trains lm_head only (main.py:210);
//   Adam (Keras defaults) and, under MirroredStrategy, a SUM all-reduce of the gradients.
// Here: w2v2_train_forward -> (caller: w2v2_ctc_loss gives d nll / d logits) -> w2v2_train_backward
// fills one flat gradient buffer (the all-reduce payload) -> w2v2_adam_step.
//
// Heavy contractions reuse the forward's fp32 MFMA GEMM:
//   dX = dY W^T   uses transposed copies of the kernels kept next to the variables;
//   dW = X^T dY   transposes the activation once and runs a split-K batched GEMM into slabs that a
//                 reduction kernel sums (deterministic: no atomics anywhere in the backward).
// The conv feature extractor has no backward: the reference never trains it in this path.
#include <string.h>

#include "model.h"
#include "train.h"

using namespace w2v2;

struct LayerSave {
    float *qkv, *ctx, *lse, *t1, *t2, *u, *gd, *t3;
    float* a;                           // prenorm only: LN(x), the attention input
    float *WqkvT, *WoT, *W1T, *W2T;     // transposed kernels for the data-gradient GEMMs
    float keep;                         // stochastic-depth draw of the last forward
    // precision mode 1: bf16 shadows of the activations the weight-gradient GEMMs contract with (dW = X^T dY reads X as a
    // transposed A).  Written by the forward's producers like the shared shadows, but kept per layer until the backward.
    uint16_t *a16 = nullptr, *ctx16 = nullptr, *t2_16 = nullptr, *gd16 = nullptr, *qkv16 = nullptr;
    uint32_t* keep_bits = nullptr;       // attention-probability dropout decisions of the forward (bf16 attention kernels)
};

struct TrainState {
    int B = 0, T = 0;
    int64_t L = 0;
    // The plan the shape-dependent buffers were built for (ensure_train_ws) and, once `forward_done`, the plan of the completed forward
    // the backward differentiates.  The two agree in everything the buffers depend on: a forward whose plan needs other buffers rebuilds.
    TrainPlan plan;
    int64_t alloc_bytes = 0;            // bytes behind `allocs`
    std::vector<void*> allocs;          // shape-dependent buffers: rebuilt when (B, L) changes
    std::vector<void*> persist;         // shape-independent buffers (gradients, Adam moments, transposed kernels, slab scratch):
                                        // allocated once -- their addresses key the bf16x3 plane cache (w2v2_model::w48)
    std::vector<LayerSave> layers;
    float *hd = nullptr, *hm = nullptr, *pos_c = nullptr, *hdf = nullptr, *hs0 = nullptr;
    float *WpT = nullptr, *WlmT = nullptr, *pos_wg_t = nullptr, *dwg = nullptr;
    float *pos_pack32 = nullptr, *pos_dw_slabs = nullptr, *pos_dc_pad = nullptr;   // scratch of the GEMM-formulated positional-conv kernel gradient
    uint16_t* pos_w16_t = nullptr;           // bf16 (groups, og, K cg) shadow of pos_wg_t (precision mode 1); follows transposes_fresh
    bool pos_w16_t_fresh = false;
    uint8_t* spec_mask = nullptr;       // (B*T) device copy, or null when not applied
    bool have_spec = false, have_mask = false;
    uint64_t trainable_sig = 0;           // signature of `trainable` at the last backward (0: none yet -> the buffer is cleared)
    bool grads_need_clear = false;
    float p = 0.f;
    uint64_t seed = 0;
    // gradient / optimizer state: flat, inventory order
    float *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    AdamChunk* adam_chunks = nullptr;        // device table for the single-launch Adam; rebuilt when `trainable` changes
    int adam_nchunks = 0;
    bool adam_table_fresh = false;
    // accumulation, clipping, AdamW, skipped steps: every buffer below is allocated by the first call that needs it
    std::vector<char> decay;                 // per variable: takes the decoupled weight decay (w2v2_set_decay_flags); empty = none
    float* grad_acc = nullptr;               // gtotal floats: the micro-step sum of w2v2_grad_accumulate
    double* norm_partial = nullptr;          // norm_cap doubles, then norm_cap int32 flags: grad_sumsq's output per chunk
    int norm_cap = 0;
    OptStats* opt_stats = nullptr;           // the device-resident record w2v2_grad_norm writes and w2v2_adamw_step reads
    bool norm_fresh = false;                 // a w2v2_grad_norm has run since the last backward / accumulate-finish
    std::vector<int64_t> goff;
    int64_t gtotal = 0;
    std::vector<char> trainable;
    bool transposes_fresh = false;
    bool transposes_full = false;            // the per-layer fp32 transposed kernels are current (not needed in bf16 mode)
    // scratch
    float *gh[4] = {nullptr, nullptr, nullptr, nullptr}, *gf = nullptr, *g3h = nullptr, *at = nullptr,
          *slabs = nullptr, *red_ws = nullptr, *dvec = nullptr, *dummy = nullptr, *dwqkv = nullptr, *dwv_scratch = nullptr,
          *attn_colpart = nullptr;     // per-block column sums of dqkv from the bf16 attention backward (-> q|k|v bias gradient)
    int64_t slab_floats = 0;
    // bf16 shadows of the gradient tensors that are the A operand of a data-gradient GEMM (precision mode 1): written by the
    // producing kernel (LayerNorm / dropout / attention backward), consumed by the GEMM enqueued right behind it
    uint16_t *dy16_h = nullptr, *dy16_f = nullptr, *dy16_3h = nullptr, *dy16_ctx = nullptr;
    float* cs_ws = nullptr;           // (slabs + 1, widest N): per-slab column sums of dY from the weight-gradient GEMM
    int64_t cs_floats = 0;
    bool forward_done = false;                    // a completed training forward stands behind `plan` and the saved activations
    // gradient buckets for overlapping the data-parallel all-reduce with the backward: completion order
    //   0 = lm_head, 1 .. N = encoder layers N-1 .. 0, N+1 = everything in front of layer 0 in the flat buffer
    std::vector<hipEvent_t> bucket_ev;
    // Weight-gradient side stream (round 5, W2V2_OPT_WGRAD_STREAM, default OFF).  dW = X^T dY is off the backward's critical path --
    // only the optimizer (and the bucket's all-reduce) reads it -- so the encoder layers' four weight-gradient GEMMs (+ their slab
    // folds) can be enqueued on a second, lower-priority stream, to fill what the critical path leaves idle: the underfilled last
    // round of every N = 768 data-gradient GEMM (576 tiles on 512 block slots), the matrix pipe under the VALU-bound attention
    // backward, the HBM-bound element-wise passes.  MEASURED (profiles/r05_ab_wgrad_stream.txt): the kernels do overlap -- every
    // family's event brackets stretch -- and the step time does not move (33.38 vs 33.39 ms base, 97.7 vs 98.0 large-robust): the
    // chip is a shared-throughput machine here (clock 1.98 GHz under the bf16 GEMMs: power; HBM under the element-wise passes), not a
    // slot-limited one.  Kept as an option because the all-reduce overlap of an 8-GPU job may still want the earlier buckets; off by
    // default.  Ordering is by events only: `wg_fork` (main -> side: the dY the GEMM reads is complete), `wg_join[site]` (side -> main,
    // waited for right before the main stream next overwrites that site's dY), and the bucket events are recorded on the side stream
    // after it has also waited for the main stream's position.  Same kernels, same operands: results are bit-identical to one stream.
    hipStream_t wg_stream = nullptr;
    hipEvent_t wg_fork = nullptr, wg_main = nullptr, wg_join[4] = {nullptr, nullptr, nullptr, nullptr};
    float* red_ws_side = nullptr;     // the side stream's own reduction scratch (red_ws belongs to the main stream's kernels)
    // Deferred folds (train.h: FoldBatch): the partial rows of a layer's gradients live until the layer's one fold launch, so each
    // deferred producer has its own scratch -- split-K slabs of the four weight gradients (0 = FFN down, 1 = FFN up, 2 = out-projection,
    // 3 = q|k|v; wg_max_slabs + 1 slabs of the kernel's size each: ensure_site_scratch) and the per-block column sums of LayerNorm 2 / the FFN
    // dropout backward / LayerNorm 1 (site_ws).  The attention backward's column partials already have theirs (attn_colpart).
    float* site_slabs[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t site_slab_floats[4] = {0, 0, 0, 0};
    float* site_ws[3] = {nullptr, nullptr, nullptr};
    int64_t red_ws_floats = 0;        // size of red_ws (and of each of red_ws_side / site_ws[k] once they exist)
};

static int t_alloc(TrainState* t, float** out, int64_t floats) {
    void* p = nullptr;
    W2V2_HIP_CHECK(hipMalloc(&p, (size_t)(floats > 0 ? floats : 1) * sizeof(float)));
    t->allocs.push_back(p);
    t->alloc_bytes += (floats > 0 ? floats : 1) * (int64_t)sizeof(float);
    *out = reinterpret_cast<float*>(p);
    return W2V2_OK;
}

static int p_alloc(TrainState* t, float** out, int64_t floats) {
    void* p = nullptr;
    W2V2_HIP_CHECK(hipMalloc(&p, (size_t)(floats > 0 ? floats : 1) * sizeof(float)));
    t->persist.push_back(p);
    *out = reinterpret_cast<float*>(p);
    return W2V2_OK;
}

static void t_free(TrainState* t) {
    for (void* p : t->allocs) (void)hipFree(p);
    t->allocs.clear();
    t->alloc_bytes = 0;
}

void w2v2_train_destroy(w2v2_model* m) {
    if (!m || !m->train) return;
    t_free(m->train);
    for (void* p : m->train->persist) (void)hipFree(p);
    m->train->persist.clear();
    if (m->train->adam_chunks) (void)hipFree(m->train->adam_chunks);
    for (void* p : {(void*)m->train->grad_acc, (void*)m->train->norm_partial, (void*)m->train->opt_stats})
        if (p) (void)hipFree(p);
    if (m->train->pos_w16_t) (void)hipFree(m->train->pos_w16_t);
    for (hipEvent_t ev : m->train->bucket_ev) (void)hipEventDestroy(ev);
    if (m->train->wg_stream) (void)hipStreamDestroy(m->train->wg_stream);
    for (hipEvent_t ev : {m->train->wg_fork, m->train->wg_main, m->train->wg_join[0], m->train->wg_join[1], m->train->wg_join[2], m->train->wg_join[3]})
        if (ev) (void)hipEventDestroy(ev);
    delete m->train;
    m->train = nullptr;
}

// a variable changed outside the optimizer (w2v2_set_param): the transposed kernel copies are stale
void w2v2_train_invalidate(w2v2_model* m) {
    if (m && m->train) m->train->transposes_fresh = false;
}

static TrainState* get_state(w2v2_model* m) {
    if (!m->train) {
        TrainState* t = new TrainState();
        t->trainable.assign(m->params.size(), 1);
        // flat gradient layout = inventory order
        t->goff.resize(m->params.size());
        int64_t off = 0;
        for (size_t i = 0; i < m->params.size(); ++i) {
            t->goff[i] = off;
            off += (m->params[i].numel + 3) & ~(int64_t)3;     // 16-byte aligned slots
        }
        t->gtotal = off;
        m->train = t;
    }
    return m->train;
}

// Shape-independent state, once per model: gradients, Adam moments, transposed kernel copies, slab scratch.  The transposed
// copies must keep their addresses across shape changes: the bf16x3 plane cache is keyed by them, and a freed-and-recycled
// address would serve stale planes.
static int ensure_persistent(w2v2_model* m) {
    TrainState* t = get_state(m);
    const w2v2_config& c = m->cfg;
    const int64_t H = c.hidden_size, F = c.intermediate_size;
    const int64_t C = c.filter_sizes[c.num_conv_layers - 1];
    const int64_t K = c.num_conv_pos_embeddings, cg = H / c.num_conv_pos_embedding_groups;
    if (!t->grads) {
        if (int e = p_alloc(t, &t->grads, t->gtotal)) return e;
        if (int e = p_alloc(t, &t->adam_m, t->gtotal)) return e;
        if (int e = p_alloc(t, &t->adam_v, t->gtotal)) return e;
        W2V2_HIP_CHECK(hipMemset(t->grads, 0, (size_t)t->gtotal * 4));
        W2V2_HIP_CHECK(hipMemset(t->adam_m, 0, (size_t)t->gtotal * 4));
        W2V2_HIP_CHECK(hipMemset(t->adam_v, 0, (size_t)t->gtotal * 4));
        if (int e = p_alloc(t, &t->WpT, H * C)) return e;
        if (int e = p_alloc(t, &t->WlmT, H * (int64_t)c.vocab_size)) return e;
        if (int e = p_alloc(t, &t->pos_wg_t, K * cg * H)) return e;
        if (int e = p_alloc(t, &t->dwg, K * cg * H)) return e;
        if (int e = p_alloc(t, &t->dwv_scratch, K * cg * H)) return e;
        t->layers.resize(c.num_layers);
        for (auto& l : t->layers) {
            if (int e = p_alloc(t, &l.WqkvT, 3 * H * H)) return e;
            if (int e = p_alloc(t, &l.WoT, H * H)) return e;
            if (int e = p_alloc(t, &l.W1T, F * H)) return e;
            if (int e = p_alloc(t, &l.W2T, H * F)) return e;
            l.keep = 1.f;
        }
        t->slab_floats = WG_MAX_SLABS * (F * H > 3 * H * H ? F * H : 3 * H * H);      // 32 split-K slabs + the reduction scratch
        if (int e = p_alloc(t, &t->slabs, t->slab_floats)) return e;
        // (the per-site slab scratches of the deferred folds are allocated by the first backward that defers: ensure_site_scratch)
        t->cs_floats = (WG_MAX_SLABS + 1) * (F > 3 * H ? F : 3 * H);
        if (int e = p_alloc(t, &t->cs_ws, t->cs_floats)) return e;
        if (int e = p_alloc(t, &t->dwqkv, 3 * H * H + 3 * H)) return e;
        if (int e = p_alloc(t, &t->dummy, 2 * (H + C + F))) return e;       // sink for gradients of frozen LN params
        t->transposes_fresh = false;
    }
    return W2V2_OK;
}

// Scratch that only some backward configurations use, allocated the first time one of them runs (it used to be allocated
// for every model -- fp32 training, W2V2_OPT_DEFER_FOLDS = 0 and the side-stream mode included): the side stream's reduction scratch,
// the deferred folds' per-site partial rows (shape-dependent: freed with the workspace) and per-site split-K slabs (persistent).
static int ensure_site_scratch(w2v2_model* m, bool side, bool defer_cols, bool defer_slabs) {
    TrainState* t = m->train;
    if (side && !t->red_ws_side)
        if (int e = t_alloc(t, &t->red_ws_side, t->red_ws_floats)) return e;
    if (defer_cols && !t->site_ws[0])
        for (int k = 0; k < 3; ++k)
            if (int e = t_alloc(t, &t->site_ws[k], t->red_ws_floats)) return e;
    if (defer_slabs && !t->site_slabs[0]) {
        const int64_t H = m->cfg.hidden_size, F = m->cfg.intermediate_size;
        const int64_t site_dims[4][2] = {{F, H}, {H, F}, {H, H}, {H, 3 * H}};
        for (int k = 0; k < 4; ++k) {
            // (+ 1: the fold's partial scratch behind the slabs -- the plan's `nslabs + 1`)
            t->site_slab_floats[k] = (wg_max_slabs(site_dims[k][0], site_dims[k][1]) + 1) * site_dims[k][0] * site_dims[k][1];
            if (int e = p_alloc(t, &t->site_slabs[k], t->site_slab_floats[k])) return e;
        }
    }
    return W2V2_OK;
}

// `lean`: which per-layer fp32 activations the coming forward will NOT write (precision mode 1 on the shadow paths keeps q|k|v, the
// attention output and the FFN hidden activation only as bf16, and u as bf16 in half of its buffer): they are not allocated -- 0.75 GB
// per layer at 32 x 246000, 9 GB for base and 24 GB for large at 16 x 480000 (rounds 2-4 allocated them regardless).  A forward that
// needs a different set (the precision or the shadow option changed on the same shapes) rebuilds the workspace.
// LEAN_LN (prenorm only): the outputs of the two LayerNorms inside a layer feed nothing but GEMMs -- q|k|v / the FFN up-projection and their
// weight gradients, which all stream the bf16 shadow -- so their fp32 copies (a, t2) are neither written nor allocated.  (Postnorm: t2 is
// also the FFN's residual and stays fp32.)
enum : int { LEAN_QKV = 1, LEAN_CTX = 2, LEAN_GD = 4, LEAN_U_HALF = 8, LEAN_LN = 16 };
static int lean_mask(const TrainPlan& p) {
    if (!p.lean_ws) return 0;
    return (p.attn16 ? LEAN_QKV : 0) | (p.ctx16_only ? LEAN_CTX : 0) | (p.ffn16_only ? LEAN_GD : 0) | (p.u16_only ? LEAN_U_HALF : 0) |
           (p.ln16_only ? LEAN_LN : 0);
}
// the same fact as w2v2_train_storage reports it: what the forward keeps as bf16 only (allocated in fp32 or not)
static int storage_mask(const TrainPlan& p) {
    return (p.attn16 ? W2V2_TRAIN_BF16_QKV : 0) | (p.ctx16_only ? W2V2_TRAIN_BF16_CTX : 0) | (p.ffn16_only ? W2V2_TRAIN_BF16_FFN : 0) |
           (p.u16_only ? W2V2_TRAIN_BF16_U : 0) | (p.ln16_only ? W2V2_TRAIN_BF16_LN : 0);
}

// The plan of a training forward over (B, L): every mode-dependent decision of the step, one line each, here and nowhere else.  Reads
// m->w16_valid and m->w16p, so it runs behind w2v2_ensure_shadows (which refreshes the bf16 weight shadows after an optimizer step).
static TrainPlan plan_train(const w2v2_model* m, int B, int64_t L) {
    const w2v2_config& c = m->cfg;
    const int H = c.hidden_size, F = c.intermediate_size;
    TrainPlan p;
    p.precision = m->precision;
    p.opt_shadows = m->opt_shadows;
    p.B = B;
    p.T = (int)w2v2_num_frames(m, L);
    p.BT = (int64_t)B * p.T;
    p.prenorm = c.attention_norm_type == 1;
    // Mode bf16: the same bf16 shadows as the inference forward (forward.hip).  Every producer of a forward GEMM operand -- conv0, GEMM
    // epilogues, LayerNorm, dropout, attention -- also writes the nearest-even bf16 copy, so the forward GEMMs stream 2-byte operands
    // by LDS-DMA instead of converting fp32 in registers; results are bit-identical either way.
    p.sh = m->precision == 1 && m->opt_shadows;
    // the attention kernels of the step (attention_route.h): the forward and the backward run from these two routes
    p.attn = attention_route(attention_problem(AP_TRAIN, m->precision, B, p.T, H, c.num_heads, false));
    p.attn_bwd = attention_route(attention_problem(AP_BWD, m->precision, B, p.T, H, c.num_heads, false));
    // the bf16 attention kernels (forward and backward) read q | k | v only as bf16: the projection then writes just that shadow
    p.attn16 = p.sh && p.attn.family == AF_BF16;
    // ... and they save lse2 = -(m C2 + log2 l) where the fp32 kernels save the natural lse
    p.lse_log2 = p.attn.lse_log2;
    // FFN hidden activation dropout(GELU(u)) as bf16 only: needs the shadow paths on both sides (forward GEMM by LDS-DMA, weight gradient
    // in the transposing-read form, whole 128-tiles) and the plain bf16 copies of the FFN kernels for the data gradients
    p.ffn16_only = p.sh && m->w16_valid && F % 128 == 0 && H % 128 == 0 && (p.BT * F) % 4 == 0 && !m->w16p.empty();
    // u = t2 W1 + b1 as bf16 only (what a mixed_bfloat16 Dense hands to its activation): the up-projection writes ONLY the bf16 copy (302 MB
    // of fp32 stores per layer gone at B = 32) and GELU + dropout, GELU' in the backward read that ...
    p.u16_only = p.ffn16_only && tune_int("W2V2_U16", 1) != 0;
    // ... while the shadow-free path of the mode rounds the fp32 u on the way into the same kernels, so both agree bit for bit
    p.u_round = m->precision == 1 ? 1 : 0;
    // The attention output O: its readers are the out-projection GEMM and that GEMM's weight gradient (both stream the bf16 shadow) and
    // D = rowsum(dO o O) of the attention backward, which is defined on the bf16 values -- no fp32 copy is written
    p.ctx16_only = p.ffn16_only && p.attn16 && tune_int("W2V2_CTX16", 1) != 0;
    // Prenorm: a = LN1(x) and t2 = LN2(t1) are read only by GEMMs that stream their shadows (the same conditions): written only as bf16
    // (196 MB of fp32 stores per layer gone at 16 x 480000).  Postnorm: t2 is also the FFN's residual and stays fp32
    p.ln16_only = p.prenorm && p.ffn16_only && p.attn16 && tune_int("W2V2_LN16", 1) != 0;
    // (tools-only build: W2V2_LEAN_WS = 0 allocates every fp32 buffer, as rounds 2-4 did, for A/B runs)
    p.lean_ws = tune_int("W2V2_LEAN_WS", 1) != 0;
    p.act = c.is_gelu_approx ? 2 : 1;
    // element-wise kernels in mode bf16 evaluate exact GELU / GELU' through the 5-term erf the bf16 GEMM epilogue uses (act 3)
    p.act_ew = (p.act == 1 && m->precision == 1) ? 3 : p.act;
    return p;
}

static int ensure_train_ws(w2v2_model* m, const TrainPlan& plan, int64_t L) {
    TrainState* t = get_state(m);
    const int B = plan.B, T = plan.T, lean = lean_mask(plan);
    if (t->B == B && t->L == L && t->B > 0 && lean_mask(t->plan) == lean) return W2V2_OK;
    if (int e = ensure_persistent(m)) return e;
    const w2v2_config& c = m->cfg;
    const int64_t H = c.hidden_size, F = c.intermediate_size, BT = (int64_t)B * T;
    const int64_t C = c.filter_sizes[c.num_conv_layers - 1];
    // ---- shape-dependent activations and scratch
    t_free(t);
    t->B = 0;
    t->forward_done = false;
    t->pos_pack32 = t->pos_dw_slabs = t->pos_dc_pad = nullptr;      // lazily re-allocated at the new shape
    if (int e = t_alloc(t, &t->hd, BT * H)) return e;
    if (int e = t_alloc(t, &t->hm, BT * H)) return e;
    if (int e = t_alloc(t, &t->pos_c, BT * H)) return e;
    if (int e = t_alloc(t, &t->hdf, BT * H)) return e;
    t->hs0 = nullptr;
    if (c.attention_norm_type == 1)
        if (int e = t_alloc(t, &t->hs0, BT * H)) return e;
    float* sm = nullptr;
    if (int e = t_alloc(t, &sm, (BT + 15) / 4 + 4)) return e;
    t->spec_mask = reinterpret_cast<uint8_t*>(sm);
    for (auto& l : t->layers) {
        l.qkv = l.ctx = l.gd = nullptr;
        if (!(lean & LEAN_QKV))
            if (int e = t_alloc(t, &l.qkv, BT * 3 * H)) return e;
        if (!(lean & LEAN_CTX))
            if (int e = t_alloc(t, &l.ctx, BT * H)) return e;
        if (int e = t_alloc(t, &l.lse, (int64_t)B * c.num_heads * T)) return e;
        if (int e = t_alloc(t, &l.t1, BT * H)) return e;
        l.t2 = nullptr;
        if (!(lean & LEAN_LN))
            if (int e = t_alloc(t, &l.t2, BT * H)) return e;
        if (int e = t_alloc(t, &l.u, (lean & LEAN_U_HALF) ? (BT * F + 1) / 2 + 4 : BT * F)) return e;
        if (!(lean & LEAN_GD))
            if (int e = t_alloc(t, &l.gd, BT * F)) return e;
        if (int e = t_alloc(t, &l.t3, BT * H)) return e;
        l.a = nullptr;
        if (c.attention_norm_type == 1 && !(lean & LEAN_LN))
            if (int e = t_alloc(t, &l.a, BT * H)) return e;
    }
    {
        // per-layer X shadows: (3 H + F) bf16 per row and layer (base, B = 32: 2.7 GB)
        auto up8 = [](int64_t n) { return (n + 7) & ~(int64_t)7; };
        for (auto& l : t->layers) {
            float* raw = nullptr;
            if (int e = t_alloc(t, &raw, (6 * up8(BT * H) + up8(BT * F)) / 2 + 16)) return e;
            l.a16 = reinterpret_cast<uint16_t*>(raw);
            l.ctx16 = l.a16 + up8(BT * H);
            l.t2_16 = l.ctx16 + up8(BT * H);
            l.gd16 = l.t2_16 + up8(BT * H);
            l.qkv16 = l.gd16 + up8(BT * F);          // q | k | v as the bf16 attention kernels read it
            // (the keep bits and, below, the column partials of the bf16 kernels: allocated wherever those kernels exist for the head size,
            // in every mode -- a step in another mode on the same shapes reuses this workspace)
            float* kb = nullptr;
            if (plan.attn.dh == ATTN_BF16_DH) {
                if (int e = t_alloc(t, &kb, attention_keep_bits_words(B, T, c.num_heads))) return e;
            }
            l.keep_bits = reinterpret_cast<uint32_t*>(kb);
        }
    }
    for (int i = 0; i < 4; ++i)
        if (int e = t_alloc(t, &t->gh[i], BT * H)) return e;
    if (int e = t_alloc(t, &t->gf, BT * F)) return e;
    if (int e = t_alloc(t, &t->g3h, BT * 3 * H)) return e;
    const int64_t widest = F > 3 * H ? F : 3 * H;
    if (int e = t_alloc(t, &t->at, widest * BT)) return e;
    int64_t rw = dropout_bwd_colsum_ws_floats(BT, (int)widest);        // (>= colsum_ws_floats of the same shape)
    const int64_t lw = ln_bwd_ws_floats(BT, (int)(H > C ? H : C));
    if (lw > rw) rw = lw;
    if (int e = t_alloc(t, &t->red_ws, rw + 16)) return e;
    t->red_ws_side = nullptr;                    // (the side stream's scratch and the deferred folds' per-site scratch: allocated by the
    t->site_ws[0] = t->site_ws[1] = t->site_ws[2] = nullptr;      //  first backward that uses them -- ensure_site_scratch)
    t->red_ws_floats = rw + 16;
    if (int e = t_alloc(t, &t->dvec, (int64_t)B * c.num_heads * T)) return e;
    t->attn_colpart = nullptr;
    if (plan.attn.dh == ATTN_BF16_DH)
        if (int e = t_alloc(t, &t->attn_colpart, (int64_t)attention_colpart_rows(B, T) * 3 * H)) return e;
    {
        // (BT + 1, H) + (BT + 1, F) + (BT + 1, 3H) + (BT, H) bf16, each 16-byte aligned.  Row BT of the first three is never written
        // and stays zero: the weight-gradient GEMMs read a short last K tile's missing rows from there (weight_grad: dy16_zero_row).
        float* raw = nullptr;
        auto up8 = [](int64_t n) { return (n + 7) & ~(int64_t)7; };
        const int64_t words = (up8((BT + 1) * H) + up8((BT + 1) * F) + up8((BT + 1) * 3 * H) + up8(BT * H)) / 2 + 16;
        if (int e = t_alloc(t, &raw, words)) return e;
        W2V2_HIP_CHECK(hipMemset(raw, 0, (size_t)words * 4));
        W2V2_HIP_CHECK(hipDeviceSynchronize());      // (a device memset may return before it ran, and the step's stream need not be a blocking one)
        t->dy16_h = reinterpret_cast<uint16_t*>(raw);
        t->dy16_f = t->dy16_h + up8((BT + 1) * H);
        t->dy16_3h = t->dy16_f + up8((BT + 1) * F);
        t->dy16_ctx = t->dy16_3h + up8((BT + 1) * 3 * H);      // dctx as the bf16 attention backward reads it
    }
    t->B = B;
    t->L = L;
    t->T = T;
    t->plan = plan;
    return W2V2_OK;
}

static int refresh_transposes(w2v2_model* m, hipStream_t s) {
    TrainState* t = m->train;
    // Precision mode 1 with shadows takes the plain bf16 copy of W as the (N, K) shadow of W^T in every data-gradient GEMM
    // that has one (all of the transformer's and the projection's), so the fp32 transposed copies of those kernels are
    // never read: only lm_head's (N = 32: no shadow) and the flipped positional kernel are needed.  `transposes_full`
    // remembers whether the fp32 copies are current, for a later switch back to fp32 / bf16x3 on the same model.
    const w2v2_config& c = m->cfg;
    bool need_full = !(m->precision == 1 && m->opt_shadows && m->w16_valid);
    if (!need_full) {      // every kernel whose fp32 copy is skipped must really have its bf16 stand-in (shapes with N % 64 != 0 do not)
        auto has = [&](const float* w) { return m->w16p.find(w) != m->w16p.end(); };
        need_full = !has(m->P("feature_projection/projection/kernel"));
        for (int i = 0; i < c.num_layers && !need_full; ++i) {
            const std::string b = "encoder/layers/" + std::to_string(i);
            need_full = !(has(m->qkv_w[i]) && has(m->P(b + "/attention/out_proj/kernel")) &&
                          has(m->P(b + "/feed_forward/intermediate_dense/kernel")) && has(m->P(b + "/feed_forward/output_dense/kernel")));
        }
    }
    if (t->transposes_fresh && (t->transposes_full || !need_full)) return W2V2_OK;
    const int H = c.hidden_size, F = c.intermediate_size;
    const int C = c.filter_sizes[c.num_conv_layers - 1];
    if (c.with_lm_head)
        if (int e = launch_transpose(m->P("lm_head/kernel"), t->WlmT, H, c.vocab_size, 1, s)) return e;
    if (need_full) {
        if (int e = launch_transpose(m->P("feature_projection/projection/kernel"), t->WpT, C, H, 1, s)) return e;
        for (int i = 0; i < c.num_layers; ++i) {
            const std::string b = "encoder/layers/" + std::to_string(i);
            LayerSave& l = t->layers[i];
            if (int e = launch_transpose(m->qkv_w[i], l.WqkvT, H, 3 * H, 1, s)) return e;
            if (int e = launch_transpose(m->P(b + "/attention/out_proj/kernel"), l.WoT, H, H, 1, s)) return e;
            if (int e = launch_transpose(m->P(b + "/feed_forward/intermediate_dense/kernel"), l.W1T, H, F, 1, s)) return e;
            if (int e = launch_transpose(m->P(b + "/feed_forward/output_dense/kernel"), l.W2T, F, H, 1, s)) return e;
        }
    }
    const int K = c.num_conv_pos_embeddings, G = c.num_conv_pos_embedding_groups;
    if (int e = launch_pos_conv_flip_regroup(m->pos_wg, t->pos_wg_t, K, H / G, G, s)) return e;
    t->pos_w16_t_fresh = false;
    t->transposes_fresh = true;
    t->transposes_full = need_full;
    return W2V2_OK;
}

static inline uint32_t layer_stream(int layer, int site) { return DS_LAYER_BASE + 4u * (uint32_t)layer + (uint32_t)site; }

static float* grad_of(w2v2_model* m, const std::string& name) {
    auto it = m->index.find(name);
    return it == m->index.end() ? nullptr : m->train->grads + m->train->goff[it->second];
}
static bool is_trainable(w2v2_model* m, const std::string& name) {
    auto it = m->index.find(name);
    return it != m->index.end() && m->train->trainable[it->second];
}

// Runs a plan of weight_grad_plan.h: dW (Kin x Nout) = A^T (Kin x M) dY (M x Nout), db = column sums of dY, A (M x Kin) row-major,
// A16 / dY16 the bf16 shadows of A and dY (same shapes) or null.  `w` is every byte of scratch it touches; `site` says who folds.
namespace w2v2 {
void weight_grad_knobs(int* dw_blocks, int* dw_uneven) {
    *dw_blocks = tune_int("W2V2_DW_BLOCKS", WG_BLOCKS_BF16);
    *dw_uneven = tune_int("W2V2_DW_UNEVEN", 1);
}

int launch_weight_grad(Profiler* prof, const WgProblem& q, const WgPlan& p, const float* A, const float* dY, const uint16_t* A16, const uint16_t* dY16,
                       float* dW, float* db, const WgScratch& w, const WgSite* site, hipStream_t s) {
    W2V2_REQUIRE(p.refusal == WGR_NONE, "%s", weight_grad_refusal_text(p.refusal));
    const int M = q.M, Kin = q.Kin, Nout = q.Nout, S = p.S, Kp = p.Kp, Mq = p.Mq, R = p.R;
    const int64_t elems = (int64_t)Kin * Nout;
    float* const dst = p.dst == WG_TO_SLABS ? w.slabs : dW;
    float* const tail_dst = dst + (int64_t)S * elems;      // slab S: the leftover rows [Mq, M)
    // S slabs of Kp rows on the bf16 kernel the plan names, A transposed on its way in
    auto slabs_bf16 = [&](const GemmShadows& x) -> int {
        return launch_gemm_bf16_x(prof, A, Kin, (int64_t)Kp * Kin, dY, Nout, (int64_t)Kp * Nout, dst, Nout, elems, nullptr, nullptr, Kin, Nout, Kp, S, 0, x, s);
    };
    // `rows` rows from row `r0` through a transposed copy `at` (Kin, rows) and the fp32 GEMM, as nb slabs of kp rows
    auto slabs_copy = [&](int r0, int rows, float* at, float* out, int kp, int nb, int64_t strideC) -> int {
        if (int e = launch_transpose(A + (int64_t)r0 * Kin, at, rows, Kin, 1, s)) return e;
        return launch_gemm_ex(prof, at, rows, nb == 1 ? 0 : kp, dY + (int64_t)r0 * Nout, Nout, nb == 1 ? 0 : (int64_t)kp * Nout, out, Nout,
                              strideC, nullptr, nullptr, Kin, Nout, kp, nb, 0, s);
    };
    GemmShadows x;
    x.transA = true;
    switch (p.form) {
        case WG_BIAS_ONLY: break;
        case WG_UNEVEN_128x256:
        case WG_RAGGED_128x128:
        case WG_DIV_SHADOWS:        // (no fp32 operand is read: callers may pass null)
            x.A16 = A16; x.B16p = dY16; x.kextra = p.kextra; x.validK = p.validK; x.b_zero_row = p.b_zero_row;
            if (S)
                if (int e = slabs_bf16(x)) return e;
            if (R)
                if (int e = launch_dw_tail_bf16(A16 + (int64_t)Mq * Kin, Kin, dY16 + (int64_t)Mq * Nout, Nout, tail_dst, R, Kin, Nout, s)) return e;
            break;
        case WG_DIV_F32_REG:
            if (p.bias == WG_BIAS_FUSED) { x.colsum = w.cs_ws; x.strideCS = Nout; }
            if (S)
                if (int e = slabs_bf16(x)) return e;
            if (R)
                if (int e = slabs_copy(Mq, R, w.at + (int64_t)Kin * Mq, tail_dst, R, 1, 0)) return e;
            break;
        case WG_DIV_F32_COPY:
            if (S)
                if (int e = slabs_copy(0, Mq, w.at, dst, Kp, S, elems)) return e;
            if (R)
                if (int e = slabs_copy(Mq, R, w.at + (int64_t)Kin * Mq, tail_dst, R, 1, 0)) return e;
            break;
        default: W2V2_REQUIRE(false, "weight_grad: unknown form %d", p.form);
    }
    // dW = sum of the slabs: as a job of the layer's fold launch, or behind the GEMM (the unpacking fold: still one launch for the sum and
    // the scatter into the three kernels; the plain one: its one-chunk partial scratch lives behind the slabs, which the plan checked)
    if (p.fold) {
        FoldBatch* const defer = (site && site->slabs) ? site->defer : nullptr;
        auto add = [&](FoldBatch& b) {
            return q.unpack ? b.add_tall(w.slabs, p.nslabs, elems, site->unpack3[0], site->unpackH, site->unpack3[1], site->unpack3[2])
                            : b.add_tall(w.slabs, p.nslabs, elems, dW);
        };
        if (defer && add(*defer)) {
        } else if (q.unpack) {
            FoldBatch one;
            W2V2_REQUIRE(add(one), "weight_grad: the unpacking fold does not fit this shape");
            if (int e = one.flush(s)) return e;
        } else if (int e = launch_colsum(w.slabs, dW, p.nslabs, (int)elems, w.slabs + (int64_t)p.nslabs * elems, 0, s)) {
            return e;
        }
    }
    if (p.bias == WG_BIAS_FUSED) {      // per-slab column sums of dY are in cs_ws (S, Nout); the leftover rows add one more row, then one small fold
        if (R)
            if (int e = launch_colsum(dY + (int64_t)Mq * Nout, w.cs_ws + (int64_t)S * Nout, R, Nout, w.red_ws, 0, s)) return e;
        return launch_colsum(w.cs_ws, db, p.nslabs, Nout, w.red_ws, 0, s);
    }
    if (p.bias == WG_BIAS_PASS) return launch_colsum(dY, db, M, Nout, w.red_ws, 0, s);
    return W2V2_OK;
}
}  // namespace w2v2

// The training step's weight gradients: the problem and the scratch from the model.  dy16_zero_row: the caller keeps row M of dY16
// all-zero (TrainState's dY shadows are allocated that way).  red_ws: the side stream passes its own (TrainState::red_ws_side).
static int weight_grad(w2v2_model* m, const float* A, const float* dY, int M, int Kin, int Nout, float* dW, float* db, hipStream_t s,
                       const uint16_t* A16 = nullptr, const uint16_t* dY16 = nullptr, bool dy16_zero_row = false, float* red_ws = nullptr,
                       const WgSite* site = nullptr) {
    TrainState* t = m->train;
    const bool own = site && site->slabs;
    int dw_blocks, dw_uneven;
    weight_grad_knobs(&dw_blocks, &dw_uneven);
    const WgProblem q{M, Kin, Nout, gemm_get_precision(), A != nullptr, dY != nullptr, A16 != nullptr, dY16 != nullptr, dy16_zero_row, dW != nullptr,
                      db != nullptr, site && site->unpackH > 0, t->slab_floats, own ? site->slab_floats : 0, t->cs_floats, dw_blocks, dw_uneven};
    const WgScratch w{own ? site->slabs : t->slabs, t->at, t->cs_ws, red_ws ? red_ws : t->red_ws};
    return launch_weight_grad(m->prof, q, weight_grad_plan(q), A, dY, A16, dY16, dW, db, w, site, s);
}

extern "C" {

int w2v2_set_trainable(w2v2_model* m, const char* prefix, int trainable) {
    W2V2_REQUIRE(m && prefix, "set_trainable: null argument");
    TrainState* t = get_state(m);
    int hits = 0;
    for (size_t i = 0; i < m->params.size(); ++i)
        if (m->params[i].name.compare(0, strlen(prefix), prefix) == 0) {
            t->trainable[i] = trainable ? 1 : 0;
            t->adam_table_fresh = false;
            ++hits;
        }
    if (!hits) {
        set_error("set_trainable: no variable starts with `%s`", prefix);
        return W2V2_ENOTFOUND;
    }
    return W2V2_OK;
}

int w2v2_set_trainable_flags(w2v2_model* m, const uint8_t* flags, int32_t n) {
    W2V2_REQUIRE(m && flags, "set_trainable_flags: null argument");
    W2V2_REQUIRE(n == (int32_t)m->params.size(), "set_trainable_flags: %d flags for %d variables", n, (int)m->params.size());
    TrainState* t = get_state(m);
    bool changed = false;
    for (int32_t i = 0; i < n; ++i) {
        const uint8_t f = flags[i] ? 1 : 0;
        changed |= t->trainable[i] != f;
        t->trainable[i] = f;
    }
    if (changed) t->adam_table_fresh = false;
    return W2V2_OK;
}

int w2v2_train_forward(w2v2_model* m, const float* wave, int32_t B, int64_t L, const int32_t* mask,
                       const uint8_t* spec_mask_host, const float* sd_keep_host, float dropout_p,
                       uint64_t seed, float* logits_out, void* stream) {
    W2V2_REQUIRE(m && wave && logits_out, "train_forward: null argument");
    // ("f16x2" is an inference mode -- its range contract |activation| < 4094 is not watched by the training kernels, and
    //  the step would silently run the six-product bf16x3 path instead)
    W2V2_REQUIRE(m->precision != 3, "train_forward: precision f16x2 is an inference-forward mode; train in fp32, bf16 or bf16x3");
    W2V2_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "train_forward: dropout %f outside [0, 1)", dropout_p);
    // (the keep decisions compare 16 hash bits with floor(p 2^16): a positive p below that resolution would scale by 1 / (1 - p) in
    //  some kernels and not drop at all in others -- one predicate everywhere: every accepted p > 0 has a non-zero threshold)
    W2V2_REQUIRE(dropout_p == 0.f || dropout_p >= 1.0f / 65536.0f, "train_forward: dropout %g is below the 2^-16 resolution of the keep decisions", dropout_p);
    if (!m->finalized) {
        set_error("train_forward: call w2v2_finalize after setting the variables");
        return W2V2_ESTATE;
    }
    const w2v2_config& c = m->cfg;
    PrecisionScope precision(m->precision);
    StepProfScope step_prof(m->prof);          // the training-only kernels' launchers find the profiler here (common.h)
    const int64_t Tll = w2v2_num_frames(m, L);
    W2V2_REQUIRE(Tll >= 1, "train_forward: input too short");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int e = w2v2_ensure_workspace(m, B, L)) return e;
    const int T = (int)Tll;
    const int H = c.hidden_size, F = c.intermediate_size;
    const int64_t BT = (int64_t)B * T;
    if (m->precision == 1 && m->opt_shadows)       // (also refreshes the bf16 weight shadows after an optimizer step: m->w16_valid, which the plan reads)
        if (int e = w2v2_ensure_shadows(m, B, T, s)) return e;
    const TrainPlan plan = plan_train(m, B, L);
    if (int e = ensure_train_ws(m, plan, L)) return e;
    TrainState* t = m->train;
    t->forward_done = false;           // (until this forward completes there is nothing for a backward to differentiate)
    Profiler* pf = m->prof;
    const bool sh = plan.sh, attn16 = plan.attn16, ffn16_only = plan.ffn16_only, u16_only = plan.u16_only, ctx16_only = plan.ctx16_only,
               ln16_only = plan.ln16_only, prenorm = plan.prenorm;
    const int act = plan.act, act_ew = plan.act_ew;
    const float eps = c.layer_norm_eps, p = dropout_p;
    t->p = p;
    t->seed = seed;
    // (the non-plane-fed routes of the inference forward's gemm(): six-product split, fp32, bf16 with shadows -- forward.hip)
    auto gemm = [&](const float* A, const uint16_t* A16, int64_t lda, int64_t strideA, const float* Bw, int64_t ldb, float* Cc,
                    uint16_t* C16, int64_t ldc, int64_t strideC, const float* bias, const float* res, int M, int N, int K,
                    int nbatch, int act_) -> int {
        return w2v2_gemm_route(m, sh, s, A, A16, lda, strideA, Bw, ldb, Cc, C16, ldc, strideC, bias, res, M, N, K, nbatch, act_);
    };
    auto S16 = [&](uint16_t* p16) -> uint16_t* { return sh ? p16 : nullptr; };

    // ---- frozen feature extractor and feature projection LN -> Dense: the inference forward's stage (no dropout inside,
    // feature_extractor.py:54-59,92-95), planned without operand planes: the bf16x3 conv GEMMs stay on the six-product kernel ----
    if (int e = w2v2_forward_frontend(m, w2v2_plan_forward(m, B, L, false, false), wave, nullptr, s)) return e;
    // ---- Dropout behind the projection (feature_extractor.py:95) ----
    if (int e = launch_dropout_fwd(m->proj, nullptr, t->hd, BT * H, 0, p, seed, DS_FEATURE_PROJECTION, s)) return e;
    // ---- spec-augment: masked frames <- masked_spec_embed (modeling.py:193-199, spec_augment.py:119-127) ----
    t->have_spec = spec_mask_host != nullptr;
    const float* enc_x = t->hd;
    if (t->have_spec) {
        W2V2_HIP_CHECK(hipMemcpyAsync(t->spec_mask, spec_mask_host, (size_t)BT, hipMemcpyHostToDevice, s));
        if (int e = launch_spec_aug_fwd(t->hd, t->spec_mask, m->P("masked_spec_embed"), t->hm, BT, H, s)) return e;
        enc_x = t->hm;
    }
    // ---- encoder (encoder.py:251-276) ----
    const int32_t* flen = nullptr;
    t->have_mask = mask != nullptr;
    if (mask) {
        if (int e = launch_frame_lengths(pf, mask, m->frame_len, B, L, c.kernal_sizes, c.strides, c.num_conv_layers, s)) return e;
        flen = m->frame_len;
    }
    // posout = xz + GELU(c), c saved for backward
    if (w2v2_pos_conv_bf16_ok(m)) {      // precision mode 1: batched bf16 GEMM (posconv.hip); m->t0 is free scratch here
        if (int e = w2v2_ensure_pos16(m, B, T, s)) return e;
        if (int e = launch_pos_conv_bf16(pf, enc_x, m->pos_w16, m->P("encoder/pos_conv_embed/conv/bias"), flen, m->posout, t->pos_c,
                                         m->pos_pack16, m->t0, B, T, H, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups,
                                         act, c.num_conv_pos_embeddings / 2, 1, s))
            return e;
    } else if (int e = launch_pos_conv_ex(pf, enc_x, m->pos_wg, m->P("encoder/pos_conv_embed/conv/bias"), flen, m->posout, t->pos_c,
                                          B, T, H, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, act,
                                          c.num_conv_pos_embeddings / 2, 1, s)) {
        return e;
    }
    // postnorm: hs[0] = dropout(LN(posout));  prenorm: hs[0] = dropout(posout)   (encoder.py:267-270)
    {
        const float* pre = m->posout;
        if (!prenorm) {
            if (int e = launch_layer_norm(pf, m->posout, m->t0, m->P("encoder/layer_norm/gamma"), m->P("encoder/layer_norm/beta"), BT, H, eps, 0, s)) return e;
            pre = m->t0;
        }
        float* h0 = prenorm ? t->hs0 : m->hs[0];      // prenorm: m->hs[0] aliases posout, keep the dropped copy apart
        // postnorm: layer 0's q|k|v GEMM reads this tensor -> shadow
        if (int e = launch_dropout_fwd_x(pre, nullptr, h0, (sh && !prenorm) ? m->hs16[0] : nullptr, BT * H, 0, p, seed, DS_ENCODER_IN, s)) return e;
    }
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string b = "encoder/layers/" + std::to_string(i);
        LayerSave& l = t->layers[i];
        const float* x = (prenorm && i == 0) ? t->hs0 : m->hs[i];
        l.keep = sd_keep_host ? sd_keep_host[i] : 1.0f;
        const float* attn_in = x;
        const uint16_t* attn_in16 = (sh && !prenorm) ? m->hs16[i] : nullptr;   // postnorm: written by the producer of hs[i]
        if (prenorm) {     // x + drop(attn(LN(x)))   (encoder.py:114-119)
            if (int e = launch_layer_norm_x(pf, x, ln16_only ? nullptr : l.a, m->P(b + "/layer_norm/gamma"), m->P(b + "/layer_norm/beta"), BT, H, eps, 0,
                                            S16(l.a16), s))
                return e;
            attn_in = ln16_only ? nullptr : l.a;
            attn_in16 = S16(l.a16);
        }
        // the bf16 attention kernels (forward and backward) read q | k | v only as bf16: the projection then writes just that shadow
        if (int e = gemm(attn_in, attn_in16, H, 0, m->qkv_w[i], 3 * H, attn16 ? nullptr : l.qkv, attn16 ? l.qkv16 : nullptr, 3 * H, 0, m->qkv_b[i],
                         nullptr, (int)BT, 3 * H, H, 1, 0))
            return e;
        AttnTrain tr{p, seed, layer_stream(i, 0), l.lse, attn16 ? l.keep_bits : nullptr};
        AttnIO aio;
        aio.qkv = attn16 ? nullptr : l.qkv; aio.qkv16 = attn16 ? l.qkv16 : nullptr; aio.frame_len = flen;
        aio.ctx = ctx16_only ? nullptr : l.ctx; aio.ctx16 = attn16 ? l.ctx16 : nullptr; aio.train = &tr;
        if (int e = launch_attention_train_routed(pf, plan.attn, aio, s)) return e;
        // o = ctx Wo + bo;  t1 = dropout(o) + x   (encoder.py:116-119)
        // (dropout + residual as their own pass: folded into this GEMM's epilogue they were measured slower, study section 12 / r03)
        if (int e = gemm(ctx16_only ? nullptr : l.ctx, attn16 ? l.ctx16 : nullptr, H, 0, m->P(b + "/attention/out_proj/kernel"), H, m->t0, nullptr, H, 0,
                         m->P(b + "/attention/out_proj/bias"), nullptr, (int)BT, H, H, 1, 0))
            return e;
        // postnorm: t2 = LN1(t1) feeds the FFN and is its residual; prenorm: t2 = LN2(t1) feeds the FFN, t1 is the residual
        const char* ln_a = prenorm ? "/final_layer_norm" : "/layer_norm";
        // (round 4: dropout + residual + LayerNorm as one pass over the row -- t1 is written once and not read back)
        // (the fused pass takes rows of up to 2048 channels, a multiple of 4, 16-byte aligned: anything else falls back to the two kernels)
        if (H % 4 == 0 && H <= 2048 && tune_int("W2V2_LN_DROP", 1) != 0 &&
            ((reinterpret_cast<uintptr_t>(m->t0) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(l.t1) | reinterpret_cast<uintptr_t>(l.t2) |
              reinterpret_cast<uintptr_t>(m->P(b + ln_a + "/gamma")) | reinterpret_cast<uintptr_t>(m->P(b + ln_a + "/beta"))) & 15) == 0 &&
            (reinterpret_cast<uintptr_t>(S16(l.t2_16)) & 7) == 0) {
            if (int e = launch_layer_norm_drop(pf, m->t0, x, l.t1, ln16_only ? nullptr : l.t2, S16(l.t2_16), m->P(b + ln_a + "/gamma"), m->P(b + ln_a + "/beta"), BT, H, eps, p,
                                               seed, layer_stream(i, 1), s))
                return e;
        } else {
            if (int e = launch_dropout_fwd(m->t0, x, l.t1, BT * H, 0, p, seed, layer_stream(i, 1), s)) return e;
            if (int e = launch_layer_norm_x(pf, l.t1, ln16_only ? nullptr : l.t2, m->P(b + ln_a + "/gamma"), m->P(b + ln_a + "/beta"), BT, H, eps, 0, S16(l.t2_16), s)) return e;
        }
        const float* ffn_res = prenorm ? l.t1 : l.t2;
        float* ffn_out = prenorm ? m->hs[i + 1] : l.t3;
        if (l.keep != 0.f) {
            // u = t2 W1 + b1;  gd = dropout(GELU(u));  out = res + keep * (gd W2 + b2)   (encoder.py:127-130)
            // (ffn16_only: every reader of gd -- the next GEMM, and the down-projection's weight gradient -- streams the bf16 shadow)
            uint16_t* const u16 = u16_only ? reinterpret_cast<uint16_t*>(l.u) : nullptr;
            if (int e = gemm(ln16_only ? nullptr : l.t2, S16(l.t2_16), H, 0, m->P(b + "/feed_forward/intermediate_dense/kernel"), F, u16_only ? nullptr : l.u, u16, F, 0,
                             m->P(b + "/feed_forward/intermediate_dense/bias"), nullptr, (int)BT, F, H, 1, 0))
                return e;
            EwBf16 uin;
            uin.a16 = u16; uin.round_in = plan.u_round;
            if (int e = launch_dropout_fwd_x(u16_only ? nullptr : l.u, nullptr, ffn16_only ? nullptr : l.gd, S16(l.gd16), BT * F, act_ew, p, seed,
                                             layer_stream(i, 2), s, uin))
                return e;
            if (int e = gemm(ffn16_only ? nullptr : l.gd, S16(l.gd16), F, 0, m->P(b + "/feed_forward/output_dense/kernel"), H, ffn_out, nullptr, H, 0,
                             m->P(b + "/feed_forward/output_dense/bias"), ffn_res, (int)BT, H, F, 1, 0))
                return e;
        } else {
            W2V2_HIP_CHECK(hipMemcpyAsync(ffn_out, ffn_res, (size_t)BT * H * 4, hipMemcpyDeviceToDevice, s));
        }
        if (!prenorm)
            if (int e = launch_layer_norm_x(pf, l.t3, m->hs[i + 1], m->P(b + "/final_layer_norm/gamma"),
                                            m->P(b + "/final_layer_norm/beta"), BT, H, eps, 0, S16(m->hs16[i + 1]), s))
                return e;
    }
    // ---- [prenorm: final encoder LN] -> Dropout -> lm_head (encoder.py:274-275, modeling.py:253-254) ----
    const float* head_in = m->hs[c.num_layers];
    if (prenorm) {
        if (int e = launch_layer_norm(pf, m->hs[c.num_layers], m->enc_out, m->P("encoder/layer_norm/gamma"),
                                      m->P("encoder/layer_norm/beta"), BT, H, eps, 0, s))
            return e;
        head_in = m->enc_out;
    }
    if (!c.with_lm_head) {
        // Wav2Vec2Model.call(training=True) (modeling.py:169-209): the backbone's hidden states (B, T, H); the head's Dropout and
        // Dense belong to Wav2Vec2ForCTC.  No backward from here (the training step differentiates the CTC model).
        W2V2_HIP_CHECK(hipMemcpyAsync(logits_out, head_in, (size_t)BT * H * 4, hipMemcpyDeviceToDevice, s));
        t->forward_done = false;
        return W2V2_OK;
    }
    if (int e = launch_dropout_fwd_x(head_in, nullptr, t->hdf, S16(m->enc16), BT * H, 0, p, seed, DS_HEAD, s)) return e;
    if (int e = gemm(t->hdf, S16(m->enc16), H, 0, m->P("lm_head/kernel"), c.vocab_size, logits_out, nullptr, c.vocab_size, 0,
                     m->P("lm_head/bias"), nullptr, (int)BT, c.vocab_size, H, 1, 0))
        return e;
    t->plan = plan;                    // what the backward reads: the per-layer X shadows (and hs16) hold this forward's activations iff plan.sh
    t->forward_done = true;
    return W2V2_OK;
}

}  // extern "C"

// ---- the backward: w2v2_train_backward sets up one BwdCtx and runs four stages over it -------------------------------------------------
// head -> encoder layers -> encoder input, positional conv, spec-augment -> feature projection.  Every mode-dependent decision comes from
// `plan`, the plan of the forward being differentiated (TrainState::plan), never from the model's settings at backward time.
struct BwdCtx {
    w2v2_model* m;
    TrainState* t;
    const TrainPlan& plan;
    hipStream_t s;
    int B, T, H, F;
    int64_t BT;
    float eps, p;
    uint64_t seed;
    const int32_t* flen;
    // dX = dY W^T reads the fp32 transposed copy WT ([out][in]) as its B operand; in mode bf16 with shadows the bf16 copy of W itself
    // ([in][out] = (N, K) for this GEMM) is the B shadow -- no transpose needed.  Bit-identical results.  `shb` also says that the
    // forward's X shadows and the dY shadows below are there for the weight-gradient GEMMs (plan.sh is part of it).
    bool shb;
    // bf16 shadows of dY (written by its producer) for the data-gradient GEMMs: only where the consumer will take them
    uint16_t *s16h, *s16f, *s16q;
    float *dh, *tmp, *tmp2, *tmp3;            // (BT, H) gradient scratch: TrainState::gh
    // weight-gradient side stream (TrainState::wg_stream) and deferred folds (train.h: FoldBatch) of the encoder layers
    bool side_on = false;
    int defer_mode = 0;
    FoldBatch fold;
    FoldBatch* fb = nullptr;
    float *ln2_ws = nullptr, *ln1_ws = nullptr;
    bool wg_pending[4] = {false, false, false, false};
    bool wg_used = false;
    // head -> layers (prenorm): the encoder LayerNorm's backward already summed dh's columns into the top layer's b2 gradient / wrote dh's shadow
    float* head_b2 = nullptr;
    bool head_dh16 = false;

    float* G(const std::string& n) const { return is_trainable(m, n) ? grad_of(m, n) : nullptr; }
    bool dx_shadowed(const float* W) const { return shb && m->w16p.find(W) != m->w16p.end(); }
    // A16: the producer's bf16 shadow of A (or null): with it both operands stream by LDS-DMA (gemm_bf16.hip source 5)
    // (C16: bf16 shadow of the result, only from the shadow branch -- callers ask for it only when `dx_shadowed(W)`)
    int gemm_dx(const float* A, const uint16_t* A16, int64_t lda, const float* WT, const float* W, float* Cc, int64_t ldc, const float* res, int M,
                int N, int K, hipStream_t st, uint16_t* C16 = nullptr) const {
        if (shb) {
            auto it = m->w16p.find(W);
            if (it != m->w16p.end()) {
                GemmShadows x;
                x.A16 = A16;
                x.C16 = C16;
                x.B16 = it->second;
                x.ldb16 = K;
                return launch_gemm_bf16_x(m->prof, A, lda, 0, WT, N, 0, Cc, ldc, 0, nullptr, res, M, N, K, 1, 0, x, st);
            }
        }
        if (w2v2_use_split_gemm(m, A, lda, 0, N, M, N, K, 1)) {                   // mode bf16x3: planes of the transposed copy
            const uint16_t* planes = nullptr;
            if (int e = w2v2_split_planes(m, WT, K, N, st, &planes)) return e;
            return launch_gemm_split(m->prof, A, lda, 0, planes, Cc, ldc, 0, nullptr, res, M, N, K, 1, 0, st);
        }
        return launch_gemm(m->prof, A, lda, 0, WT, N, Cc, ldc, 0, nullptr, res, M, N, K, 1, 0, st);
    }
    // With the shadows on, the weight-gradient GEMMs take the LDS-DMA / transposing-read kernel, which has no fp32 dY in registers to
    // sum for the bias gradient: the PRODUCER of each dY leaves its column sums instead (dropout backward, LayerNorm backward), and
    // weight_grad is called without a bias target.  `bias_done` says that happened.
    int dropout_bwd_bias(const float* u, const float* dy, float* dx, uint16_t* dx16, int64_t rows, int cols, int act_, uint32_t stream_id, float* bias_grad,
                         bool* bias_done, const EwBf16& in = EwBf16{}, bool deferrable = false) {
        *bias_done = false;
        if (shb && bias_grad) {
            *bias_done = true;
            const bool d = deferrable && fb;        // (the FFN site: its partial rows live in site_ws[1] until the layer's fold launch)
            return launch_dropout_bwd_colsum(u, dy, dx, dx16, bias_grad, rows, cols, act_, p, seed, stream_id, d ? t->site_ws[1] : t->red_ws, s, in,
                                             d ? fb : nullptr);
        }
        return launch_dropout_bwd_x(u, dy, dx, dx16, rows * cols, act_, p, seed, stream_id, s, in);
    }
    WgSite wg_site(int k) {
        WgSite w;
        if (defer_mode == 2) { w.slabs = t->site_slabs[k]; w.slab_floats = t->site_slab_floats[k]; w.defer = fb; }
        return w;
    }
    // side(site, f): run f(stream, reduction scratch) -- a weight gradient -- behind everything the main stream has enqueued so far
    template <class Fn>
    int side(int site, Fn&& f) {
        if (!side_on) return f(s, t->red_ws);
        W2V2_HIP_CHECK(hipEventRecord(t->wg_fork, s));
        W2V2_HIP_CHECK(hipStreamWaitEvent(t->wg_stream, t->wg_fork, 0));
        if (int e = f(t->wg_stream, t->red_ws_side)) return e;
        W2V2_HIP_CHECK(hipEventRecord(t->wg_join[site], t->wg_stream));
        wg_pending[site] = wg_used = true;
        return W2V2_OK;
    }
    // the main stream is about to overwrite what site's weight gradient reads
    int side_wait(int site) {
        if (wg_pending[site]) {
            W2V2_HIP_CHECK(hipStreamWaitEvent(s, t->wg_join[site], 0));
            wg_pending[site] = false;
        }
        return W2V2_OK;
    }
    // bucket k's slice of the flat buffer is final once this is recorded (w2v2_train_bucket_wait): with the side stream in use the
    // event goes THERE, after the side stream has caught up with the main stream's position (LayerNorm / bias gradients come from it)
    int bucket_done(int k) {
        if (wg_used) {
            W2V2_HIP_CHECK(hipEventRecord(t->wg_main, s));
            W2V2_HIP_CHECK(hipStreamWaitEvent(t->wg_stream, t->wg_main, 0));
            W2V2_HIP_CHECK(hipEventRecord(t->bucket_ev[k], t->wg_stream));
            return W2V2_OK;
        }
        W2V2_HIP_CHECK(hipEventRecord(t->bucket_ev[k], s));
        return W2V2_OK;
    }
    // the two branches of an encoder layer, written once for both norms (below)
    int qkv_weight_grad(const std::string& b, const float* attn_in, const uint16_t* attn_in16, bool only16, hipStream_t st, float* rws);
    int ffn_branch_bwd(int i, LayerSave& l, const std::string& b, const float* dy, const uint16_t* dy16, bool b2_done, float* dx, const float* res);
    bool do16_only(const std::string& b) const;
    int attn_branch_bwd(int i, LayerSave& l, const std::string& b, const float* dt1, const float* attn_in, const uint16_t* attn_in16, bool do_tail,
                        float* dx, const float* res);
};

// ---- head: lm_head's gradients (bucket 0), then dh = d loss / d hs[N] ----
static int bwd_head(BwdCtx& x, const float* dlogits, bool below_head) {
    w2v2_model* m = x.m;
    TrainState* t = x.t;
    const w2v2_config& c = m->cfg;
    const int H = x.H, V = c.vocab_size;
    const int64_t BT = x.BT;
    hipStream_t s = x.s;
    if (int e = weight_grad(m, t->hdf, dlogits, (int)BT, H, V, x.G("lm_head/kernel"), x.G("lm_head/bias"), s)) return e;
    if (int e = x.bucket_done(0)) return e;
    if (!below_head) return W2V2_OK;          // stage 1 of the reference: only lm_head trains (main.py:210)
    if (int e = launch_gemm(m->prof, dlogits, V, 0, t->WlmT, H, x.tmp, H, 0, nullptr, nullptr, (int)BT, H, V, 1, 0, s)) return e;
    if (!x.plan.prenorm) return launch_dropout_bwd(nullptr, x.tmp, x.dh, BT * H, 0, x.p, x.seed, DS_HEAD, s);
    // prenorm: hdf = dropout(LN_enc(hs[N]))   (encoder.py:274-275)
    if (int e = launch_dropout_bwd(nullptr, x.tmp, x.tmp2, BT * H, 0, x.p, x.seed, DS_HEAD, s)) return e;
    float* dg = x.G("encoder/layer_norm/gamma");
    float* db = x.G("encoder/layer_norm/beta");
    // (round 5: this pass also leaves dh's bf16 shadow -- a separate rounding kernel before -- and, on the shadow path, the column
    //  sums of dh = the top layer's down-projection bias gradient: see `b2_done` in bwd_layers)
    const bool top16 = x.s16h && (BT * H) % 4 == 0 && (reinterpret_cast<uintptr_t>(x.dh) & 15) == 0;
    x.head_b2 = (x.shb && tune_int("W2V2_B2_FROM_LN", 1) != 0 && c.num_layers > 0 && t->layers[c.num_layers - 1].keep != 0.f)
                    ? x.G("encoder/layers/" + std::to_string(c.num_layers - 1) + "/feed_forward/output_dense/bias") : nullptr;
    if (int e = launch_ln_bwd_x(m->hs[c.num_layers], m->P("encoder/layer_norm/gamma"), x.tmp2, x.dh, top16 ? x.s16h : nullptr, dg ? dg : t->dummy,
                                db ? db : t->dummy + H, BT, H, x.eps, t->red_ws, s, x.head_b2))
        return e;
    x.head_dh16 = top16;
    return W2V2_OK;
}

// packed q|k|v projection: dW (H, 3H) -> the three (H, H) kernels, db (3H) -> the three biases.  only16: dqkv exists only as bf16
// (+ the attention backward's column partials for the bias gradient)
int BwdCtx::qkv_weight_grad(const std::string& b, const float* attn_in, const uint16_t* attn_in16, bool only16, hipStream_t st, float* rws) {
    float* dWqkv = t->dwqkv;
    float* dbqkv = dWqkv + (int64_t)3 * H * H;
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    float* gw3[3];
    float* gb3[3];
    bool all6 = true;
    for (int j = 0; j < 3; ++j) {
        gw3[j] = G(b + "/attention/" + names[j] + "/kernel");
        gb3[j] = G(b + "/attention/" + names[j] + "/bias");
        all6 = all6 && gw3[j] && gb3[j];
    }
    if (fb && only16 && all6 && H % 4 == 0 && fold.tab.n + 2 <= FOLD_MAX_JOBS) {
        // deferred: the layer's fold launch sums the (H, 3H) slabs straight into the three (H, H) kernels and the attention backward's
        // column partials into the three biases (group g of the wide job = columns [g H, (g + 1) H) of the 3H-wide partial rows)
        WgSite site = wg_site(3);
        site.unpackH = H;
        for (int j = 0; j < 3; ++j) site.unpack3[j] = gw3[j];
        if (int e = weight_grad(m, attn_in, nullptr, (int)BT, H, 3 * H, dWqkv, nullptr, st, s16q ? attn_in16 : nullptr, s16q, s16q != nullptr, rws, &site))
            return e;
        W2V2_REQUIRE(fb->add_wide(t->attn_colpart, attention_colpart_rows(B, T), H, (int64_t)3 * H, 3, gb3[0], gb3[1], gb3[2]),
                     "train_backward: fold table full");
        return W2V2_OK;
    }
    if (int e = weight_grad(m, attn_in, only16 ? nullptr : t->g3h, (int)BT, H, 3 * H, dWqkv, only16 ? nullptr : dbqkv, st, s16q ? attn_in16 : nullptr, s16q,
                            s16q != nullptr, rws))
        return e;
    if (only16)
        if (int e = launch_colsum_fold(t->attn_colpart, dbqkv, attention_colpart_rows(B, T), 3 * H, st)) return e;
    if (H % 4 == 0) return launch_qkv_unpack(dWqkv, dbqkv, gw3, gb3, H, st);
    for (int j = 0; j < 3; ++j) {
        if (gw3[j])
            W2V2_HIP_CHECK(hipMemcpy2DAsync(gw3[j], (size_t)H * 4, dWqkv + j * H, (size_t)3 * H * 4, (size_t)H * 4, (size_t)H, hipMemcpyDeviceToDevice, st));
        if (gb3[j]) W2V2_HIP_CHECK(hipMemcpyAsync(gb3[j], dbqkv + j * H, (size_t)H * 4, hipMemcpyDeviceToDevice, st));
    }
    return W2V2_OK;
}

// FFN branch of layer i, f = dropout(GELU(in W1 + b1)) W2 + b2, for both norms: given dy = d loss / d f (fp32, and its bf16 shadow dy16 or
// null) it leaves the four FFN gradients and dx = d loss / d `in` (+ res, the residual path's gradient, if given).  b2_done: the kernel
// that produced dy already left its column sums in the down-projection's bias gradient.
int BwdCtx::ffn_branch_bwd(int i, LayerSave& l, const std::string& b, const float* dy, const uint16_t* dy16, bool b2_done, float* dx,
                          const float* res) {
    const bool f16 = plan.ffn16_only;
    const float* W1 = m->P(b + "/feed_forward/intermediate_dense/kernel");
    const float* W2 = m->P(b + "/feed_forward/output_dense/kernel");
    const WgSite ws0 = wg_site(0), ws1 = wg_site(1);
    W2V2_REQUIRE(!f16 || dy16, "train_backward: no bf16 shadow of the FFN output's gradient");
    // (dy16 is null or the H-wide dY shadow of TrainState, whose row BT stays zero: weight_grad's dy16_zero_row.  Without dy16 the
    //  weight gradient takes no shadow at all, so gd16 is passed only along with it)
    if (int e = side(0, [&](hipStream_t st, float* rws) {
            return weight_grad(m, f16 ? nullptr : l.gd, dy, (int)BT, F, H, G(b + "/feed_forward/output_dense/kernel"),
                               b2_done ? nullptr : G(b + "/feed_forward/output_dense/bias"), st, (shb && dy16) ? l.gd16 : nullptr, dy16, dy16 != nullptr,
                               rws, &ws0);
        }))
        return e;
    // du = dgd * keep/(1-p) * GELU'(u)   (+ its column sums = the up-projection's bias gradient)
    bool b1_done = false;
    float* const gb1 = G(b + "/feed_forward/intermediate_dense/bias");
    // (f16: du is needed only as bf16 -- both consumers stream the shadow -- unless its fp32 column sums are still to be taken)
    const bool du16_only = f16 && (!gb1 || shb) && dx_shadowed(W1);
    float* const du = du16_only ? nullptr : t->gf;
    if (int e = side_wait(1)) return e;              // (du / its shadow: read by the layer above's up-projection weight gradient)
    // dgd = dy W2^T (the down-projection's data gradient) into t->gf, then du = dropout-backward(dgd) * GELU'(u) with its column sums
    // (the up-projection's bias gradient) as one element-wise pass.  (In round 2 that pass rode in the GEMM's epilogue; with the GEMM
    // on the 128 x 256 kernel the separate pass at the HBM roofline is faster: profiles/r03_gemm_bf16_study.md.)
    EwBf16 in;
    in.round_in = plan.u_round;
    if (plan.u16_only) {
        // the forward kept u only as bf16; the gradient of the hidden activation is written only as bf16 too (the data-gradient
        // GEMM's bf16 epilogue, into the buffer du's shadow will occupy) and GELU' x dropout-backward runs on it in place
        W2V2_REQUIRE(s16f && dx_shadowed(W2), "train_backward: the forward kept u as bf16 only, which needs the shadow path for the down-projection's data gradient");
        if (int e = gemm_dx(dy, dy16, H, l.W2T, W2, nullptr, F, nullptr, (int)BT, F, H, s, s16f)) return e;
        in.a16 = reinterpret_cast<const uint16_t*>(l.u); in.b16 = s16f;
        if (int e = dropout_bwd_bias(nullptr, nullptr, du, s16f, BT, F, plan.act_ew, layer_stream(i, 2), gb1, &b1_done, in, true)) return e;
    } else {
        if (int e = gemm_dx(dy, dy16, H, l.W2T, W2, t->gf, F, nullptr, (int)BT, F, H, s)) return e;
        if (int e = dropout_bwd_bias(l.u, t->gf, du, s16f, BT, F, plan.act_ew, layer_stream(i, 2), gb1, &b1_done, in, true)) return e;
    }
    if (int e = side(1, [&](hipStream_t st, float* rws) {
            return weight_grad(m, l.t2, du, (int)BT, H, F, G(b + "/feed_forward/intermediate_dense/kernel"), b1_done ? nullptr : gb1, st,
                               shb ? l.t2_16 : nullptr, s16f, s16f != nullptr, rws, &ws1);
        }))
        return e;
    return gemm_dx(du, s16f, F, l.W1T, W1, dx, H, res, (int)BT, H, F, s);
}

// d_o (the gradient of the out-projection's output) is read only as bf16 when both of its GEMMs stream shadows and its column sums come
// from the producer: the dropout backward that makes it then rides in the tail of the LayerNorm backward that produces dt1
bool BwdCtx::do16_only(const std::string& b) const {
    return shb && plan.attn16 && s16h && H % 128 == 0 && (BT * H) % 4 == 0 && dx_shadowed(m->P(b + "/attention/out_proj/kernel"));
}

// Attention branch of layer i, t1 = dropout(attn(attn_in) Wo + bo) + residual, for both norms: given dt1 (in tmp3) it leaves the eight
// attention gradients and dx = d loss / d attn_in (+ res, if given).  attn_in / attn_in16: what the q|k|v projection read (prenorm
// l.a / l.a16, postnorm hs[i] / hs16[i]).  do_tail: the LayerNorm backward that produced dt1 already left d_o's shadow in s16h and its
// column sums in the out-projection's bias gradient.  Scratch: d_o in tmp, dctx in tmp2 (the caller's earlier tenants are dead).
int BwdCtx::attn_branch_bwd(int i, LayerSave& l, const std::string& b, const float* dt1, const float* attn_in, const uint16_t* attn_in16,
                           bool do_tail, float* dx, const float* res) {
    const float* Wo = m->P(b + "/attention/out_proj/kernel");
    const WgSite ws2 = wg_site(2);
    const bool o16 = do16_only(b);
    float* const gbo = G(b + "/attention/out_proj/bias");
    bool bo_done = do_tail && gbo;
    float* d_o = tmp;
    if (!do_tail)
        if (int e = dropout_bwd_bias(nullptr, dt1, o16 ? nullptr : d_o, s16h, BT, H, 0, layer_stream(i, 1), gbo, &bo_done)) return e;
    float* dctx = tmp2;
    // (the bf16 attention backward reads dctx and q | k | v as bf16: the GEMM leaves the dctx shadow, the forward left qkv16)
    uint16_t* const dctx16 = (s16q && dx_shadowed(Wo)) ? t->dy16_ctx : nullptr;
    // (c16: the forward kept O only as bf16 -- dctx is then written only as bf16 too and the backward reads both as bf16)
    const bool c16 = plan.ctx16_only;
    W2V2_REQUIRE(!c16 || (dctx16 && shb), "train_backward: the forward kept the attention output as bf16 only, which needs the shadow paths");
    if (int e = gemm_dx(o16 ? nullptr : d_o, s16h, H, l.WoT, Wo, c16 ? nullptr : dctx, H, nullptr, (int)BT, H, H, s, dctx16)) return e;
    AttnTrain tr{p, seed, layer_stream(i, 0), l.lse, plan.attn16 ? l.keep_bits : nullptr};
    // dqkv only as bf16 (+ per-block column sums for the bias gradient) when all three of its readers can do without the fp32 copy
    const bool q16 = shb && s16q && plan.attn16 && t->attn_colpart && attn_in16 && H % 128 == 0 && dx_shadowed(m->qkv_w[i]);
    auto out_weight_grad = [&](hipStream_t st, float* rws) {
        return weight_grad(m, c16 ? nullptr : l.ctx, o16 ? nullptr : d_o, (int)BT, H, H, G(b + "/attention/out_proj/kernel"), bo_done ? nullptr : gbo, st,
                           (shb && plan.attn16) ? l.ctx16 : nullptr, s16h, s16h != nullptr, rws, &ws2);
    };
    // (side stream: the out-projection's weight gradient goes out BEFORE the attention backward, to run under it)
    if (side_on)
        if (int e = side(2, out_weight_grad)) return e;
    if (int e = side_wait(3)) return e;                  // (dqkv / its shadow / the column partials: the layer above's q|k|v weight gradient)
    AttnIO aio;
    aio.qkv = plan.attn16 ? nullptr : l.qkv; aio.qkv16 = plan.attn16 ? l.qkv16 : nullptr; aio.frame_len = flen; aio.train = &tr;
    aio.ctx = c16 ? nullptr : l.ctx; aio.ctx16 = c16 ? l.ctx16 : nullptr;
    aio.dctx = c16 ? nullptr : dctx; aio.dctx16 = dctx16;
    aio.dqkv = q16 ? nullptr : t->g3h; aio.dqkv16 = s16q; aio.dvec_ws = t->dvec; aio.colpart = q16 ? t->attn_colpart : nullptr;
    if (int e = launch_attention_bwd_routed(m->prof, plan.attn_bwd, aio, s)) return e;
    // (one stream: the out-projection's weight gradient runs here, not before its data gradient: the attention backward has just read O, so
    //  the GEMM finds it in the Infinity Cache instead of streaming it from HBM cold; d_o / its shadow are untouched until below)
    if (!side_on)
        if (int e = out_weight_grad(s, t->red_ws)) return e;
    if (int e = side(3, [&](hipStream_t st, float* rws) { return qkv_weight_grad(b, attn_in, attn_in16, q16, st, rws); })) return e;
    if (dx == d_o && !o16)
        if (int e = side_wait(2)) return e;              // (prenorm: dx goes where the fp32 d_o lives, which the out-projection's weight gradient reads)
    return gemm_dx(q16 ? nullptr : t->g3h, s16q, 3 * H, l.WqkvT, m->qkv_w[i], dx, H, res, (int)BT, H, 3 * H, s);
}

// ---- encoder layers N-1 .. 0 (buckets 1 .. N): dh = d loss / d (layer output) comes in and goes out in x.dh.  The two branch functions
// above do the work for both norms; the norm decides where the LayerNorm backward passes sit and which buffers they read and write ----
static int bwd_layers(BwdCtx& x) {
    w2v2_model* m = x.m;
    TrainState* t = x.t;
    const w2v2_config& c = m->cfg;
    const TrainPlan& plan = x.plan;
    const int H = x.H;
    const int64_t BT = x.BT;
    hipStream_t s = x.s;
    float *dh = x.dh, *tmp = x.tmp, *tmp2 = x.tmp2, *dt1 = x.tmp3;
    uint16_t* const s16h = x.s16h;
    const bool fuse_do_tail = !tune_int("W2V2_NO_DO_TAIL", 0);
    // prenorm: dh's bf16 shadow lives in s16h between layers (written by the pass that produced dh; s16h is free again by then) ...
    bool dh16_valid = x.head_dh16;
    // ... and b2_done: that pass (the encoder LayerNorm's backward for the top layer, the LayerNorm-1 backward of layer i + 1) also left
    // dh's column sums -- dh is the dY of this layer's down-projection, so they are its bias gradient -- and the weight gradient needs
    // no separate pass over the fp32 dh (two launches and a 98 MB read per layer at 16 x 480000)
    bool b2_done = x.head_b2 != nullptr;
    if (plan.prenorm && !dh16_valid && s16h && (BT * H) % 4 == 0 && (reinterpret_cast<uintptr_t>(dh) & 15) == 0) {
        // the last layer's output gradient arrives in fp32 only: round it once so that its down-projection GEMMs stream shadows too
        if (int e = launch_to_bf16(dh, s16h, BT * H, s)) return e;
        dh16_valid = true;
    }
    for (int i = c.num_layers - 1; i >= 0; --i) {
        const std::string b = "encoder/layers/" + std::to_string(i);
        LayerSave& l = t->layers[i];
        const bool keep = l.keep != 0.f;
        float* const gbo = x.G(b + "/attention/out_proj/bias");
        // (do_tail: d_o's shadow and column sums come from the LayerNorm backward that produces dt1 -- see do16_only)
        bool do_tail = x.do16_only(b) && fuse_do_tail;
        const LnDropTail do_drop{x.p, x.seed, layer_stream(i, 1)};
        float* const do_sum = do_tail ? (gbo ? gbo : t->dummy + 2 * H) : nullptr;
        float* dg1 = x.G(b + "/layer_norm/gamma");
        float* db1 = x.G(b + "/layer_norm/beta");
        float* dg2 = x.G(b + "/final_layer_norm/gamma");
        float* db2 = x.G(b + "/final_layer_norm/beta");
        if (plan.prenorm) {
            // prenorm layer (encoder.py:111-134):  t1 = x + drop(attn(LN1(x)));  out = t1 + keep * FFN(LN2(t1))
            const float* xin = i == 0 ? t->hs0 : m->hs[i];
            if (keep) {
                // the FFN's dY is dh itself; d LN2(t1) goes to tmp
                if (int e = x.ffn_branch_bwd(i, l, b, dh, dh16_valid ? s16h : nullptr, b2_done, tmp, nullptr)) return e;
                // dt1 = dh (residual) + LN2-backward(tmp), one pass (+ d_o's shadow and column sums where nothing reads d_o in fp32;
                // dh16 in s16h is dead by now -- once the down-projection's weight gradient has read it)
                if (int e = x.side_wait(0)) return e;
                if (int e = launch_ln_bwd_x(l.t1, m->P(b + "/final_layer_norm/gamma"), tmp, dt1, do_tail ? s16h : nullptr, dg2 ? dg2 : t->dummy,
                                            db2 ? db2 : t->dummy + H, BT, H, x.eps, x.ln2_ws, s, do_sum, dh, do_tail ? &do_drop : nullptr, x.fb))
                    return e;
            } else {
                W2V2_HIP_CHECK(hipMemcpyAsync(dt1, dh, (size_t)BT * H * 4, hipMemcpyDeviceToDevice, s));
                do_tail = false;
            }
            // d LN1(x) goes to tmp (where the fp32 d_o lived)
            if (int e = x.attn_branch_bwd(i, l, b, dt1, l.a, l.a16, do_tail, tmp, nullptr)) return e;
            // dh = dt1 (residual) + LN1-backward(tmp), one pass (+ the shadow the next iteration's down-projection GEMMs stream)
            dh16_valid = s16h && H % 4 == 0 && (reinterpret_cast<uintptr_t>(dt1) & 15) == 0;
            if (int e = x.side_wait(2)) return e;                  // (d_o's shadow in s16h: the out-projection's weight gradient)
            if (int e = x.side_wait(0)) return e;                  // (dh in fp32, when the down-projection's weight gradient read that)
            // (+ the column sums of dh: the down-projection bias gradient of layer i - 1, unless stochastic depth dropped that layer's FFN)
            float* const next_b2 = (x.shb && tune_int("W2V2_B2_FROM_LN", 1) != 0 && i > 0 && t->layers[i - 1].keep != 0.f)
                                       ? x.G("encoder/layers/" + std::to_string(i - 1) + "/feed_forward/output_dense/bias") : nullptr;
            if (int e = launch_ln_bwd_x(xin, m->P(b + "/layer_norm/gamma"), tmp, dh, dh16_valid ? s16h : nullptr, dg1 ? dg1 : t->dummy,
                                        db1 ? db1 : t->dummy + H, BT, H, x.eps, x.ln1_ws, s, next_b2, dt1, nullptr, x.fb))
                return e;
            b2_done = next_b2 != nullptr;
        } else {
            // postnorm layer:  t1 = x + drop(attn(x));  t2 = LN1(t1);  t3 = t2 + keep * FFN(t2);  out = LN2(t3)
            float *dt3 = tmp, *dt2 = tmp2;
            // (dt3 is the dY of the FFN down-projection: its column sums are that layer's bias gradient, its shadow goes to s16h)
            float* const gb2 = (x.shb && keep) ? x.G(b + "/feed_forward/output_dense/bias") : nullptr;
            uint16_t* const dt3_16 = (keep && H % 4 == 0) ? s16h : nullptr;
            if (int e = x.side_wait(2)) return e;                  // (tmp / s16h still hold the d_o the layer above's out-projection weight gradient reads)
            if (int e = launch_ln_bwd_x(l.t3, m->P(b + "/final_layer_norm/gamma"), dh, dt3, dt3_16, dg2 ? dg2 : t->dummy, db2 ? db2 : t->dummy + H, BT, H,
                                        x.eps, x.ln2_ws, s, gb2, nullptr, nullptr, x.fb))
                return e;
            if (keep) {
                // dt2 = d FFN input + dt3 (the residual branch)
                if (int e = x.ffn_branch_bwd(i, l, b, dt3, dt3_16, gb2 != nullptr, dt2, dt3)) return e;
            } else {
                W2V2_HIP_CHECK(hipMemcpyAsync(dt2, dt3, (size_t)BT * H * 4, hipMemcpyDeviceToDevice, s));
            }
            if (int e = x.side_wait(0)) return e;                  // (dt3 in tmp / s16h: the down-projection's weight gradient; d_o goes there next)
            if (int e = launch_ln_bwd_x(l.t1, m->P(b + "/layer_norm/gamma"), dt2, dt1, do_tail ? s16h : nullptr, dg1 ? dg1 : t->dummy,
                                        db1 ? db1 : t->dummy + H, BT, H, x.eps, x.ln1_ws, s, do_sum, nullptr, do_tail ? &do_drop : nullptr, x.fb))
                return e;
            // dh = d attention input + dt1 (residual); dt3 and dt2 are dead: d_o and dctx take their buffers
            const uint16_t* const hs16_i = m->hs16.size() > (size_t)i ? m->hs16[i] : nullptr;
            if (int e = x.attn_branch_bwd(i, l, b, dt1, m->hs[i], hs16_i, do_tail, dh, dt1)) return e;
        }
        if (int e = x.fold.flush(s)) return e;                 // (the layer's deferred folds: its gradients are final behind this launch)
        if (int e = x.bucket_done(c.num_layers - i)) return e;
    }
    return W2V2_OK;
}

// ---- encoder input, positional conv, spec-augment: x.dh = d loss / d hs[0] comes in, *dhd = d loss / d (dropped projection) goes out ----
static int bwd_encoder_input(BwdCtx& x, float** dhd) {
    w2v2_model* m = x.m;
    TrainState* t = x.t;
    const w2v2_config& c = m->cfg;
    Profiler* pf = m->prof;
    const int B = x.B, T = x.T, H = x.H;
    const int64_t BT = x.BT;
    hipStream_t s = x.s;
    float *dh = x.dh, *tmp = x.tmp, *tmp2 = x.tmp2, *tmp3 = x.tmp3;
    // (the scratch the layers' gradients flowed through is reused from here on, and the last weight gradient below shares the slabs)
    for (int k = 0; k < 4; ++k)
        if (int e = x.side_wait(k)) return e;
    // postnorm hs[0] = dropout(LN(posout));  prenorm hs0 = dropout(posout)
    float* dpos = tmp2;
    if (x.plan.prenorm) {
        if (int e = launch_dropout_bwd(nullptr, dh, dpos, BT * H, 0, x.p, x.seed, DS_ENCODER_IN, s)) return e;
    } else {
        if (int e = launch_dropout_bwd(nullptr, dh, tmp, BT * H, 0, x.p, x.seed, DS_ENCODER_IN, s)) return e;
        float* dg = x.G("encoder/layer_norm/gamma");
        float* db = x.G("encoder/layer_norm/beta");
        if (int e = launch_ln_bwd(m->posout, m->P("encoder/layer_norm/gamma"), tmp, dpos, dg ? dg : t->dummy, db ? db : t->dummy + H, BT, H,
                                  x.eps, t->red_ws, s))
            return e;
    }
    // ---- positional conv: posout = xz + GELU(c),  c = conv(xz; W_eff) + bias ----
    const int K = c.num_conv_pos_embeddings, Gr = c.num_conv_pos_embedding_groups, cg = H / Gr;
    float* dc = tmp;
    if (int e = launch_dropout_bwd(t->pos_c, dpos, dc, BT * H, x.plan.act_ew, 0.f, 0, 0, s)) return e;       // dc = dpos * GELU'(c)
    if (float* gb = x.G("encoder/pos_conv_embed/conv/bias"))
        if (int e = launch_colsum(dc, gb, BT, H, t->red_ws, 0, s)) return e;
    const float* enc_x = t->have_spec ? t->hm : t->hd;
    const float* xz = enc_x;
    if (x.flen) {
        if (int e = launch_mask_rows(enc_x, x.flen, tmp3, B, T, H, s)) return e;
        xz = tmp3;
    }
    float* gv = x.G("encoder/pos_conv_embed/conv/weight_v");
    float* gg = x.G("encoder/pos_conv_embed/conv/weight_g");
    if (gv || gg) {
        if (w2v2_pos_conv_bf16_ok(m) && B <= 64) {
            // mode bf16: batched transposed-A GEMM on the bf16 pipe (one (K cg, og) slab per sample and group, summed after);
            // the frames are padded to a multiple of 64 with zero rows of dc (T = 1499 at 480000 samples)
            const int Tk = (T + 63) / 64 * 64;
            if (!t->pos_pack32) {
                if (int e = t_alloc(t, &t->pos_pack32, (int64_t)B * (Tk + K - 1) * H)) return e;
                // (one (K cg, og) slab per group and per SLAB of samples: at most four since the samples are concatenated along K -- posconv.hip;
                //  the one-slab-per-sample form of the tools-only build keeps B of them)
                const int nslab = tune_int("W2V2_POS_DW_KCAT", 1) != 0 ? (B < 4 ? B : 4) : B;
                if (int e = t_alloc(t, &t->pos_dw_slabs, (int64_t)nslab * K * cg * H)) return e;
                if (Tk != T)
                    if (int e = t_alloc(t, &t->pos_dc_pad, (int64_t)B * Tk * H)) return e;
            }
            if (int e = launch_pos_conv_dw_bf16(pf, xz, dc, t->dwg, t->pos_pack32, t->pos_dw_slabs, t->red_ws, B, T, H, K, Gr, s, t->pos_dc_pad))
                return e;
        } else if (int e = launch_pos_conv_dw(pf, xz, dc, t->dwg, nullptr, B, T, H, K, Gr, s)) {
            return e;
        }
        float* gvd = gv ? gv : t->dwv_scratch;   // scratch targets when only one of the pair trains
        float* ggd = gg ? gg : t->dummy;
        if (int e = launch_weight_norm_bwd(m->P("encoder/pos_conv_embed/conv/weight_v"), m->P("encoder/pos_conv_embed/conv/weight_g"),
                                           t->dwg, gvd, ggd, K, cg, H, Gr, s))
            return e;
    }
    // dxz = dpos + conv^T(dc)   (transposed kernel, pad_left = K - 1 - K/2), then the frame mask
    float* dxz = dh;
    if (w2v2_pos_conv_bf16_ok(m) && m->pos_pack16) {
        if (!t->pos_w16_t) W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t->pos_w16_t), (size_t)K * cg * H * sizeof(uint16_t)));
        if (!t->pos_w16_t_fresh) {
            if (int e = launch_pos_conv_weight_shadow(t->pos_wg_t, t->pos_w16_t, K, cg, Gr, s)) return e;
            t->pos_w16_t_fresh = true;
        }
        if (int e = launch_pos_conv_bf16(pf, dc, t->pos_w16_t, nullptr, nullptr, dxz, nullptr, m->pos_pack16, nullptr, B, T, H, K, Gr, 0,
                                         K - 1 - K / 2, 0, s))
            return e;
    } else if (int e = launch_pos_conv_ex(pf, dc, t->pos_wg_t, nullptr, nullptr, dxz, nullptr, B, T, H, K, Gr, 0, K - 1 - K / 2, 0, s)) {
        return e;
    }
    if (int e = launch_axpby(dxz, dpos, dxz, BT * H, 1.f, 1.f, s)) return e;
    if (x.flen)
        if (int e = launch_mask_rows(dxz, x.flen, dxz, B, T, H, s)) return e;
    // ---- spec-augment ----
    *dhd = dxz;
    if (t->have_spec) {
        if (int e = launch_spec_aug_bwd(dxz, t->spec_mask, tmp, tmp2, BT, H, s)) return e;
        if (float* ge = x.G("masked_spec_embed"))
            if (int e = launch_colsum(tmp2, ge, BT, H, t->red_ws, 0, s)) return e;
        *dhd = tmp;
    }
    return W2V2_OK;
}

// ---- feature projection: hd = dropout(ln512 Wp + bp),  ln512 = LN(conv_out) ----
static int bwd_projection(BwdCtx& x, const float* dhd) {
    w2v2_model* m = x.m;
    TrainState* t = x.t;
    const w2v2_config& c = m->cfg;
    const int H = x.H;
    const int64_t BT = x.BT;
    hipStream_t s = x.s;
    float* dproj = x.tmp3;
    if (int e = launch_dropout_bwd(nullptr, dhd, dproj, BT * H, 0, x.p, x.seed, DS_FEATURE_PROJECTION, s)) return e;
    const int C = c.filter_sizes[c.num_conv_layers - 1];
    if (int e = weight_grad(m, m->ln512, dproj, (int)BT, C, H, x.G("feature_projection/projection/kernel"),
                            x.G("feature_projection/projection/bias"), s))
        return e;
    float* dgp = x.G("feature_projection/layer_norm/gamma");
    float* dbp = x.G("feature_projection/layer_norm/beta");
    if (dgp || dbp) {
        float* dln = x.tmp2;       // (BT, C) fits a (BT, H) buffer when C <= H; otherwise use the FFN scratch
        if (C > H) dln = t->gf;
        if (int e = x.gemm_dx(dproj, nullptr, H, t->WpT, m->P("feature_projection/projection/kernel"), dln, C, nullptr, (int)BT, C, H, s)) return e;
        float* dxc = C > H ? t->g3h : x.tmp;    // gradient w.r.t. the frozen conv output: computed and dropped
        if (int e = launch_ln_bwd(m->conv[c.num_conv_layers - 1], m->P("feature_projection/layer_norm/gamma"), dln, dxc,
                                  dgp ? dgp : t->dummy, dbp ? dbp : t->dummy + C, BT, C, x.eps, t->red_ws, s))
            return e;
    }
    return W2V2_OK;
}

static const char* precision_name(int p) {
    static const char* const names[] = {"fp32", "bf16", "bf16x3", "f16x2"};
    return p >= 0 && p < 4 ? names[p] : "?";
}

extern "C" {

int w2v2_train_backward(w2v2_model* m, const float* dlogits, void* stream) {
    W2V2_REQUIRE(m && dlogits, "train_backward: null argument");
    TrainState* t = m->train;
    if (!t || !t->forward_done) {
        set_error("train_backward: no training forward to differentiate");
        return W2V2_ESTATE;
    }
    const w2v2_config& c = m->cfg;
    const TrainPlan& plan = t->plan;
    // The saved activations are in the forms, and the saved lse in the domain, of the mode the forward ran in (TrainPlan): a backward in
    // another mode would read buffers that were never written, or a log2-domain lse as a natural one.  Refused before the first launch.
    if (m->precision != plan.precision || m->opt_shadows != plan.opt_shadows) {
        set_error("train_backward: the forward ran with precision %s, bf16_shadows %s; the model is now set to precision %s, bf16_shadows %s -- "
                  "restore the settings or run the forward again",
                  precision_name(plan.precision), plan.opt_shadows ? "on" : "off", precision_name(m->precision), m->opt_shadows ? "on" : "off");
        return W2V2_ESTATE;
    }
    const bool shb = plan.sh && m->w16_valid;
    // (a variable set between the forward and the backward invalidates the bf16 weight shadows the bf16-only activations depend on)
    W2V2_REQUIRE(!plan.ffn16_only || shb, "train_backward: a variable changed since the forward, which kept activations as bf16 only; run the forward again");
    for (size_t i = 0; i < m->params.size(); ++i)
        if (t->trainable[i] && m->params[i].name.compare(0, 18, "feature_extractor/") == 0) {
            set_error("train_backward: `%s` is trainable, but the conv feature extractor has no backward "
                      "(the reference freezes it, main.py:234-237); call freeze_feature_extractor()", m->params[i].name.c_str());
            return W2V2_ESTATE;
        }
    PrecisionScope precision(plan.precision);
    StepProfScope step_prof(m->prof);          // the training-only kernels' launchers find the profiler here (common.h)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    t->norm_fresh = false;                     // the OptStats of an earlier gradient say nothing about this one (w2v2_adamw_step)
    const int H = c.hidden_size, F = c.intermediate_size;
    const int64_t BT = plan.BT;
    BwdCtx x{m, t, plan, s, plan.B, plan.T, H, F, BT, c.layer_norm_eps, t->p, t->seed, t->have_mask ? m->frame_len : nullptr, shb,
             shb ? t->dy16_h : nullptr, shb ? t->dy16_f : nullptr, (shb && plan.attn_bwd.family == AF_BF16) ? t->dy16_3h : nullptr,
             t->gh[0], t->gh[1], t->gh[2], t->gh[3]};
    if (shb && BT % 64 != 0) {
        // Ragged row count: the weight-gradient GEMMs read the missing rows of their last K tile from the zero row behind each dY
        // shadow.  Re-assert the invariant on THIS stream every backward (three rows, a few KB): nothing may have padded into them.
        W2V2_HIP_CHECK(hipMemsetAsync(t->dy16_h + BT * H, 0, (size_t)H * 2, s));
        W2V2_HIP_CHECK(hipMemsetAsync(t->dy16_f + BT * F, 0, (size_t)F * 2, s));
        W2V2_HIP_CHECK(hipMemsetAsync(t->dy16_3h + BT * 3 * H, 0, (size_t)3 * H * 2, s));
    }
    // Gradient buffer at the start of a backward.  Rounds 1-5 zeroed all of it every step (360 MB / 1.25 GB: the runtime's fill kernels,
    // 0.23 / 0.8 ms per step and the only framework kernels left in it).  Every producer below STORES its gradient (no accumulation
    // into the buffer: folds, column sums and GEMM epilogues overwrite), so a slot needs zeros only if nothing will write it this time:
    //   * slots of variables that are not trainable, and the 16-byte padding between slots: zero since allocation, never written;
    //   * masked_spec_embed when this step has no spec-augment mask;
    //   * everything, conservatively, when the trainable set changed since the last backward (a slot that was written before keeps
    //     its last gradient) or when stochastic depth dropped a layer (its branch's gradients are not computed: zeros).
    // tests/test_train_gpu.py poisons the buffer with NaN before its gradient checks: a trainable slot nobody wrote shows up there.
    {
        uint64_t sig = 1469598103934665603ull;
        for (size_t i = 0; i < t->trainable.size(); ++i) sig = (sig ^ (uint64_t)(t->trainable[i] ? 0x9E : 0x3C)) * 1099511628211ull;
        bool dropped = false;
        for (int i = 0; i < c.num_layers; ++i) dropped = dropped || t->layers[i].keep == 0.f;
        if (sig != t->trainable_sig || dropped || t->grads_need_clear) {
            W2V2_HIP_CHECK(hipMemsetAsync(t->grads, 0, (size_t)t->gtotal * 4, s));
            t->trainable_sig = sig;
            t->grads_need_clear = dropped;        // (the step after a dropped layer starts from zeros as well: its slots hold nothing new)
        } else if (!t->have_spec) {
            auto it = m->index.find("masked_spec_embed");
            if (it != m->index.end() && t->trainable[it->second])
                W2V2_HIP_CHECK(hipMemsetAsync(t->grads + t->goff[it->second], 0, (size_t)m->params[it->second].numel * 4, s));
        }
    }
    if (int e = refresh_transposes(m, s)) return e;
    const int nbuckets = c.num_layers + 2;
    while ((int)t->bucket_ev.size() < nbuckets) {
        hipEvent_t ev;
        W2V2_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        t->bucket_ev.push_back(ev);
    }
    // ---- weight-gradient side stream (TrainState::wg_stream): the bf16 shadow path only -- there every dY a weight gradient reads is a
    // shadow with a known next writer (the wait points of the stages); the other paths keep one stream.
    // (tools-only build: W2V2_WGRAD_STREAM = 0 / 1 overrides the option for A/B runs)
    const int wg_knob = tune_int("W2V2_WGRAD_STREAM", -1);
    x.side_on = shb && plan.attn16 && t->attn_colpart && (wg_knob < 0 ? m->opt_wgrad_stream : wg_knob != 0);
    if (x.side_on && !t->wg_stream) {
        int lo = 0, hi = 0;
        W2V2_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));           // (lo = the numerically largest = least urgent)
        W2V2_HIP_CHECK(hipStreamCreateWithPriority(&t->wg_stream, hipStreamNonBlocking, lo));
        W2V2_HIP_CHECK(hipEventCreateWithFlags(&t->wg_fork, hipEventDisableTiming));
        W2V2_HIP_CHECK(hipEventCreateWithFlags(&t->wg_main, hipEventDisableTiming));
        for (int k = 0; k < 4; ++k) W2V2_HIP_CHECK(hipEventCreateWithFlags(&t->wg_join[k], hipEventDisableTiming));
    }
    // Deferred folds of the encoder layers (W2V2_OPT_DEFER_FOLDS).  The side stream keeps the folds behind their GEMMs: its weight
    // gradients run ahead of / behind the main stream's position.
    // (tools-only build: W2V2_DEFER_FOLDS = 0 none, 1 the column-sum folds only -- slab sums behind their GEMMs --, 2 everything.
    //  One box, arms interleaved, profiles/r05_ab_defer_folds.txt: base step 33.80 / 33.55 / 33.50 ms, large-robust 98.38 / 97.94 / 97.74)
    x.defer_mode = (!x.side_on && m->opt_defer_folds) ? tune_int("W2V2_DEFER_FOLDS", 2) : 0;
    if (x.defer_mode != 0) x.fb = &x.fold;
    if (int e = ensure_site_scratch(m, x.side_on, x.defer_mode != 0, x.defer_mode == 2)) return e;
    x.ln2_ws = x.fb ? t->site_ws[0] : t->red_ws;
    x.ln1_ws = x.fb ? t->site_ws[2] : t->red_ws;
    // does anything below the head train?
    bool below_head = false;
    for (size_t i = 0; i < m->params.size(); ++i)
        if (t->trainable[i] && m->params[i].name.compare(0, 8, "lm_head/") != 0) below_head = true;

    if (int e = bwd_head(x, dlogits, below_head)) return e;
    if (!below_head) {                          // stage 1 of the reference: only lm_head trains (main.py:210)
        for (int k = 1; k < nbuckets; ++k)
            if (int e = x.bucket_done(k)) return e;
        return W2V2_OK;
    }
    if (int e = bwd_layers(x)) return e;
    float* dhd = nullptr;
    if (int e = bwd_encoder_input(x, &dhd)) return e;
    if (int e = bwd_projection(x, dhd)) return e;
    return x.bucket_done(nbuckets - 1);
}


/* Gradient buckets: slices of the flat buffer in the order the backward completes them.  Data-parallel callers enqueue
 * one all-reduce per bucket on a communication stream that waits (w2v2_train_bucket_wait) for that bucket only, so the
 * collectives of the upper layers run under the backward of the lower ones. */
int w2v2_train_storage(const w2v2_model* m, int32_t* mask, int64_t* workspace_bytes) {
    W2V2_REQUIRE(m && mask && workspace_bytes, "train_storage: null argument");
    const TrainState* t = m->train;
    *mask = 0;
    *workspace_bytes = t ? t->alloc_bytes : 0;
    if (t && t->B > 0)
        *mask = storage_mask(t->plan);
    return W2V2_OK;
}

int w2v2_train_num_buckets(const w2v2_model* m) { return m ? m->cfg.num_layers + 2 : W2V2_EINVAL; }

int w2v2_train_bucket(w2v2_model* m, int32_t k, int64_t* offset, int64_t* numel) {
    W2V2_REQUIRE(m && offset && numel, "train_bucket: null argument");
    TrainState* t = get_state(m);
    const int nl = m->cfg.num_layers, nb = nl + 2;
    W2V2_REQUIRE(k >= 0 && k < nb, "train_bucket: bucket %d outside [0, %d)", k, nb);
    // inventory order: [front: everything before encoder/layers/0][layers 0 .. N-1][lm_head]
    auto first_with = [&](const std::string& prefix) -> int64_t {
        for (size_t i = 0; i < m->params.size(); ++i)
            if (m->params[i].name.compare(0, prefix.size(), prefix) == 0) return t->goff[i];
        return t->gtotal;
    };
    auto layer_begin = [&](int i) { return i < nl ? first_with("encoder/layers/" + std::to_string(i) + "/") : first_with("lm_head/"); };
    int64_t lo, hi;
    if (k == 0) { lo = first_with("lm_head/"); hi = t->gtotal; }
    else if (k <= nl) { const int i = nl - k; lo = layer_begin(i); hi = layer_begin(i + 1); }
    else { lo = 0; hi = layer_begin(0); }
    W2V2_REQUIRE(lo <= hi, "train_bucket: the variable inventory is not in [front | layers | lm_head] order");
    *offset = lo;
    *numel = hi - lo;
    return W2V2_OK;
}

/* Slot of one variable in the flat gradient / Adam buffers (16-byte aligned slots, inventory order). */
int w2v2_grad_slot(w2v2_model* m, const char* name, int64_t* offset, int64_t* numel) {
    W2V2_REQUIRE(m && name && offset && numel, "grad_slot: null argument");
    TrainState* t = get_state(m);
    auto it = m->index.find(name);
    if (it == m->index.end()) {
        set_error("grad_slot: unknown variable `%s`", name);
        return W2V2_ENOTFOUND;
    }
    *offset = t->goff[it->second];
    *numel = m->params[it->second].numel;
    return W2V2_OK;
}

int w2v2_train_bucket_wait(w2v2_model* m, int32_t k, void* stream) {
    W2V2_REQUIRE(m && m->train, "train_bucket_wait: no training state");
    TrainState* t = m->train;
    W2V2_REQUIRE(k >= 0 && k < (int)t->bucket_ev.size(), "train_bucket_wait: bucket %d has not been produced yet (run a backward first)", k);
    W2V2_HIP_CHECK(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), t->bucket_ev[k], 0));
    return W2V2_OK;
}

/* A fresh optimizer: the reference builds a new tf.keras.optimizers.Adam for each stage (src/main.py:213,240), i.e. zero
 * moments and iteration 0.  The moments live here (not in the Python Trainer), so a new Trainer on a used model resets them. */
int w2v2_adam_reset(w2v2_model* m, void* stream) {
    W2V2_REQUIRE(m, "adam_reset: null model");
    if (int e = ensure_persistent(m)) return e;
    TrainState* t = m->train;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    W2V2_HIP_CHECK(hipMemsetAsync(t->adam_m, 0, (size_t)t->gtotal * 4, s));
    W2V2_HIP_CHECK(hipMemsetAsync(t->adam_v, 0, (size_t)t->gtotal * 4, s));
    if (t->opt_stats) W2V2_HIP_CHECK(hipMemsetAsync(&t->opt_stats->skipped_total, 0, sizeof(int64_t), s));   // a fresh optimizer has skipped nothing
    return W2V2_OK;
}

/* Adam's first / second moment buffers (flat, the gradient buffer's layout) for checkpoint / resume. */
int w2v2_adam_buffers(w2v2_model* m, float** m_dev, float** v_dev, int64_t* numel) {
    W2V2_REQUIRE(m && m_dev && v_dev && numel, "adam_buffers: null argument");
    if (int e = ensure_persistent(m)) return e;        // the moments do not depend on the batch shape: no forward needed
    TrainState* t = m->train;
    *m_dev = t->adam_m;
    *v_dev = t->adam_v;
    *numel = t->gtotal;
    return W2V2_OK;
}

int w2v2_grad_buffer(w2v2_model* m, float** dev_ptr, int64_t* numel) {
    W2V2_REQUIRE(m && dev_ptr && numel, "grad_buffer: null argument");
    if (int e = ensure_persistent(m)) return e;
    TrainState* t = m->train;
    *dev_ptr = t->grads;
    *numel = t->gtotal;
    return W2V2_OK;
}

int w2v2_get_grad(w2v2_model* m, const char* name, float* host_dst, int64_t numel, void* stream) {
    W2V2_REQUIRE(m && name && host_dst, "get_grad: null argument");
    TrainState* t = m->train;
    if (!t || !t->grads) {
        set_error("get_grad: run a training forward/backward first");
        return W2V2_ESTATE;
    }
    auto it = m->index.find(name);
    if (it == m->index.end()) {
        set_error("get_grad: unknown variable `%s`", name);
        return W2V2_ENOTFOUND;
    }
    W2V2_REQUIRE(numel == m->params[it->second].numel, "get_grad: element count mismatch for `%s`", name);
    W2V2_HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    W2V2_HIP_CHECK(hipMemcpy(host_dst, t->grads + t->goff[it->second], (size_t)numel * 4, hipMemcpyDeviceToHost));
    return W2V2_OK;
}

// The device table of trainable 4096-element chunks every optimizer kernel runs over; rebuilt when the trainable set or the decay
// flags changed.
static int ensure_chunk_table(w2v2_model* m, TrainState* t) {
    if (t->adam_table_fresh) return W2V2_OK;
    std::vector<AdamChunk> host;
    for (size_t i = 0; i < m->params.size(); ++i) {
        if (!t->trainable[i]) continue;
        const Param& p = m->params[i];
        const int decay = !t->decay.empty() && t->decay[i];
        for (int64_t o = 0; o < p.numel; o += 4096)
            host.push_back(AdamChunk{p.dev + o, t->goff[i] + o, (int)(p.numel - o < 4096 ? p.numel - o : 4096), decay});
    }
    if (t->adam_chunks) (void)hipFree(t->adam_chunks);
    t->adam_chunks = nullptr;
    t->adam_nchunks = (int)host.size();
    if (!host.empty()) {
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t->adam_chunks), host.size() * sizeof(AdamChunk)));
        W2V2_HIP_CHECK(hipMemcpy(t->adam_chunks, host.data(), host.size() * sizeof(AdamChunk), hipMemcpyHostToDevice));
    }
    t->adam_table_fresh = true;
    return W2V2_OK;
}

int w2v2_adam_step(w2v2_model* m, float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
    W2V2_REQUIRE(m && step >= 1, "adam_step: bad argument");
    TrainState* t = m->train;
    if (!t || !t->grads) {
        set_error("adam_step: no gradients");
        return W2V2_ESTATE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StepProfScope step_prof(m->prof);
    // Keras: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t);  p -= lr_t * m / (sqrt(v) + eps)
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    if (int e = ensure_chunk_table(m, t)) return e;
    if (t->adam_nchunks > 0)
        if (int e = launch_adam_multi(t->adam_chunks, t->adam_nchunks, t->grads, t->adam_m, t->adam_v, (float)lr_t, beta1, beta2, eps, s))
            return e;
    t->transposes_fresh = false;
    m->finalized = false;
    return w2v2_finalize(m, stream);     // re-derive the effective positional kernel and the packed q|k|v
}

/* ---- accumulation, global-norm clipping, AdamW, skipped steps ---- */

int w2v2_set_decay_flags(w2v2_model* m, const uint8_t* flags, int32_t n) {
    W2V2_REQUIRE(m && flags, "set_decay_flags: null argument");
    W2V2_REQUIRE(n == (int32_t)m->params.size(), "set_decay_flags: %d flags for %d variables", n, (int)m->params.size());
    TrainState* t = get_state(m);
    if (t->decay.empty()) t->decay.assign(m->params.size(), 0);
    bool changed = false;
    for (int32_t i = 0; i < n; ++i) {
        const char f = flags[i] ? 1 : 0;
        changed |= t->decay[i] != f;
        t->decay[i] = f;
    }
    if (changed) t->adam_table_fresh = false;
    return W2V2_OK;
}

// the gradient buffer and the chunk table of a model that has run a backward
static int optimizer_ready(w2v2_model* m, const char* who, TrainState** out) {
    TrainState* t = m ? m->train : nullptr;
    if (!t || !t->grads) {
        set_error("%s: no gradients", who);
        return W2V2_ESTATE;
    }
    *out = t;
    return ensure_chunk_table(m, t);
}

int w2v2_grad_accumulate(w2v2_model* m, int32_t mode, void* stream) {
    W2V2_REQUIRE(m && mode >= W2V2_ACCUM_STORE && mode <= W2V2_ACCUM_FINISH, "grad_accumulate: bad argument");
    TrainState* t = nullptr;
    if (int e = optimizer_ready(m, "grad_accumulate", &t)) return e;
    if (!t->grad_acc) {
        W2V2_REQUIRE(mode == W2V2_ACCUM_STORE, "grad_accumulate: nothing has been stored yet (the first micro-step is W2V2_ACCUM_STORE)");
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t->grad_acc), (size_t)t->gtotal * 4));
        W2V2_HIP_CHECK(hipMemset(t->grad_acc, 0, (size_t)t->gtotal * 4));     // (a slot that turns trainable inside an accumulation adds zeros)
    }
    if (mode == W2V2_ACCUM_FINISH) t->norm_fresh = false;      // the gradient changes under an earlier norm
    if (t->adam_nchunks == 0) return W2V2_OK;
    StepProfScope step_prof(m->prof);
    return launch_grad_accumulate(t->adam_chunks, t->adam_nchunks, t->grads, t->grad_acc, mode, reinterpret_cast<hipStream_t>(stream));
}

static int ensure_opt_stats(TrainState* t) {
    if (!t->opt_stats) {
        const OptStats zero{0.0, 0.f, 1.f, 0, 0, 0};
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t->opt_stats), sizeof(OptStats)));
        W2V2_HIP_CHECK(hipMemcpy(t->opt_stats, &zero, sizeof(OptStats), hipMemcpyHostToDevice));
    }
    return W2V2_OK;
}

int w2v2_grad_norm(w2v2_model* m, float max_norm, int32_t skip_nonfinite, void* stream) {
    W2V2_REQUIRE(m, "grad_norm: null model");
    TrainState* t = nullptr;
    if (int e = optimizer_ready(m, "grad_norm", &t)) return e;
    W2V2_REQUIRE(t->adam_nchunks > 0, "grad_norm: no variable is trainable");
    if (int e = ensure_opt_stats(t)) return e;
    if (t->norm_cap < t->adam_nchunks) {
        // (freeing synchronises with the kernels that may still read the old scratch; the table changes between stages, not steps)
        if (t->norm_partial) (void)hipFree(t->norm_partial);
        t->norm_partial = nullptr;
        t->norm_cap = 0;
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t->norm_partial), (size_t)t->adam_nchunks * (sizeof(double) + sizeof(int32_t))));
        t->norm_cap = t->adam_nchunks;
    }
    StepProfScope step_prof(m->prof);
    if (int e = launch_grad_norm(t->adam_chunks, t->adam_nchunks, t->grads, 0, t->norm_partial,
                                 reinterpret_cast<int32_t*>(t->norm_partial + t->norm_cap), max_norm, skip_nonfinite ? 1 : 0, t->opt_stats,
                                 reinterpret_cast<hipStream_t>(stream)))
        return e;
    t->norm_fresh = true;
    return W2V2_OK;
}

int w2v2_adamw_step(w2v2_model* m, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
    W2V2_REQUIRE(m && step >= 1 && weight_decay >= 0.f, "adamw_step: bad argument");
    TrainState* t = nullptr;
    if (int e = optimizer_ready(m, "adamw_step", &t)) return e;
    if (!t->norm_fresh) {
        set_error("adamw_step: no w2v2_grad_norm since the last backward (it leaves the clip factor and the skip decision this call reads)");
        return W2V2_ESTATE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StepProfScope step_prof(m->prof);
    // lr_t as in w2v2_adam_step; t counts the calls, skipped ones included (the host does not know the skip: DESIGN 22)
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    if (int e = launch_adamw_multi(t->adam_chunks, t->adam_nchunks, t->grads, t->adam_m, t->adam_v, t->opt_stats, lr, weight_decay, (float)lr_t,
                                   beta1, beta2, eps, s))
        return e;
    t->transposes_fresh = false;
    m->finalized = false;
    return w2v2_finalize(m, stream);
}

int w2v2_optimizer_stats(w2v2_model* m, float* norm, float* scale, int32_t* skipped_last, int64_t* skipped_total, void* stream) {
    W2V2_REQUIRE(m && norm && scale && skipped_last && skipped_total, "optimizer_stats: null argument");
    OptStats st{0.0, 0.f, 1.f, 0, 0, 0};
    if (m->train && m->train->opt_stats) {
        W2V2_HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
        W2V2_HIP_CHECK(hipMemcpy(&st, m->train->opt_stats, sizeof(OptStats), hipMemcpyDeviceToHost));
    }
    *norm = st.norm;
    *scale = st.scale;
    *skipped_last = st.skip;
    *skipped_total = st.skipped_total;
    return W2V2_OK;
}

}  // extern "C"

// What a data-parallel SUM all-reduce of bucket k has to send (comm.hip; the host-side mirror is wav2vec2/dist.py::trainable_ranges):
// the runs of trainable slots, adjacent slots merged (a slot is its variable rounded up to 4 floats; the padding rides along, it is
// zero on every rank).  Frozen slots -- the conv stack in stage 2 (main.py:234-237), everything but lm_head in stage 1 -- stay home.
int w2v2_train_trainable_runs(w2v2_model* m, int k, std::vector<std::pair<int64_t, int64_t>>* runs, float** grads) {
    W2V2_REQUIRE(m && runs, "trainable_runs: null argument");
    int64_t lo = 0, n = 0;
    if (int e = w2v2_train_bucket(m, k, &lo, &n)) return e;
    if (int e = ensure_persistent(m)) return e;
    TrainState* t = m->train;
    const int64_t hi = lo + n;
    runs->clear();
    for (size_t i = 0; i < m->params.size(); ++i) {
        const int64_t off = t->goff[i];
        if (off < lo || off >= hi || !t->trainable[i]) continue;
        int64_t end = off + ((m->params[i].numel + 3) & ~(int64_t)3);
        if (end > hi) end = hi;
        if (!runs->empty() && runs->back().first + runs->back().second == off) runs->back().second = end - runs->back().first;
        else runs->emplace_back(off, end - off);
    }
    if (grads) *grads = t->grads;
    return W2V2_OK;
}

