// The inference forward (w2v2_forward, w2v2_forward_packed, w2v2_forward_windows): the forward plan, the extractor + projection
// stage it shares with the training forward, and the buffers / weight images its precision modes need.  Host code only.
//
// Forward order follows the reference exactly: Wav2Vec2ForCTC.call
// (modeling.py:239-255) -> Wav2Vec2Model.call (modeling.py:169-209) ->
// FeatureExtractorLayer x7 (feature_extractor.py:54-59) -> FeatureProjection
// (feature_extractor.py:92-95) -> Wav2Vec2Encoder.call (encoder.py:251-276) ->
// TransformerLayer.call (encoder.py:111-134) -> lm_head.
#include <algorithm>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "model.h"

using namespace w2v2;

static constexpr unsigned F32 = ForwardPlan::F32, B16 = ForwardPlan::B16, PLANES = ForwardPlan::PLANES;

// ---- bf16 shadows for the forward in precision mode 1 -----------------------------------------------------------------------------
// Every producer of a GEMM operand also writes its nearest-even bf16 copy, the GEMMs stream those (2 bytes per element, no
// conversion) and the weights come from (N, K) bf16 shadows.  w2v2_set_option(m, W2V2_OPT_BF16_SHADOWS, 0) turns them off (every
// GEMM then rounds its fp32 operands itself): same results bit for bit, used by the tests to prove exactly that.
//
// A conv-stack output whose only consumer is the next layer's GEMM reading the bf16 shadow is written ONLY as bf16 -- 6.3 GB of fp32
// stores per B = 32 x 246000 forward that nothing would read: in group-norm mode by the GEMM epilogue, in LayerNorm mode (robust /
// xlsr) by the LN + GELU pass (the GEMM's own fp32 output is that pass's input and stays).  Stage taps of those tensors
// (w2v2_copy_activation) then report an error; W2V2_OPT_KEEP_ACTIVATIONS keeps the fp32 copies.  (m->conv_T: the shadows exist only
// in the dense forwards, whose workspace is exactly the input's.)
bool w2v2_conv_bf16_only(const w2v2_model* m, int i, bool sh) {
    const w2v2_config& c = m->cfg;
    if (!sh || i + 1 >= c.num_conv_layers || m->opt_keep_acts) return false;
    const int64_t cin = c.filter_sizes[i];
    return gemm_bf16_streams_a16(c.kernal_sizes[i + 1] * (int)cin, (int64_t)c.strides[i + 1] * cin, (int64_t)m->conv_T[i] * cin);
}

static int sh_alloc(std::vector<void*>& pool, uint16_t** out, int64_t n) {
    void* p = nullptr;
    W2V2_HIP_CHECK(hipMalloc(&p, (size_t)(n > 0 ? n : 1) * sizeof(uint16_t)));
    pool.push_back(p);
    *out = reinterpret_cast<uint16_t*>(p);
    return W2V2_OK;
}

int w2v2_ensure_shadows(w2v2_model* m, int B, int T, hipStream_t s) {
    const w2v2_config& c = m->cfg;
    const int64_t H = c.hidden_size, F = c.intermediate_size, BT = (int64_t)B * T;
    if (!m->sh_ready) {
        for (int i = 0; i + 1 < c.num_conv_layers; ++i) {       // the last conv output feeds a LayerNorm, not a GEMM
            uint16_t* p = nullptr;
            if (int e = sh_alloc(m->sh_allocs, &p, (int64_t)B * m->conv_T[i] * c.filter_sizes[i])) return e;
            m->conv16.push_back(p);
        }
        if (int e = sh_alloc(m->sh_allocs, &m->ln512_16, BT * c.filter_sizes[c.num_conv_layers - 1])) return e;
        for (int i = 0; i <= c.num_layers; ++i) {
            uint16_t* p = nullptr;
            if (int e = sh_alloc(m->sh_allocs, &p, BT * H)) return e;
            m->hs16.push_back(p);
        }
        if (int e = sh_alloc(m->sh_allocs, &m->ctx16, BT * H)) return e;
        if (int e = sh_alloc(m->sh_allocs, &m->qkv16, BT * 3 * H)) return e;
        if (int e = sh_alloc(m->sh_allocs, &m->t0_16, BT * H)) return e;
        if (int e = sh_alloc(m->sh_allocs, &m->t2_16, BT * H)) return e;
        if (int e = sh_alloc(m->sh_allocs, &m->ffn16, BT * F)) return e;
        if (int e = sh_alloc(m->sh_allocs, &m->enc16, BT * H)) return e;
        m->sh_ready = true;
    }
    if (!m->w16_valid) {
        // (re)build the job table when it does not exist yet or the plain copies have become necessary (training started)
        const bool want_plain = m->train != nullptr;
        if (!m->shadow_jobs || (want_plain && !m->shadow_jobs_train)) {
            std::vector<ShadowJob> jobs;
            auto shadow = [&](const float* w, int K, int N) -> int {
                uint16_t*& dst = m->w16[w];
                if (!dst)
                    if (int e = sh_alloc(m->w16_allocs, &dst, (int64_t)K * N)) return e;
                uint16_t* plain = nullptr;
                if (want_plain && N % 64 == 0 && (K * (int64_t)N) % 4 == 0) {     // training: the backward's dX GEMM contracts over N
                    uint16_t*& dp = m->w16p[w];
                    if (!dp)
                        if (int e = sh_alloc(m->w16_allocs, &dp, (int64_t)K * N)) return e;
                    plain = dp;
                }
                for (int k0 = 0; k0 < K; k0 += 64)
                    for (int n0 = 0; n0 < N; n0 += 64) jobs.push_back(ShadowJob{w, dst, plain, K, N, k0, n0});
                return W2V2_OK;
            };
            for (int i = 1; i < c.num_conv_layers; ++i)
                if (int e = shadow(m->P("feature_extractor/conv_layers/" + std::to_string(i) + "/conv/kernel"),
                                   c.kernal_sizes[i] * c.filter_sizes[i - 1], c.filter_sizes[i]))
                    return e;
            if (int e = shadow(m->P("feature_projection/projection/kernel"), c.filter_sizes[c.num_conv_layers - 1], (int)H)) return e;
            for (int i = 0; i < c.num_layers; ++i) {
                const std::string b = "encoder/layers/" + std::to_string(i);
                if (int e = shadow(m->qkv_w[i], (int)H, 3 * (int)H)) return e;
                if (int e = shadow(m->P(b + "/attention/out_proj/kernel"), (int)H, (int)H)) return e;
                if (int e = shadow(m->P(b + "/feed_forward/intermediate_dense/kernel"), (int)H, (int)F)) return e;
                if (int e = shadow(m->P(b + "/feed_forward/output_dense/kernel"), (int)F, (int)H)) return e;
            }
            if (c.with_lm_head)
                if (int e = shadow(m->P("lm_head/kernel"), (int)H, c.vocab_size)) return e;
            if (m->shadow_jobs) W2V2_HIP_CHECK(hipFree(m->shadow_jobs));
            m->shadow_jobs = nullptr;
            W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->shadow_jobs), jobs.size() * sizeof(ShadowJob)));
            W2V2_HIP_CHECK(hipMemcpy(m->shadow_jobs, jobs.data(), jobs.size() * sizeof(ShadowJob), hipMemcpyHostToDevice));
            m->shadow_njobs = (int)jobs.size();
            m->shadow_jobs_train = want_plain;
        }
        if (int e = launch_weight_shadows_multi(m->shadow_jobs, m->shadow_njobs, s)) return e;
        m->w16_valid = true;
    }
    return W2V2_OK;
}

// ---- precision modes 2 / 3: operand planes (gemm_split_sw.hip) ----------------------------------------------------------------
int w2v2_ensure_planes(w2v2_model* m, int B, int64_t L, int fmt) {
    if (m->pl_fmt == fmt && m->pl_B == B && m->pl_L == L) return W2V2_OK;
    w2v2_free_planes(m);
    const w2v2_config& c = m->cfg;
    const int np = plane_count(fmt);
    auto alloc = [&](w2v2_model::PlaneBuf& b, int64_t elems) -> int {
        b.plane = (elems + 7) & ~(int64_t)7;                 // 16-byte aligned planes
        void* p = nullptr;
        W2V2_HIP_CHECK(hipMalloc(&p, (size_t)b.plane * np * sizeof(uint16_t)));
        m->pl_allocs.push_back(p);
        b.p = reinterpret_cast<uint16_t*>(p);
        return W2V2_OK;
    };
    const int NC = c.num_conv_layers;
    m->conv48.resize(NC > 1 ? NC - 1 : 0);
    for (int i = 0; i + 1 < NC; ++i)
        if (int e = alloc(m->conv48[i], (int64_t)B * m->conv_T[i] * c.filter_sizes[i])) return e;
    const int64_t BT = (int64_t)B * m->conv_T[NC - 1], H = c.hidden_size;
    if (int e = alloc(m->ln512_48, BT * c.filter_sizes[NC - 1])) return e;
    if (int e = alloc(m->attn_in48, BT * H)) return e;
    if (int e = alloc(m->ctx48, BT * H)) return e;
    if (int e = alloc(m->ffn_in48, BT * H)) return e;
    if (int e = alloc(m->ffn48, BT * c.intermediate_size)) return e;
    if (!m->range_flag) {
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->range_flag), sizeof(int)));
        W2V2_HIP_CHECK(hipMemset(m->range_flag, 0, sizeof(int)));
    }
    m->pl_fmt = fmt;
    m->pl_B = B;
    m->pl_L = L;
    return W2V2_OK;
}

int w2v2_split_images(w2v2_model* m, const float* W, int K, int N, int fmt, hipStream_t s, const uint16_t** img, const float** out_scale) {
    W2V2_REQUIRE(W && (fmt == PF_BF16X3 || fmt == PF_F16X2), "split_images: bad argument");
    w2v2_model::SplitImages& e = m->wimg[fmt][W];
    const int64_t elems = (int64_t)plane_count(fmt) * K * N;
    if (!e.img || e.elems != elems) {
        if (e.img) (void)hipFree(e.img);
        e.img = nullptr;
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e.img), (size_t)elems * sizeof(uint16_t)));
        if (!e.scale_ws) W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e.scale_ws), 2 * sizeof(float)));
        e.elems = elems;
        e.epoch = 0;
    }
    if (e.epoch != m->w48_epoch) {
        if (int err = launch_split_weight_sw(W, e.img, K, N, fmt, e.scale_ws, s)) return err;
        e.epoch = m->w48_epoch;
    }
    *img = e.img;
    *out_scale = fmt == PF_F16X2 ? e.scale_ws + 1 : nullptr;
    return W2V2_OK;
}

bool w2v2_use_split_gemm(const w2v2_model* m, const float* A, int64_t lda, int64_t strideA, int64_t ldb, int M, int N, int K, int nbatch) {
    // (precision mode 3 falls back to this six-product kernel for the shapes / call sites its plane-fed kernel does not serve)
    if (m->precision < W2V2_PRECISION_BF16X3 || ldb != N || N % 256 != 0) return false;
    if (tune_int("W2V2_SPLIT_GEMM", 1) == 0) return false;      // (tools-only: tools/nll_drift_probe.py separates the GEMMs from the attention)
    // (below ~half a wave of 128 x 256 tiles the fp32 path's small tiles and split-K serve a single utterance better)
    const int64_t split_tiles = (int64_t)((M + 127) / 128) * (N / 256) * nbatch;
    return split_tiles >= 128 && gemm_split_supported(A, lda, strideA, M, N, K);
}

int w2v2_split_planes(w2v2_model* m, const float* W, int K, int N, hipStream_t s, const uint16_t** planes) {
    w2v2_model::SplitPlanes& e = m->w48[W];
    const int64_t need = 3 * (int64_t)K * N;
    if (!e.p || e.elems != need) {
        if (e.p) W2V2_HIP_CHECK(hipFree(e.p));
        e.p = nullptr;
        W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e.p), (size_t)need * sizeof(uint16_t)));
        e.elems = need;
        e.epoch = 0;
    }
    if (e.epoch != m->w48_epoch) {
        if (int err = launch_split_weight(W, e.p, K, N, s)) return err;
        e.epoch = m->w48_epoch;
    }
    *planes = e.p;
    return W2V2_OK;
}

bool w2v2_pos_conv_bf16_ok(const w2v2_model* m) {
    const int cg = m->cfg.hidden_size / m->cfg.num_conv_pos_embedding_groups;
    return m->precision == 1 && cg % 8 == 0 && cg <= 64 && (m->cfg.num_conv_pos_embeddings * cg) % 64 == 0;
}

// the bf16 shadow of the regrouped positional-conv kernel (both the dense and the packed bf16 positional conv read it)
static int ensure_pos_w16(w2v2_model* m, hipStream_t s) {
    const w2v2_config& c = m->cfg;
    const int H = c.hidden_size, K = c.num_conv_pos_embeddings, G = c.num_conv_pos_embedding_groups, cg = H / G;
    if (!m->pos_w16) W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->pos_w16), (size_t)K * cg * H * sizeof(uint16_t)));
    if (!m->pos16_valid) {
        if (int e = launch_pos_conv_weight_shadow(m->pos_wg, m->pos_w16, K, cg, G, s)) return e;
        m->pos16_valid = true;
    }
    return W2V2_OK;
}

int w2v2_ensure_pos16(w2v2_model* m, int B, int T, hipStream_t s) {
    const w2v2_config& c = m->cfg;
    const int H = c.hidden_size, K = c.num_conv_pos_embeddings;
    if (int e = ensure_pos_w16(m, s)) return e;
    if (!m->pos_pack16) {
        float* p = nullptr;
        if (int e = w2v2_ws_alloc(m, &p, (pos_conv_bf16_pack_elems(B, T, H, K) + 1) / 2 + 4)) return e;
        m->pos_pack16 = reinterpret_cast<uint16_t*>(p);
    }
    return W2V2_OK;
}

// ---- the forward plan ---------------------------------------------------------------------------------------------------------
// Every rule of DESIGN.md's table ("The forward plan") is one line here, and nowhere else.
//
// Precision mode 1 with bf16 shadows (`sh`): `sh` false = plain pointers everywhere, the GEMMs then round their fp32 operands
// themselves, with identical results.  Precision mode 2: fp32 operands, each an exact sum of three bf16 terms, six MFMA products
// (gemm_split.hip); shapes the split kernel does not take (lm_head: N = 32) stay on the fp32 MFMA.  Precision modes 2 / 3 with operand
// planes (W2V2_OPT_SPLIT_PLANES, default; `pm`): every producer of a GEMM operand writes its planes -- three bf16 terms (bf16x3) or
// two fp16 terms (f16x2) per element -- and the GEMM streams them (gemm_split_sw.hip).  Whether a call site does is decided here from
// its shape, so that the producer knows: whole 256-column tiles, K % 64 == 0, 16-byte aligned rows, and enough tiles to fill the chip
// (below that the fp32 path's small tiles serve a single utterance better).
ForwardPlan w2v2_plan_forward(const w2v2_model* m, int B, int64_t L, bool planes, bool packed) {
    const w2v2_config& c = m->cfg;
    ForwardPlan p;
    const int NC = p.NC = c.num_conv_layers;
    p.B = B;
    p.L = L;
    p.conv_T.resize(NC);
    {
        int64_t t = L;
        for (int i = 0; i < NC; ++i) p.conv_T[i] = (int)(t = 1 + (t - c.kernal_sizes[i]) / c.strides[i]);
    }
    p.T = p.conv_T[NC - 1];
    const int64_t BT = p.BT = (int64_t)B * p.T;
    const int H = c.hidden_size, F = c.intermediate_size;
    p.sh = m->precision == 1 && m->opt_shadows;
    // the attention kernel: one route for every layer, dense or over the packed stream's tiles (B = 1).  The bf16 family runs in
    // mode 1 with or without shadows; with them q | k | v and ctx are also kept as bf16
    p.attn = attention_route(attention_problem(AP_INFER, m->precision, packed ? 1 : B, p.T, H, c.num_heads, packed));
    p.attn16 = p.sh && p.attn.family == AF_BF16;
    p.pm = planes && m->precision >= W2V2_PRECISION_BF16X3 && m->opt_planes;
    p.fmt = m->precision == W2V2_PRECISION_F16X2 ? PF_F16X2 : PF_BF16X3;
    p.keep = m->opt_keep_acts;
    p.layer_mode = c.feature_extractor_norm_type == 1;
    p.prenorm = c.attention_norm_type == 1;
    p.act = c.is_gelu_approx ? 2 : 1;
    // element-wise kernels in precision mode 1 evaluate exact GELU through the 5-term erf the bf16 GEMM epilogue uses (act 3)
    p.act_ew = (p.act == 1 && m->precision == 1) ? 3 : p.act;
    // (dense and packed alike: the packed forward runs in mode 1 only under W2V2_OPT_BF16_PACKED, and then with the segment form)
    p.pos16 = w2v2_pos_conv_bf16_ok(m);
    const bool sh = p.sh, pm = p.pm, keep = p.keep;

    // ---- plane-fed call sites ----
    auto site = [&](int64_t M_, int N_, int K_, int nb, int64_t lda_, int64_t sA_) {
        return pm && N_ % 256 == 0 && K_ % 64 == 0 && lda_ % 8 == 0 && sA_ % 8 == 0 && 128 * lda_ < (1 << 29) && ((M_ + 127) / 128) * (N_ / 256) * nb >= 128;
    };
    p.cp.assign(NC + 1, 0);
    for (int i = 1; i < NC; ++i)
        p.cp[i] = site(p.conv_T[i], c.filter_sizes[i], c.kernal_sizes[i] * c.filter_sizes[i - 1], B, (int64_t)c.strides[i] * c.filter_sizes[i - 1],
                       (int64_t)p.conv_T[i - 1] * c.filter_sizes[i - 1]) && c.filter_sizes[i - 1] % 4 == 0;
    const int C512 = c.filter_sizes[NC - 1];
    p.p_proj = site(BT, H, C512, 1, C512, 0) && C512 % 4 == 0;
    p.p_qkv = site(BT, 3 * H, H, 1, H, 0) && H % 4 == 0;
    p.p_out = site(BT, H, H, 1, H, 0);
    p.p_f1 = site(BT, F, H, 1, H, 0);
    p.p_f2 = site(BT, H, F, 1, F, 0) && F % 8 == 0;
    p.any_planes = p.p_proj || p.p_qkv || p.p_out || p.p_f1 || p.p_f2;
    for (int i = 1; i < NC; ++i) p.any_planes = p.any_planes || p.cp[i];
    // the fused plane output needs conv0's 16-byte-store kernel (K = 10, stride 5); other geometries write fp32 and split it.  (The
    // packed group-norm pass, launch_conv0_packed, applies through the same kernel and writes exactly what the dense pass writes.)
    p.fused = NC > 1 && p.cp[1] && c.kernal_sizes[0] == 10 && c.strides[0] == 5 && 256 % (c.filter_sizes[0] / 4) == 0 && c.filter_sizes[0] / 4 <= 256;
    // the split attention kernel (precision modes 2 / 3, planes or not) -- and, where the out-projection is plane-fed, it writes ctx's
    // planes itself; any other attention kernel leaves fp32 to be split.  (p_out implies modes 2 / 3: ctx_fused implies split_attn.)
    p.split_attn = p.attn.family == AF_SPLIT;
    p.ctx_fused = p.p_out && p.split_attn;

    // ---- mode bf16: tensors whose one reader is a GEMM certain to stream the bf16 shadow are written only as bf16 ----
    // One predicate, gemm_bf16_streams_a16 (gemm_bf16_route.h), for all of them.  The weight side needs no test: w2v2_ensure_shadows, which
    // every forward with `sh` runs first, creates the (N, K) shadow of every GEMM weight, and no entry of m->w16 is ever erased.
    // K = lda = H (or F), strideA = 0: the predicate comes to H % 64 == 0 (F % 64 == 0).
    const bool h_streams = gemm_bf16_streams_a16(H, H, 0), f_streams = gemm_bf16_streams_a16(F, F, 0);
    const bool ln16_only = sh && !keep && h_streams;     // prenorm: the two in-layer LayerNorm outputs (2 x 98 MB per layer at 16 x 480000)
    p.ctx16_only = p.attn16 && h_streams;                // (75 MB per layer at B = 32).  Does NOT honour `keep`: ctx is no tap
    p.ffn_sh_only = sh && f_streams;                     // (302 MB per layer).  Does NOT honour `keep` either: the FFN hidden is no tap

    // ---- forms ----
    auto forms = [](bool f32, bool b16, bool pl) { return (unsigned)((f32 ? F32 : 0) | (b16 ? B16 : 0) | (pl ? PLANES : 0)); };
    p.conv.resize(NC);
    for (int i = 0; i < NC; ++i) {
        const bool last = i + 1 >= NC;               // the last conv output feeds a LayerNorm, not a GEMM: fp32 only
        const bool out_pl = !last && p.cp[i + 1];    // the next layer's GEMM streams this output's planes
        // planes and nothing else when nothing else is read: conv0 through its fused kernel; a group-norm layer when its own GEMM is
        // plane-fed (that kernel's epilogue writes fp32 or planes, not both); a LayerNorm-mode layer always (its LN + GELU pass writes both freely)
        const bool pl_only = out_pl && !keep && (i == 0 ? p.fused : (p.layer_mode || p.cp[i]));
        p.conv[i] = forms(!w2v2_conv_bf16_only(m, i, sh) && !pl_only, sh && !last, out_pl);
    }
    p.conv0_kernel = p.fused ? p.conv[0] : (p.conv[0] & ~(unsigned)PLANES);
    p.ln512 = forms(!(p.p_proj && !keep), sh, p.p_proj);
    p.proj = F32;
    p.hidden = F32;            // posout, hs[i] (prenorm), t1, t3: residual stream and LayerNorm inputs
    // the attention input: hs[i] (postnorm; also the residual and a tap, so fp32 stays) or t0 (prenorm)
    p.attn_in = p.prenorm ? forms(!((p.p_qkv && !keep) || ln16_only), sh, p.p_qkv) : forms(true, sh, p.p_qkv);
    // the bf16 attention kernels read q | k | v only as bf16: the projection then writes just that shadow
    p.qkv = p.attn16 ? (unsigned)B16 : (unsigned)F32;
    // (the packed forward in mode 1 runs the segment form of the same kernel, so this one line serves the dense and the packed forward)
    p.ctx = forms(!(p.ctx16_only || (p.ctx_fused && !keep)), p.attn16, p.p_out);
    p.attn_kernel = p.ctx_fused ? p.ctx : (p.ctx & ~(unsigned)PLANES);
    // the FFN input t2: postnorm it is also the FFN's residual, so fp32 stays
    p.ffn_in = p.prenorm ? forms(!((p.p_f1 && !keep) || ln16_only), sh, p.p_f1) : forms(true, sh, p.p_f1);
    // the FFN hidden: planes only when both FFN GEMMs are plane-fed (the plane-fed epilogue writes fp32 or planes)
    p.ffn = forms(!p.ffn_sh_only && !(p.p_f1 && p.p_f2 && !keep), sh, p.p_f2);
    p.head_in = forms(true, sh, false);       // hs[num_layers] (postnorm) or enc_out (prenorm)
    return p;
}

// ---- GEMM routing ---------------------------------------------------------------------------------------------------------------
// C = act(A Bw + bias) + res for a GEMM that is not plane-fed, on the route the mode selects: the six-product split kernel (modes
// bf16x3 / f16x2, shapes it takes), the fp32 MFMA, or -- `sh` -- the bf16 kernel with the shadows A16 / C16 and the weight's.  Raw
// pointers; a form the caller's forward did not write is passed as null, and a route that would read it is an error, not a stale read.
// Shared by the inference forward (gemm() below) and the training forward (w2v2_train.hip).
int w2v2_gemm_route(w2v2_model* m, bool sh, hipStream_t s, const float* A, const uint16_t* A16, int64_t lda, int64_t strideA, const float* Bw,
                    int64_t ldb, float* Cc, uint16_t* C16, int64_t ldc, int64_t strideC, const float* bias, const float* res, int M, int N, int K,
                    int nbatch, int act_) {
    Profiler* pf = m->prof;
    if (w2v2_use_split_gemm(m, A, lda, strideA, ldb, M, N, K, nbatch)) {
        W2V2_REQUIRE(A, "forward: the six-product GEMM (M=%d N=%d K=%d) reads an fp32 A this forward did not write", M, N, K);
        const uint16_t* planes = nullptr;
        if (int e = w2v2_split_planes(m, Bw, K, N, s, &planes)) return e;
        return launch_gemm_split(pf, A, lda, strideA, planes, Cc, ldc, strideC, bias, res, M, N, K, nbatch, act_, s);
    }
    if (!sh) {
        W2V2_REQUIRE(A, "forward: the fp32 GEMM (M=%d N=%d K=%d) reads an fp32 A this forward did not write", M, N, K);
        return launch_gemm(pf, A, lda, strideA, Bw, ldb, Cc, ldc, strideC, bias, res, M, N, K, nbatch, act_, s);
    }
    GemmShadows x;
    x.A16 = A16; x.B16 = m->w16[Bw]; x.C16 = C16; x.ldb16 = K;
    W2V2_REQUIRE(A || (A16 && gemm_bf16_streams_a16(K, lda, strideA)),
                 "forward: the bf16 GEMM (M=%d N=%d K=%d) cannot stream A's shadow and this forward wrote no fp32 A", M, N, K);
    return launch_gemm_bf16_x(pf, A, lda, strideA, Bw, ldb, 0, Cc, ldc, strideC, bias, res, M, N, K, nbatch, act_, x, s);
}

// One tensor as a GEMM sees it: the forms this forward fills (ForwardPlan) and the buffers of the three forms (null where the
// model has none).  gemm() masks the buffers by the forms, so a call site names buffers and a plan field, never a condition.
struct Tens {
    unsigned forms;
    float* f32;
    uint16_t* b16;
    const w2v2_model::PlaneBuf* pl;
};

// C = act(A Bw + bias) + res on the route the mode and `plane_fed` (the call site's plan field) select; C is written in exactly
// C.forms (planes the route's epilogue cannot write are split off the fp32 result).  A route that would read a form of A the plan
// did not have written is an error, not a read of a stale buffer.
static int gemm(w2v2_model* m, const ForwardPlan& plan, hipStream_t s, bool plane_fed, const Tens& A, int64_t lda, int64_t strideA, const float* Bw,
                int64_t ldb, const Tens& C, int64_t ldc, int64_t strideC, const float* bias, const float* res, int M, int N, int K, int nbatch,
                int act_) {
    Profiler* pf = m->prof;
    float* Cc = ForwardPlan::f32(C.forms, C.f32);
    const w2v2_model::PlaneBuf* Cpl = (C.forms & PLANES) ? C.pl : nullptr;
    auto split_out = [&]() -> int {
        W2V2_REQUIRE(Cc && ldc == N && (nbatch == 1 || strideC == (int64_t)M * N), "forward: plane output of a strided result");
        return launch_split_planes(Cc, Cpl->p, Cpl->plane, (int64_t)nbatch * M * N, plan.fmt, m->range_flag, s);
    };
    if (plane_fed) {
        W2V2_REQUIRE((A.forms & PLANES) && A.pl, "forward: a plane-fed GEMM (M=%d N=%d K=%d) whose A has no planes in this forward", M, N, K);
        W2V2_REQUIRE(Cc || Cpl, "forward: a plane-fed GEMM (M=%d N=%d K=%d) with neither an fp32 nor a plane output", M, N, K);
        const uint16_t* img = nullptr;
        const float* sc = nullptr;
        if (int e = w2v2_split_images(m, Bw, K, N, plan.fmt, s, &img, &sc)) return e;
        const bool planes_only = !Cc;          // the plane epilogue writes fp32 or planes
        if (int e = launch_gemm_split_sw(pf, plan.fmt, A.pl->p, A.pl->plane, lda, strideA, img, sc, Cc, planes_only ? Cpl->p : nullptr,
                                         planes_only ? Cpl->plane : 0, ldc, strideC, bias, res, M, N, K, nbatch, act_, m->range_flag, s))
            return e;
        return (Cpl && !planes_only) ? split_out() : W2V2_OK;
    }
    if (int e = w2v2_gemm_route(m, plan.sh, s, ForwardPlan::f32(A.forms, A.f32), ForwardPlan::b16(A.forms, A.b16), lda, strideA, Bw, ldb, Cc,
                                ForwardPlan::b16(C.forms, C.b16), ldc, strideC, bias, res, M, N, K, nbatch, act_))
        return e;
    return Cpl ? split_out() : W2V2_OK;
}

// What the packed forward hands the shared forward body: the stream's utterance and tile tables (device) and where the
// stream-sized head output goes.  The workspace holds at least the stream (ws_B == 1, ws_L >= L).
struct PackedPlan {
    const PackSeg* segs;
    int nseg;
    const SegTile* pos_tiles;
    int npos;
    const SegTile* attn_tiles;
    int nattn;
    double sum_nf2;
    float* head_out;          // (stream frames, vocab) when the model has a head
    double* gram_ws;          // w2v2_forward_windows: conv0's GroupNorm statistics as the dense forward takes them, or null
    int max_conv0_rows;       // conv0 rows of the longest utterance
};

// ---- feature extractor (feature_extractor.py:54-59) and feature projection (feature_extractor.py:92-95) ---------------------------
// The same sequence in the inference and the training forward (frozen, no dropout inside); training plans it without planes.
int w2v2_forward_frontend(w2v2_model* m, const ForwardPlan& plan, const float* wave, const PackedPlan* pk, hipStream_t s) {
    const w2v2_config& c = m->cfg;
    Profiler* pf = m->prof;
    const int NC = plan.NC, B = plan.B, H = c.hidden_size;
    const int64_t L = plan.L, BT = plan.BT;
    auto fe = [&](int i, const char* leaf) { return m->P("feature_extractor/conv_layers/" + std::to_string(i) + leaf); };
    // conv-stack output i as a GEMM operand (the shadow and plane buffers exist only in the modes, and for the layers, that use them)
    auto conv = [&](int i, unsigned forms) {
        return Tens{forms, m->conv[i], ForwardPlan::b16(forms, m->conv16, i), ForwardPlan::planes(forms, m->conv48, i)};
    };
    // "convI" cannot be read back exactly when this forward writes no fp32 copy of it (LayerNorm mode: conv[i] then holds the pre-norm values)
    m->acts_skipped.clear();
    for (int i = 0; i < NC; ++i)
        if (!(plan.conv[i] & F32)) m->acts_skipped.push_back("conv" + std::to_string(i));
    {
        const unsigned k = plan.conv0_kernel;
        const PlaneDst po = plan.plane_out(ForwardPlan::planes(k, m->conv48, 0), m->range_flag);
        if (pk && !plan.layer_mode) {     // GroupNorm statistics per utterance, over exactly its rows
            if (int e = launch_conv0_packed(pf, wave, fe(0, "/conv/kernel"), c.conv_bias ? fe(0, "/conv/bias") : nullptr, fe(0, "/layer_norm/gamma"),
                                            fe(0, "/layer_norm/beta"), ForwardPlan::f32(k, m->conv[0]), m->conv0_ws, m->pk_scale, L, c.kernal_sizes[0],
                                            c.strides[0], c.filter_sizes[0], 1e-5f, plan.act_ew, pk->segs, pk->nseg, s, po, pk->gram_ws,
                                            pk->max_conv0_rows, ForwardPlan::b16(k, m->conv16, 0)))
                return e;
        } else if (int e = launch_conv0_x(pf, wave, fe(0, "/conv/kernel"), c.conv_bias ? fe(0, "/conv/bias") : nullptr,
                                          fe(0, "/layer_norm/gamma"), fe(0, "/layer_norm/beta"), ForwardPlan::f32(k, m->conv[0]),
                                          ForwardPlan::b16(k, m->conv16, 0), m->conv0_ws, B, L, c.kernal_sizes[0], c.strides[0],
                                          c.filter_sizes[0], 1e-5f, plan.layer_mode ? 2 : 0, plan.act_ew, s, po)) {    // (layer mode: conv + LayerNorm + GELU in one pass)
            return e;
        }
        if ((plan.conv[0] & PLANES) && !(k & PLANES)) {
            W2V2_REQUIRE(k & F32, "forward: conv0's planes are to be split off an fp32 output this forward does not write");
            if (int e = launch_split_planes(m->conv[0], m->conv48[0].p, m->conv48[0].plane, (int64_t)B * plan.conv_T[0] * c.filter_sizes[0], plan.fmt, m->range_flag, s))
                return e;
        }
    }
    for (int i = 1; i < NC; ++i) {
        const int cin = c.filter_sizes[i - 1], cout = c.filter_sizes[i];
        const int Tin = plan.conv_T[i - 1], Tout = plan.conv_T[i];
        // strided Conv1D == GEMM over an overlapping window view: lda = stride * C_in < K * C_in
        // This layer's output in its planned forms: from the GEMM epilogue (group-norm mode: bias + GELU there) or from the
        // LayerNorm + GELU pass behind it (layer-norm mode: the GEMM output is that pass's fp32 input)
        if (int e = gemm(m, plan, s, plan.cp[i], conv(i - 1, plan.conv[i - 1]), (int64_t)c.strides[i] * cin, (int64_t)Tin * cin, fe(i, "/conv/kernel"), cout,
                         conv(i, plan.conv_gemm_out(i)), cout, (int64_t)Tout * cout, c.conv_bias ? fe(i, "/conv/bias") : nullptr, nullptr, Tout, cout,
                         c.kernal_sizes[i] * cin, B, plan.layer_mode ? 0 : plan.act))
            return e;
        if (plan.layer_mode) {
            const Tens y = conv(i, plan.conv[i]);
            const PlaneDst po = plan.plane_out(y.pl, m->range_flag);
            if (int e = launch_layer_norm_x(pf, m->conv[i], ForwardPlan::f32(y.forms, y.f32), fe(i, "/layer_norm/gamma"), fe(i, "/layer_norm/beta"),
                                            (int64_t)B * Tout, cout, 1e-5f, plan.act_ew, y.b16, s, po))
                return e;
        }
    }
    const int C = c.filter_sizes[NC - 1];
    const Tens ln512{plan.ln512, m->ln512, m->ln512_16, &m->ln512_48}, proj{plan.proj, m->proj, nullptr, nullptr};
    {
        const PlaneDst po = plan.plane_out(ForwardPlan::planes(plan.ln512, m->ln512_48), m->range_flag);
        if (int e = launch_layer_norm_x(pf, m->conv[NC - 1], ForwardPlan::f32(plan.ln512, m->ln512), m->P("feature_projection/layer_norm/gamma"),
                                        m->P("feature_projection/layer_norm/beta"), BT, C, c.layer_norm_eps, 0, ForwardPlan::b16(plan.ln512, m->ln512_16), s, po))
            return e;
    }
    return gemm(m, plan, s, plan.p_proj, ln512, C, 0, m->P("feature_projection/projection/kernel"), H, proj, H, 0,
                m->P("feature_projection/projection/bias"), nullptr, (int)BT, H, C, 1, 0);
}

// The inference forward over (B, L).  pk null: the batched forward (w2v2_forward).  pk set: one stream of packed utterances
// (B = 1; precision modes fp32, bf16x3, f16x2, and bf16 under W2V2_OPT_BF16_PACKED); the three stages that mix frames -- conv0's GroupNorm statistics, the positional
// conv and attention -- take their segment-aware forms, everything else runs unchanged over the stream.  The stream rows no
// utterance owns (1-2 behind each) are zeroed in the two buffers only segment kernels write, posout and ctx, so that every
// row a plane producer reads is defined by the call's own inputs.
static int forward_impl(w2v2_model* m, const float* wave, int32_t B, int64_t L, const int32_t* mask, float* out, hipStream_t s,
                        const PackedPlan* pk) {
    const w2v2_config& c = m->cfg;
    PrecisionScope precision(m->precision);
    const int64_t Tll = w2v2_num_frames(m, L);
    W2V2_REQUIRE(Tll >= 1, "forward: %lld samples are shorter than the conv stack's receptive field", (long long)L);
    if (!pk)
        if (int e = w2v2_ensure_workspace(m, B, L)) return e;
    W2V2_REQUIRE(m->ws_B == B && m->ws_L >= L, "forward: workspace (%d, %lld) does not hold (%d, %lld)", m->ws_B, (long long)m->ws_L,
                 B, (long long)L);
    const ForwardPlan plan = w2v2_plan_forward(m, B, L, true, pk != nullptr);
    // (packed: the shadows are sized once per workspace, so for its capacity -- a later, longer stream that fits reuses them)
    if (plan.sh)
        if (int e = w2v2_ensure_shadows(m, B, pk ? m->conv_T.back() : plan.T, s)) return e;
    // (packed: sized for the workspace's capacity, so that a later packed call whose stream fits reuses them as it reuses the workspace)
    if (plan.any_planes)
        if (int e = w2v2_ensure_planes(m, B, pk ? m->ws_L : L, plan.fmt)) return e;
    Profiler* pf = m->prof;
    const int T = plan.T, H = c.hidden_size, F = c.intermediate_size, NL = c.num_layers;
    const int64_t BT = plan.BT;
    const int act = plan.act;
    const bool prenorm = plan.prenorm;
    const float eps = c.layer_norm_eps;

    if (int e = w2v2_forward_frontend(m, plan, wave, pk, s)) return e;
    // ---- encoder (encoder.py:251-276) ----
    const int32_t* flen = nullptr;
    if (mask) {
        if (int e = launch_frame_lengths(pf, mask, m->frame_len, B, L, c.kernal_sizes, c.strides, c.num_conv_layers, s)) return e;
        flen = m->frame_len;
    }
    if (pk && plan.pos16) {              // packed, precision mode 1: the dense mode's batched GEMM over a padded stream (posconv.hip);
        if (int e = ensure_pos_w16(m, s)) return e;      // it zeroes the rows of posout that no utterance owns itself
        if (int e = launch_pos_conv_bf16_packed(pf, m->proj, m->pos_w16, m->P("encoder/pos_conv_embed/conv/bias"), m->posout, pk->segs, pk->nseg, T, H,
                                                c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, act, s))
            return e;
    } else if (pk) {                     // each utterance zero-padded at its own edges (the fp32 kernel, as the dense forward outside mode 1's shapes)
        if (int e = launch_pos_conv_packed(pf, m->proj, m->pos_wg, m->P("encoder/pos_conv_embed/conv/bias"), m->posout, pk->pos_tiles, pk->npos,
                                           T, H, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, act, s))
            return e;
        if (int e = launch_pack_zero_gaps(m->posout, nullptr, T, H, pk->segs, pk->nseg, s)) return e;
    } else if (plan.pos16) {             // precision mode 1: one batched bf16 GEMM over (sample, group); m->t0 is free here
        if (int e = w2v2_ensure_pos16(m, B, T, s)) return e;
        if (int e = launch_pos_conv_bf16(pf, m->proj, m->pos_w16, m->P("encoder/pos_conv_embed/conv/bias"), flen, m->posout, nullptr,
                                         m->pos_pack16, m->t0, B, T, H, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups,
                                         act, c.num_conv_pos_embeddings / 2, 1, s))
            return e;
    } else if (int e = launch_pos_conv(pf, m->proj, m->pos_wg, m->P("encoder/pos_conv_embed/conv/bias"), flen, m->posout, B, T,
                                       H, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, act, s)) {
        return e;
    }
    // the planes each producer leaves for its consumer (one buffer serves every layer: stream order)
    const PlaneDst po_attn = plan.plane_out(ForwardPlan::planes(plan.attn_in, m->attn_in48), m->range_flag),
                   po_ctx = plan.plane_out(ForwardPlan::planes(plan.ctx, m->ctx48), m->range_flag),
                   po_ffn_in = plan.plane_out(ForwardPlan::planes(plan.ffn_in, m->ffn_in48), m->range_flag);
    // ... and what the attention kernel is handed: ctx's planes where it writes them itself; with planes on but none wanted from it, the
    // split attention still reports f16x2 saturation through the flag
    PlaneDst attn_pl = plan.plane_out(ForwardPlan::planes(plan.attn_kernel, m->ctx48), m->range_flag);
    if (!attn_pl.on && plan.pm) {
        attn_pl.o.range_flag = m->range_flag;
        attn_pl.on = true;
    }
    // packed with the bf16 family: ctx exists in the forms that kernel writes
    const bool pk_attn16 = pk && plan.attn.family == AF_BF16;
    if (pk_attn16) {                     // (the forms of ctx that kernel writes in this plan: with ctx16_only just the shadow)
        if (int e = launch_pack_zero_gaps(ForwardPlan::f32(plan.ctx, m->ctx), nullptr, T, H, pk->segs, pk->nseg, s, ForwardPlan::b16(plan.ctx, m->ctx16))) return e;
    } else if (pk) {                     // (the attention kernels write only the utterances' rows of ctx and of its planes, in every layer)
        if (int e = launch_pack_zero_gaps(m->ctx, po_ctx, T, H, pk->segs, pk->nseg, s)) return e;
    }
    // the tensors of a layer as GEMM operands.  Postnorm: the attention input is hs[i], written by the previous LayerNorm; prenorm: t0.
    const Tens qkv{plan.qkv, m->qkv, m->qkv16, nullptr}, ctx{plan.ctx, m->ctx, m->ctx16, &m->ctx48}, t1{plan.hidden, m->t1, nullptr, nullptr},
               ffn_in{plan.ffn_in, m->t2, m->t2_16, &m->ffn_in48}, ffn{plan.ffn, m->ffn, m->ffn16, &m->ffn48};
    auto hs = [&](int i, unsigned forms) { return Tens{forms, m->hs[i], ForwardPlan::b16(forms, m->hs16, i), &m->attn_in48}; };
    // what the attention kernel of every layer reads and writes: the forms of q | k | v and ctx this plan has (the packed fp32 family reads the fp32 q | k | v)
    AttnIO attn_io;
    attn_io.qkv = ForwardPlan::f32(plan.qkv, m->qkv);
    attn_io.qkv16 = ForwardPlan::b16(plan.qkv, m->qkv16);
    attn_io.ctx = ForwardPlan::f32(plan.ctx, m->ctx);
    attn_io.ctx16 = ForwardPlan::b16(plan.ctx, m->ctx16);
    attn_io.planes = plan.attn.family == AF_SPLIT ? (const PlaneOut*)attn_pl : nullptr;
    if (pk) {
        attn_io.tiles = pk->attn_tiles; attn_io.ntiles = pk->nattn; attn_io.frames = T; attn_io.sum_nf2 = pk->sum_nf2;
    } else {
        attn_io.frame_len = flen;
    }
    if (!prenorm)
        if (int e = launch_layer_norm_x(pf, m->posout, m->hs[0], m->P("encoder/layer_norm/gamma"), m->P("encoder/layer_norm/beta"), BT, H, eps, 0,
                                        ForwardPlan::b16(plan.attn_in, m->hs16, 0), s, po_attn))
            return e;
    for (int i = 0; i < NL; ++i) {
        const std::string b = "encoder/layers/" + std::to_string(i);
        const float* x = m->hs[i];
        const Tens attn_in = prenorm ? Tens{plan.attn_in, m->t0, m->t0_16, &m->attn_in48} : hs(i, plan.attn_in);
        if (prenorm)
            if (int e = launch_layer_norm_x(pf, x, ForwardPlan::f32(plan.attn_in, m->t0), m->P(b + "/layer_norm/gamma"), m->P(b + "/layer_norm/beta"), BT, H, eps, 0,
                                            ForwardPlan::b16(plan.attn_in, m->t0_16), s, po_attn))
                return e;
        if (int e = gemm(m, plan, s, plan.p_qkv, attn_in, H, 0, m->qkv_w[i], 3 * H, qkv, 3 * H, 0, m->qkv_b[i], nullptr, (int)BT, 3 * H, H, 1, 0))
            return e;
        if (int e = launch_attention_routed(pf, plan.attn, attn_io, s)) return e;
        if ((plan.ctx & PLANES) && !(plan.attn_kernel & PLANES)) {
            W2V2_REQUIRE(plan.ctx & F32, "forward: ctx's planes are to be split off an fp32 ctx this forward does not write");
            if (int e = launch_split_planes(m->ctx, m->ctx48.p, m->ctx48.plane, BT * H, plan.fmt, m->range_flag, s)) return e;
        }
        // out projection + residual (encoder.py:31,117-119)
        if (int e = gemm(m, plan, s, plan.p_out, ctx, H, 0, m->P(b + "/attention/out_proj/kernel"), H, t1, H, 0, m->P(b + "/attention/out_proj/bias"), x,
                         (int)BT, H, H, 1, 0))
            return e;
        if (int e = launch_layer_norm_x(pf, m->t1, ForwardPlan::f32(plan.ffn_in, m->t2), m->P(b + (prenorm ? "/final_layer_norm/gamma" : "/layer_norm/gamma")),
                                        m->P(b + (prenorm ? "/final_layer_norm/beta" : "/layer_norm/beta")), BT, H, eps, 0,
                                        ForwardPlan::b16(plan.ffn_in, m->t2_16), s, po_ffn_in))
            return e;
        const float* ffn_res = prenorm ? m->t1 : m->t2;
        // the FFN intermediate has one consumer: with shadows only its bf16 form is written (302 MB of fp32 stores saved)
        if (int e = gemm(m, plan, s, plan.p_f1, ffn_in, H, 0, m->P(b + "/feed_forward/intermediate_dense/kernel"), F, ffn, F, 0,
                         m->P(b + "/feed_forward/intermediate_dense/bias"), nullptr, (int)BT, F, H, 1, act))
            return e;
        // output dense + residual; StochasticDepth at inference is a plain add (tensorflow_addons.py:386-390)
        const Tens dst{plan.hidden, prenorm ? m->hs[i + 1] : m->t3, nullptr, nullptr};
        if (int e = gemm(m, plan, s, plan.p_f2, ffn, F, 0, m->P(b + "/feed_forward/output_dense/kernel"), H, dst, H, 0,
                         m->P(b + "/feed_forward/output_dense/bias"), ffn_res, (int)BT, H, F, 1, 0))
            return e;
        if (!prenorm) {     // (its planes are the next layer's attention input; the last layer's output is the head's)
            const unsigned y = i + 1 < NL ? plan.attn_in : plan.head_in;
            const PlaneDst po = plan.plane_out(ForwardPlan::planes(y, m->attn_in48), m->range_flag);
            if (int e = launch_layer_norm_x(pf, m->t3, m->hs[i + 1], m->P(b + "/final_layer_norm/gamma"), m->P(b + "/final_layer_norm/beta"), BT, H, eps, 0,
                                            ForwardPlan::b16(y, m->hs16, i + 1), s, po))
                return e;
        }
    }
    if (prenorm)
        if (int e = launch_layer_norm_x(pf, m->hs[NL], m->enc_out, m->P("encoder/layer_norm/gamma"), m->P("encoder/layer_norm/beta"), BT, H, eps, 0,
                                        ForwardPlan::b16(plan.head_in, m->enc16), s))
            return e;
    // ---- head (modeling.py:253-254) ----
    // (packed: the stream's rows; w2v2_forward_packed gathers the utterances' frames from them)
    if (c.with_lm_head) {
        const Tens head_in = prenorm ? Tens{plan.head_in, m->enc_out, m->enc16, nullptr} : hs(NL, plan.head_in);
        const Tens logits{F32, pk ? pk->head_out : out, nullptr, nullptr};
        if (int e = gemm(m, plan, s, false, head_in, H, 0, m->P("lm_head/kernel"), c.vocab_size, logits, c.vocab_size, 0, m->P("lm_head/bias"), nullptr,
                         (int)BT, c.vocab_size, H, 1, 0))
            return e;
    } else if (!pk) {
        W2V2_HIP_CHECK(hipMemcpyAsync(out, m->enc_out, (size_t)BT * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return W2V2_OK;
}

// eps of Wav2Vec2Processor._normalize (processor.py: (x - mean) / sqrt(var + 1e-5))
constexpr double kWaveNormEps = 1e-5;

// one piece of a packed stream: samples [src0, src0 + len) of the caller's buffer, computed as an utterance of its own; rows
// [keep0, keep0 + keepn) of its frames go to the caller's output
struct StreamPiece {
    int64_t src0, len;
    int32_t keep0, keepn;
};

static int stream_forward_ready(w2v2_model* m, const char* who) {
    if (!m->finalized) {
        set_error("%s: call w2v2_finalize after setting the variables", who);
        return W2V2_ESTATE;
    }
    static const char* modes[] = {"fp32", "bf16", "bf16x3", "f16x2"};
    W2V2_REQUIRE(m->precision == W2V2_PRECISION_FP32 || m->precision == W2V2_PRECISION_BF16X3 || m->precision == W2V2_PRECISION_F16X2 ||
                     (m->precision == W2V2_PRECISION_BF16 && m->opt_bf16_packed),
                 "%s: precision mode %s is not supported (fp32, bf16x3, f16x2; bf16 with the option W2V2_OPT_BF16_PACKED)", who,
                 (m->precision >= 0 && m->precision <= 3) ? modes[m->precision] : "?");
    return W2V2_OK;
}

// The body of w2v2_forward_packed and w2v2_forward_windows: the (checked) pieces into the aligned stream, one B = 1 forward over
// it with the three segment-aware stages, the kept rows out.  normalize: each piece's samples as Wav2Vec2Processor._normalize
// gives them, on the device (packed.hip: pack_stats_kernel, pack_scatter_kernel).  dense_stats: conv0's GroupNorm statistics of
// each piece in the dense forward's Gram form (conv0.hip), so that a piece carries the bits w2v2_forward gives it alone; the
// packed entry keeps the chunk partials it has always used, and its bits.
static int forward_stream(w2v2_model* m, const char* who, const float* wave, const std::vector<StreamPiece>& pieces, int normalize,
                          bool dense_stats, float* out, hipStream_t s) {
    const w2v2_config& c = m->cfg;
    const int n = (int)pieces.size();
    // alignment unit: a multiple of the total stride (whole frames at every layer) and of conv0's stats chunk in samples
    int64_t A = 1;
    for (int i = 0; i < c.num_conv_layers; ++i) A *= c.strides[i];
    const int64_t chunk = (int64_t)c.strides[0] * conv0_chunk_frames();
    int64_t g = A, r = chunk;
    while (r) { const int64_t t = g % r; g = r; r = t; }
    const int64_t U = A / g * chunk;
    // utterances in the stream, and the tiles of the two stages that work per utterance
    std::vector<PackSeg> segs((size_t)n);
    int64_t L = 0, rows = 0;
    int max_rows0 = 0;
    double sum_nf2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const int64_t len = pieces[i].len, nf = w2v2_num_frames(m, len);
        max_rows0 = std::max(max_rows0, (int)(1 + (len - c.kernal_sizes[0]) / c.strides[0]));
        segs[i] = PackSeg{L, len, pieces[i].src0, (int32_t)(L / A), (int32_t)nf, (int32_t)rows, pieces[i].keep0};
        L += (len + U - 1) / U * U;
        rows += pieces[i].keepn;
        sum_nf2 += (double)nf * (double)nf;
    }
    const int64_t T = w2v2_num_frames(m, L);
    W2V2_REQUIRE(T < (1 << 24) && (int64_t)segs.back().f0 + segs.back().nf <= T, "%s: stream of %lld samples out of range", who,
                 (long long)L);
    // (attention tiles of the height of the kernel that will run: 128 queries for mode 1's bf16 kernel, 256 for the others)
    const int H = c.hidden_size, PR = pos_conv_packed_rows();
    const AttnRoute attn = attention_route(attention_problem(AP_INFER, m->precision, 1, (int)T, H, c.num_heads, true));
    W2V2_REQUIRE(!attn.refusal, attention_refusal_text(attn), attn.dh);
    const int AR = attn.rows;
    std::vector<SegTile> tiles;
    for (const int rows_per_tile : {PR, AR})
        for (const PackSeg& sg : segs)
            for (int t0 = 0; t0 < sg.nf; t0 += rows_per_tile) tiles.push_back(SegTile{sg.f0, sg.nf, t0, 0});
    int npos = 0;
    for (const PackSeg& sg : segs) npos += (sg.nf + PR - 1) / PR;
    const int nattn = (int)tiles.size() - npos;

    // workspace of a B = 1 forward over at least the stream, rounded up so that later streams that fit reuse it
    if (!(m->ws_B == 1 && m->ws_L >= L))
        if (int e = w2v2_ensure_workspace(m, 1, (L + 64 * U - 1) / (64 * U) * (64 * U))) return e;
    if (m->pk_L != m->ws_L) {
        const int64_t Tcap = w2v2_num_frames(m, m->ws_L);
        m->pk_seg_cap = (int)(m->ws_L / U);
        m->pk_tile_cap = (int)(2 * (int64_t)m->pk_seg_cap + Tcap / PR + Tcap / ATTN_MIN_PACKED_ROWS);
        if (int e = w2v2_ws_alloc(m, &m->pk_wave, m->ws_L)) return e;
        if (int e = w2v2_ws_alloc(m, &m->pk_scale, (int64_t)m->pk_seg_cap * 2 * c.filter_sizes[0])) return e;
        if (int e = w2v2_ws_alloc(m, &m->pk_out, c.with_lm_head ? Tcap * c.vocab_size : 0)) return e;
        float* tab = nullptr;
        if (int e = w2v2_ws_alloc(m, &tab, ((int64_t)m->pk_seg_cap * sizeof(PackSeg) + (int64_t)m->pk_tile_cap * sizeof(SegTile)) / sizeof(float))) return e;
        m->pk_tab = tab;
        float* stats = nullptr;
        if (int e = w2v2_ws_alloc(m, &stats, (int64_t)m->pk_seg_cap * 2 * (sizeof(double) / sizeof(float)))) return e;
        m->pk_stats = reinterpret_cast<double*>(stats);
        float* gram = nullptr;
        if (int e = w2v2_ws_alloc(m, &gram, conv0_gram_ws_doubles(m->ws_L, c.strides[0], m->pk_seg_cap) * (sizeof(double) / sizeof(float)))) return e;
        m->pk_gram = reinterpret_cast<double*>(gram);
        m->pk_L = m->ws_L;
    }
    W2V2_REQUIRE(n <= m->pk_seg_cap && (int64_t)tiles.size() <= m->pk_tile_cap, "%s: tables exceed their capacity", who);
    // tables -> device through pinned staging; the previous call's copy out of it must have completed before it is rewritten
    const size_t seg_bytes = segs.size() * sizeof(PackSeg), bytes = seg_bytes + tiles.size() * sizeof(SegTile);
    if (int e = pinned_stage_begin(m->pk_stage, bytes, (size_t)64 << 10)) return e;
    memcpy(m->pk_stage.p, segs.data(), seg_bytes);
    memcpy(static_cast<char*>(m->pk_stage.p) + seg_bytes, tiles.data(), bytes - seg_bytes);
    if (int e = pinned_stage_upload(m->pk_stage, m->pk_tab, bytes, s)) return e;
    const PackSeg* dsegs = static_cast<const PackSeg*>(m->pk_tab);
    const SegTile* dtiles = reinterpret_cast<const SegTile*>(static_cast<const char*>(m->pk_tab) + seg_bytes);

    if (normalize)
        if (int e = launch_pack_stats(wave, dsegs, n, kWaveNormEps, m->pk_stats, s)) return e;
    if (int e = launch_pack_scatter(wave, m->pk_wave, L, dsegs, n, s, normalize ? m->pk_stats : nullptr)) return e;
    const PackedPlan plan{dsegs, n, dtiles, npos, dtiles + npos, nattn, sum_nf2, m->pk_out, dense_stats ? m->pk_gram : nullptr, max_rows0};
    if (int e = forward_impl(m, m->pk_wave, 1, L, nullptr, out, s, &plan)) return e;
    return launch_pack_gather(c.with_lm_head ? m->pk_out : m->enc_out, out, rows, c.with_lm_head ? c.vocab_size : H, dsegs, n, s);
}

extern "C" {

int w2v2_forward(w2v2_model* m, const float* wave, int32_t B, int64_t L, const int32_t* mask,
                 float* out, void* stream) {
    W2V2_REQUIRE(m && wave && out, "forward: null argument");
    W2V2_REQUIRE(B > 0 && L > 0, "forward: bad batch shape (%d, %lld)", B, (long long)L);
    if (!m->finalized) {
        set_error("forward: call w2v2_finalize after setting the variables");
        return W2V2_ESTATE;
    }
    return forward_impl(m, wave, B, L, mask, out, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int w2v2_forward_packed(w2v2_model* m, const float* wave, int32_t n, const int64_t* cu_samples, float* out, void* stream) {
    W2V2_REQUIRE(m && wave && cu_samples && out, "forward_packed: null argument");
    if (int e = stream_forward_ready(m, "forward_packed")) return e;
    W2V2_REQUIRE(n >= 1, "forward_packed: %d utterances (need at least one)", n);
    W2V2_REQUIRE(cu_samples[0] == 0, "forward_packed: cu_samples[0] = %lld, must be 0", (long long)cu_samples[0]);
    // the special case of w2v2_forward_windows: utterance i from cu[i] on, every frame kept, no normalisation
    std::vector<StreamPiece> pieces((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int64_t len = cu_samples[i + 1] - cu_samples[i];
        W2V2_REQUIRE(len >= 0, "forward_packed: cu_samples decreases at utterance %d", i);
        const int64_t nf = w2v2_num_frames(m, len);
        W2V2_REQUIRE(nf >= 1, "forward_packed: utterance %d has %lld samples, shorter than the conv stack's receptive field", i,
                     (long long)len);
        pieces[i] = StreamPiece{cu_samples[i], len, 0, (int32_t)nf};
    }
    return forward_stream(m, "forward_packed", wave, pieces, 0, false, out, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_forward_windows(w2v2_model* m, const float* wave, int64_t wave_samples, int32_t n, const int64_t* sample0,
                         const int64_t* samples, const int32_t* keep0, const int32_t* keepn, int32_t normalize, float* out,
                         void* stream) {
    W2V2_REQUIRE(m && wave && sample0 && samples && keep0 && keepn && out, "forward_windows: null argument");
    if (int e = stream_forward_ready(m, "forward_windows")) return e;
    W2V2_REQUIRE(n >= 1, "forward_windows: %d windows (need at least one)", n);
    W2V2_REQUIRE(wave_samples >= 1, "forward_windows: a recording of %lld samples", (long long)wave_samples);
    W2V2_REQUIRE(normalize == 0 || normalize == 1, "forward_windows: normalize = %d, must be 0 or 1", normalize);
    std::vector<StreamPiece> pieces((size_t)n);
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(sample0[i] >= 0 && samples[i] >= 0 && samples[i] <= wave_samples && sample0[i] <= wave_samples - samples[i],
                     "forward_windows: window %d, samples [%lld, %lld + %lld), lies outside the recording's [0, %lld)", i,
                     (long long)sample0[i], (long long)sample0[i], (long long)samples[i], (long long)wave_samples);
        const int64_t nf = w2v2_num_frames(m, samples[i]);
        W2V2_REQUIRE(nf >= 1, "forward_windows: window %d has %lld samples, shorter than the conv stack's receptive field", i,
                     (long long)samples[i]);
        W2V2_REQUIRE(keepn[i] != 0, "forward_windows: window %d keeps no frame", i);
        W2V2_REQUIRE(keep0[i] >= 0 && keepn[i] > 0 && keep0[i] <= nf - keepn[i],
                     "forward_windows: window %d keeps frames [%d, %d + %d) of its %lld", i, keep0[i], keep0[i], keepn[i], (long long)nf);
        pieces[i] = StreamPiece{sample0[i], samples[i], keep0[i], keepn[i]};
    }
    return forward_stream(m, "forward_windows", wave, pieces, normalize, true, out, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_op_normalize_windows(const float* wave, int32_t n, const int64_t* sample0, const int64_t* samples, float* out, void* stream) {
    W2V2_REQUIRE(wave && sample0 && samples && out, "op_normalize_windows: null argument");
    W2V2_REQUIRE(n >= 1, "op_normalize_windows: %d windows (need at least one)", n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the windows back to back as the "stream": no alignment, no gaps
    std::vector<PackSeg> segs((size_t)n);
    int64_t L = 0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(sample0[i] >= 0 && samples[i] >= 1, "op_normalize_windows: window %d is [%lld, %lld + %lld)", i, (long long)sample0[i],
                     (long long)sample0[i], (long long)samples[i]);
        segs[i] = PackSeg{L, samples[i], sample0[i], 0, 0, 0, 0};
        L += samples[i];
    }
    const size_t tab_bytes = up256((size_t)n * sizeof(PackSeg));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_WINDOWS, s, tab_bytes + (size_t)n * 2 * sizeof(double), &raw)) return e;
    double* stats = reinterpret_cast<double*>(static_cast<char*>(raw) + tab_bytes);
    if (int e = staged_upload(SCRATCH_WINDOWS, s, raw, {{segs.data(), (size_t)n * sizeof(PackSeg), 0}}, (size_t)16 << 10)) return e;
    const PackSeg* dsegs = static_cast<const PackSeg*>(raw);
    if (int e = launch_pack_stats(wave, dsegs, n, kWaveNormEps, stats, s)) return e;
    return launch_pack_scatter(wave, out, L, dsegs, n, s, stats);
}
}  // extern "C"
