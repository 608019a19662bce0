// C ABI (include/w2v2.h): model lifetime, variable I/O, the activation workspace, options,
// profiling and the single-operator entry points.  Host code only; the forward is in
// forward.hip, training in w2v2_train.hip and the kernels in the sibling .hip files.
#include <algorithm>
#include <mutex>
#include <atomic>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "gemm_f32_route.h"
#include "model.h"
#include "train.h"

namespace w2v2 {

// ---- errors ---------------------------------------------------------------
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

const char* family_name(int f) {
    static const char* names[FAM_COUNT] = {"conv0_stats", "conv0_apply", "gemm_f32", "gemm_bf16", "gemm_split", "layer_norm",
                                           "pos_conv",    "attention",   "ctc",      "misc",      "dropout",    "reduce",
                                           "layer_norm_bwd", "optimizer"};
    return (f >= 0 && f < FAM_COUNT) ? names[f] : "?";
}

// ---- kernel-launch counters (common.h: W2V2_LAUNCH) ---------------------------
thread_local int tl_launch_family = FAM_MISC;
thread_local int tl_prof_depth = 0;
thread_local Profiler* tl_step_prof = nullptr;
static std::atomic<int64_t> g_kernel_launches[FAM_COUNT];
void note_kernel_launch() {
    const int f = tl_launch_family;
    g_kernel_launches[(f >= 0 && f < FAM_COUNT) ? f : FAM_MISC].fetch_add(1, std::memory_order_relaxed);
}
int64_t kernel_launches(int family) {
    return (family >= 0 && family < FAM_COUNT) ? g_kernel_launches[family].load(std::memory_order_relaxed) : 0;
}

// ---- profiler ---------------------------------------------------------------
struct ProfRec {
    int family;
    double flops, bytes;
    hipEvent_t e0, e1;
};
struct Profiler {
    bool enabled = false;
    unsigned mask = 0xFFFFFFFFu;    // families that get an event pair
    int stride = 1;                 // of a family's launches, every stride-th gets the pair (w2v2_profile_sampling)
    int64_t seen[32] = {0};         // launches of each family since the last reset, sampled or not
    int64_t launch_base[32] = {0};  // the process-wide kernel-launch counters at the last reset (a reset never clears them: another model,
                                    // or another thread's, keeps counting from its own base)
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;   // recycled events
};
Profiler* profiler_create() { return new Profiler(); }
void profiler_reset(Profiler* p) {
    for (auto& r : p->recs) {
        p->pool.push_back(r.e0);
        p->pool.push_back(r.e1);
    }
    p->recs.clear();
    for (auto& n : p->seen) n = 0;
    for (int f = 0; f < FAM_COUNT; ++f) p->launch_base[f] = kernel_launches(f);
}
int64_t profiler_kernel_launches(const Profiler* p, int family) {
    return (p && family >= 0 && family < FAM_COUNT) ? kernel_launches(family) - p->launch_base[family] : 0;
}
void profiler_destroy(Profiler* p) {
    if (!p) return;
    profiler_reset(p);
    for (auto e : p->pool) (void)hipEventDestroy(e);
    delete p;
}
void profiler_enable(Profiler* p, bool on) { p->enabled = on; }
void profiler_set_mask(Profiler* p, unsigned mask) { p->mask = mask ? mask : 0xFFFFFFFFu; }
bool profiler_enabled(const Profiler* p) { return p->enabled; }
static hipEvent_t prof_event(Profiler* p) {
    if (!p->pool.empty()) {
        hipEvent_t e = p->pool.back();
        p->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
void profiler_set_stride(Profiler* p, int stride) { p->stride = stride < 1 ? 1 : stride; }
int64_t profiler_seen(const Profiler* p, int family) { return p->seen[family & 31]; }
int profiler_begin(Profiler* p, int family, double flops, double bytes, hipStream_t s) {
    if (!p || !p->enabled || !((p->mask >> family) & 1u)) return -1;
    if ((p->seen[family & 31]++ % p->stride) != 0) return -1;
    ProfRec r{family, flops, bytes, prof_event(p), prof_event(p)};
    (void)hipEventRecord(r.e0, s);
    p->recs.push_back(r);
    return (int)p->recs.size() - 1;
}
void profiler_end(Profiler* p, int token, hipStream_t s) {
    if (!p || token < 0 || token >= (int)p->recs.size()) return;
    (void)hipEventRecord(p->recs[token].e1, s);
}
int profiler_read(Profiler* p, int family, int64_t* launches, double* ms, double* flops, double* bytes) {
    int64_t n = 0;
    double t = 0, f = 0, by = 0;
    for (auto& r : p->recs) {
        if (r.family != family) continue;
        W2V2_HIP_CHECK(hipEventSynchronize(r.e1));
        float dt = 0.f;
        W2V2_HIP_CHECK(hipEventElapsedTime(&dt, r.e0, r.e1));
        t += dt; f += r.flops; by += r.bytes; ++n;
    }
    *launches = n; *ms = t; *flops = f; *bytes = by;
    return W2V2_OK;
}

}  // namespace w2v2

using namespace w2v2;

static void add_param(w2v2_model* m, const std::string& name, std::vector<int64_t> shape) {
    Param p;
    p.name = name;
    p.shape = shape;
    p.numel = 1;
    for (auto d : shape) p.numel *= d;
    m->index[name] = (int)m->params.size();
    m->params.push_back(p);
}

// Same inventory and order as gsoc-wav2vec2_amd/wav2vec2/variables.py (the
// reference's 213 variables for base CTC).
static void build_inventory(w2v2_model* m) {
    const w2v2_config& c = m->cfg;
    const int64_t H = c.hidden_size, F = c.intermediate_size;
    add_param(m, "masked_spec_embed", {H});
    int64_t cin = 1;
    for (int i = 0; i < c.num_conv_layers; ++i) {
        const std::string b = "feature_extractor/conv_layers/" + std::to_string(i);
        add_param(m, b + "/conv/kernel", {c.kernal_sizes[i], cin, c.filter_sizes[i]});
        if (c.conv_bias) add_param(m, b + "/conv/bias", {c.filter_sizes[i]});
        if (c.feature_extractor_norm_type == 1 || i == 0) {
            add_param(m, b + "/layer_norm/gamma", {c.filter_sizes[i]});
            add_param(m, b + "/layer_norm/beta", {c.filter_sizes[i]});
        }
        cin = c.filter_sizes[i];
    }
    add_param(m, "feature_projection/layer_norm/gamma", {cin});
    add_param(m, "feature_projection/layer_norm/beta", {cin});
    add_param(m, "feature_projection/projection/kernel", {cin, H});
    add_param(m, "feature_projection/projection/bias", {H});
    const int64_t K = c.num_conv_pos_embeddings, G = c.num_conv_pos_embedding_groups;
    add_param(m, "encoder/pos_conv_embed/conv/bias", {H});
    add_param(m, "encoder/pos_conv_embed/conv/weight_g", {K, 1, 1});
    add_param(m, "encoder/pos_conv_embed/conv/weight_v", {K, H / G, H});
    add_param(m, "encoder/layer_norm/gamma", {H});
    add_param(m, "encoder/layer_norm/beta", {H});
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string b = "encoder/layers/" + std::to_string(i);
        for (const char* p : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
            add_param(m, b + "/attention/" + p + "/kernel", {H, H});
            add_param(m, b + "/attention/" + p + "/bias", {H});
        }
        add_param(m, b + "/layer_norm/gamma", {H});
        add_param(m, b + "/layer_norm/beta", {H});
        add_param(m, b + "/feed_forward/intermediate_dense/kernel", {H, F});
        add_param(m, b + "/feed_forward/intermediate_dense/bias", {F});
        add_param(m, b + "/feed_forward/output_dense/kernel", {F, H});
        add_param(m, b + "/feed_forward/output_dense/bias", {H});
        add_param(m, b + "/final_layer_norm/gamma", {H});
        add_param(m, b + "/final_layer_norm/beta", {H});
    }
    if (c.with_lm_head) {
        add_param(m, "lm_head/kernel", {H, c.vocab_size});
        add_param(m, "lm_head/bias", {c.vocab_size});
    }
}

void w2v2_free_planes(w2v2_model* m) {
    for (void* p : m->pl_allocs) (void)hipFree(p);
    m->pl_allocs.clear();
    m->conv48.clear();
    m->ln512_48 = m->attn_in48 = m->ctx48 = m->ffn_in48 = m->ffn48 = w2v2_model::PlaneBuf{};
    m->pl_fmt = -1;
    m->pl_B = 0;
    m->pl_L = 0;
}

static void free_workspace(w2v2_model* m) {
    w2v2_free_planes(m);
    for (void* p : m->allocs) (void)hipFree(p);
    m->allocs.clear();
    for (void* p : m->sh_allocs) (void)hipFree(p);
    m->sh_allocs.clear();
    m->conv16.clear();
    m->hs16.clear();
    m->sh_ready = false;
    m->pos_pack16 = nullptr;       // lives in `allocs`
    m->acts.clear();
    m->conv.clear();
    m->conv_T.clear();
    m->hs.clear();
    m->ws_B = 0;
    m->ws_L = 0;
    m->pk_L = 0;                   // the packed stream buffers live in `allocs`
    m->pk_wave = m->pk_scale = m->pk_out = nullptr;
    m->pk_tab = nullptr;
    m->pk_stats = nullptr;
    m->pk_gram = nullptr;
    m->pk_seg_cap = m->pk_tile_cap = 0;
}

int w2v2_ws_alloc(w2v2_model* m, float** out, int64_t floats) {
    void* p = nullptr;
    W2V2_HIP_CHECK(hipMalloc(&p, (size_t)(floats > 0 ? floats : 1) * sizeof(float)));
    m->allocs.push_back(p);
    *out = reinterpret_cast<float*>(p);
    return W2V2_OK;
}

int w2v2_ensure_workspace(w2v2_model* m, int B, int64_t L) {
    if (m->ws_B == B && m->ws_L == L) return W2V2_OK;
    free_workspace(m);
    const w2v2_config& c = m->cfg;
    const int64_t H = c.hidden_size, F = c.intermediate_size;
    int64_t T = L;
    for (int i = 0; i < c.num_conv_layers; ++i) {
        T = 1 + (T - c.kernal_sizes[i]) / c.strides[i];
        float* p = nullptr;
        if (int e = w2v2_ws_alloc(m, &p, (int64_t)B * T * c.filter_sizes[i])) return e;
        m->conv.push_back(p);
        m->conv_T.push_back((int)T);
        m->acts["conv" + std::to_string(i)] = Act{p, {B, T, c.filter_sizes[i]}};
    }
    const int64_t C = c.filter_sizes[c.num_conv_layers - 1];
    const int64_t BT = (int64_t)B * T;
    if (int e = w2v2_ws_alloc(m, &m->conv0_ws, conv0_ws_floats(B, L, c.kernal_sizes[0], c.strides[0], c.filter_sizes[0]))) return e;
    if (int e = w2v2_ws_alloc(m, &m->ln512, BT * C)) return e;
    if (int e = w2v2_ws_alloc(m, &m->proj, BT * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->posout, BT * H)) return e;
    m->acts["projection"] = Act{m->proj, {B, T, H}};
    for (int i = 0; i <= c.num_layers; ++i) {
        float* p = nullptr;
        if (c.attention_norm_type == 1 && i == 0) {
            p = m->posout;           // prenorm: encoder_in IS x + pos_conv(x)
        } else if (int e = w2v2_ws_alloc(m, &p, BT * H)) {
            return e;
        }
        m->hs.push_back(p);
        m->acts[i == 0 ? std::string("encoder_in") : "layer" + std::to_string(i - 1)] = Act{p, {B, T, H}};
    }
    if (int e = w2v2_ws_alloc(m, &m->qkv, BT * 3 * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->ctx, BT * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->t0, BT * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->t1, BT * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->t2, BT * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->t3, BT * H)) return e;
    if (int e = w2v2_ws_alloc(m, &m->ffn, BT * F)) return e;
    if (c.attention_norm_type == 1) {
        if (int e = w2v2_ws_alloc(m, &m->enc_out, BT * H)) return e;
    } else {
        m->enc_out = m->hs[c.num_layers];
    }
    m->acts["encoder_out"] = Act{m->enc_out, {B, T, H}};
    float* fl = nullptr;
    if (int e = w2v2_ws_alloc(m, &fl, B + 4)) return e;
    m->frame_len = reinterpret_cast<int32_t*>(fl);
    m->ws_B = B;
    m->ws_L = L;
    return W2V2_OK;
}

#ifdef W2V2_TUNING
namespace w2v2 {
int tune_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
}  // namespace w2v2
#endif

extern "C" {

const char* w2v2_last_error(void) { return g_err; }
int w2v2_release_scratch(void) { return w2v2::stream_scratch_release(); }
const char* w2v2_version(void) { return "w2v2-gfx950 0.1 (fp32 MFMA path; bf16-operand and bf16x3-split precision modes)"; }

int w2v2_create(const w2v2_config* cfg, w2v2_model** out) {
    W2V2_REQUIRE(cfg && out, "create: null argument");
    const w2v2_config& c = *cfg;
    W2V2_REQUIRE(c.num_conv_layers > 0 && c.num_conv_layers <= W2V2_MAX_CONV_LAYERS, "create: num_conv_layers=%d", c.num_conv_layers);
    W2V2_REQUIRE(c.hidden_size > 0 && c.num_heads > 0 && c.hidden_size % c.num_heads == 0,
                 "create: hidden_size %d is not a multiple of num_heads %d", c.hidden_size, c.num_heads);
    W2V2_REQUIRE(c.num_conv_pos_embedding_groups > 0 && c.hidden_size % c.num_conv_pos_embedding_groups == 0,
                 "create: hidden_size %d is not a multiple of the positional conv groups", c.hidden_size);
    W2V2_REQUIRE(c.feature_extractor_norm_type == 0 || c.feature_extractor_norm_type == 1, "create: bad conv norm type");
    W2V2_REQUIRE(c.attention_norm_type == 0 || c.attention_norm_type == 1, "create: bad attention norm type");
    W2V2_REQUIRE(c.num_layers >= 1 && c.intermediate_size > 0 && c.vocab_size > 0, "create: bad transformer sizes");
    for (int i = 0; i < c.num_conv_layers; ++i) {
        W2V2_REQUIRE(c.filter_sizes[i] > 0 && c.kernal_sizes[i] > 0 && c.strides[i] > 0, "create: bad conv layer %d", i);
        W2V2_REQUIRE(c.filter_sizes[i] % 4 == 0, "create: conv filters must be a multiple of 4");
    }
    w2v2_model* m = new w2v2_model();
    m->cfg = c;
    build_inventory(m);
    for (auto& p : m->params) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p.dev), (size_t)p.numel * sizeof(float));
        if (e == hipSuccess) e = hipMemset(p.dev, 0, (size_t)p.numel * sizeof(float));
        if (e != hipSuccess) {
            set_error("create: allocating `%s` failed: %s", p.name.c_str(), hipGetErrorString(e));
            w2v2_destroy(m);
            return W2V2_EHIP;
        }
    }
    m->prof = profiler_create();
    *out = m;
    return W2V2_OK;
}

void w2v2_destroy(w2v2_model* m) {
    if (!m) return;
    w2v2_comm_free(m);
    w2v2_train_destroy(m);
    free_workspace(m);
    for (auto& p : m->params)
        if (p.dev) (void)hipFree(p.dev);
    if (m->pos_wg) (void)hipFree(m->pos_wg);
    for (auto p : m->qkv_w) (void)hipFree(p);
    for (auto p : m->qkv_b) (void)hipFree(p);
    for (void* p : m->w16_allocs) (void)hipFree(p);
    for (auto& kv : m->w48)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& tab : m->wimg)
        for (auto& kv : tab) {
            if (kv.second.img) (void)hipFree(kv.second.img);
            if (kv.second.scale_ws) (void)hipFree(kv.second.scale_ws);
        }
    if (m->range_flag) (void)hipFree(m->range_flag);
    if (m->pos_w16) (void)hipFree(m->pos_w16);
    if (m->shadow_jobs) (void)hipFree(m->shadow_jobs);
    pinned_stage_free(m->pk_stage);
    profiler_destroy(m->prof);
    delete m;
}

int w2v2_num_params(const w2v2_model* m) { return m ? (int)m->params.size() : 0; }

int w2v2_param_info(const w2v2_model* m, int index, const char** name, int64_t shape[4], int* rank) {
    W2V2_REQUIRE(m && index >= 0 && index < (int)m->params.size(), "param_info: bad index %d", index);
    const Param& p = m->params[index];
    if (name) *name = p.name.c_str();
    if (rank) *rank = (int)p.shape.size();
    if (shape)
        for (size_t i = 0; i < 4; ++i) shape[i] = i < p.shape.size() ? p.shape[i] : 1;
    return W2V2_OK;
}

int w2v2_set_param(w2v2_model* m, const char* name, const float* host_src, const int64_t* shape, int rank) {
    W2V2_REQUIRE(m && name && host_src && shape, "set_param: null argument");
    auto it = m->index.find(name);
    if (it == m->index.end()) {
        set_error("set_param: unknown variable `%s`", name);
        return W2V2_ENOTFOUND;
    }
    Param& p = m->params[it->second];
    bool ok = rank == (int)p.shape.size();
    for (int i = 0; ok && i < rank; ++i) ok = shape[i] == p.shape[i];
    W2V2_REQUIRE(ok, "set_param: shape mismatch for `%s`", name);
    W2V2_HIP_CHECK(hipMemcpy(p.dev, host_src, (size_t)p.numel * sizeof(float), hipMemcpyHostToDevice));
    p.set = true;
    m->finalized = false;
    w2v2_train_invalidate(m);
    return W2V2_OK;
}

int w2v2_get_param(w2v2_model* m, const char* name, float* host_dst, int64_t numel) {
    W2V2_REQUIRE(m && name && host_dst, "get_param: null argument");
    auto it = m->index.find(name);
    if (it == m->index.end()) {
        set_error("get_param: unknown variable `%s`", name);
        return W2V2_ENOTFOUND;
    }
    Param& p = m->params[it->second];
    W2V2_REQUIRE(numel == p.numel, "get_param: `%s` has %lld elements, caller asked for %lld", name,
                 (long long)p.numel, (long long)numel);
    W2V2_HIP_CHECK(hipDeviceSynchronize());
    W2V2_HIP_CHECK(hipMemcpy(host_dst, p.dev, (size_t)p.numel * sizeof(float), hipMemcpyDeviceToHost));
    return W2V2_OK;
}

int w2v2_finalize(w2v2_model* m, void* stream) {
    W2V2_REQUIRE(m, "finalize: null model");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const w2v2_config& c = m->cfg;
    const int64_t H = c.hidden_size;
    const int K = c.num_conv_pos_embeddings, G = c.num_conv_pos_embedding_groups, cg = (int)(H / G);
    if (!m->pos_wg) W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->pos_wg), (size_t)K * cg * H * sizeof(float)));
    if (int e = launch_weight_norm_regroup(m->prof, m->P("encoder/pos_conv_embed/conv/weight_v"),
                                           m->P("encoder/pos_conv_embed/conv/weight_g"), m->pos_wg, K, cg,
                                           (int)H, G, s))
        return e;
    // packed q|k|v projection: one (H, 3H) GEMM per layer instead of three (H, H)
    if (m->qkv_w.empty()) {
        m->qkv_w.resize(c.num_layers, nullptr);
        m->qkv_b.resize(c.num_layers, nullptr);
        for (int i = 0; i < c.num_layers; ++i) {
            W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->qkv_w[i]), (size_t)H * 3 * H * sizeof(float)));
            W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->qkv_b[i]), (size_t)3 * H * sizeof(float)));
        }
    }
    if (H % 4 == 0 && c.num_layers > 0) {       // all layers in one launch (24 per launch): this runs after every optimizer step
        std::vector<const float*> wl(3 * (size_t)c.num_layers), bl(3 * (size_t)c.num_layers);
        for (int i = 0; i < c.num_layers; ++i) {
            const std::string b = "encoder/layers/" + std::to_string(i) + "/attention/";
            const char* names[3] = {"q_proj", "k_proj", "v_proj"};
            for (int j = 0; j < 3; ++j) {
                wl[3 * i + j] = m->P(b + names[j] + "/kernel");
                bl[3 * i + j] = m->P(b + names[j] + "/bias");
            }
        }
        if (int e = launch_qkv_pack_layers(m->qkv_w.data(), m->qkv_b.data(), wl.data(), bl.data(), c.num_layers, H, s)) return e;
    }
    for (int i = 0; i < c.num_layers && H % 4 != 0; ++i) {
        const std::string b = "encoder/layers/" + std::to_string(i) + "/attention/";
        const char* names[3] = {"q_proj", "k_proj", "v_proj"};
        const float* wj[3];
        const float* bj[3];
        for (int j = 0; j < 3; ++j) {
            wj[j] = m->P(b + names[j] + "/kernel");
            bj[j] = m->P(b + names[j] + "/bias");
        }
        {
            for (int j = 0; j < 3; ++j) {
                W2V2_HIP_CHECK(hipMemcpy2DAsync(m->qkv_w[i] + j * H, (size_t)3 * H * sizeof(float), wj[j], (size_t)H * sizeof(float),
                                                (size_t)H * sizeof(float), (size_t)H, hipMemcpyDeviceToDevice, s));
                W2V2_HIP_CHECK(hipMemcpyAsync(m->qkv_b[i] + j * H, bj[j], (size_t)H * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
        }
    }
    m->finalized = true;
    m->w16_valid = false;      // the bf16 weight shadows (if any) follow the variables
    ++m->w48_epoch;
    m->pos16_valid = false;
    return W2V2_OK;
}

int64_t w2v2_num_frames(const w2v2_model* m, int64_t n) {
    if (!m) return -1;
    for (int i = 0; i < m->cfg.num_conv_layers; ++i) {
        if (n < m->cfg.kernal_sizes[i]) return 0;
        n = 1 + (n - m->cfg.kernal_sizes[i]) / m->cfg.strides[i];
    }
    return n;
}

int w2v2_set_precision(w2v2_model* m, int32_t mode) {
    W2V2_REQUIRE(m, "set_precision: null model");
    W2V2_REQUIRE(mode >= W2V2_PRECISION_FP32 && mode <= W2V2_PRECISION_F16X2, "set_precision: unknown mode %d", mode);
    m->precision = mode;
    return W2V2_OK;
}
int w2v2_get_precision(const w2v2_model* m) { return m ? m->precision : W2V2_EINVAL; }

int w2v2_set_option(w2v2_model* m, int32_t option, int32_t value) {
    W2V2_REQUIRE(m, "set_option: null model");
    switch (option) {
        case W2V2_OPT_BF16_SHADOWS: m->opt_shadows = value != 0; return W2V2_OK;
        case W2V2_OPT_KEEP_ACTIVATIONS: m->opt_keep_acts = value != 0; return W2V2_OK;
        case W2V2_OPT_SPLIT_PLANES: m->opt_planes = value != 0; return W2V2_OK;
        case W2V2_OPT_WGRAD_STREAM: m->opt_wgrad_stream = value != 0; return W2V2_OK;
        case W2V2_OPT_DEFER_FOLDS: m->opt_defer_folds = value != 0; return W2V2_OK;
        case W2V2_OPT_BF16_PACKED: m->opt_bf16_packed = value != 0; return W2V2_OK;
        default: set_error("set_option: unknown option %d", option); return W2V2_EINVAL;
    }
}
int w2v2_get_option(const w2v2_model* m, int32_t option) {
    if (!m) return W2V2_EINVAL;
    switch (option) {
        case W2V2_OPT_BF16_SHADOWS: return m->opt_shadows ? 1 : 0;
        case W2V2_OPT_KEEP_ACTIVATIONS: return m->opt_keep_acts ? 1 : 0;
        case W2V2_OPT_SPLIT_PLANES: return m->opt_planes ? 1 : 0;
        case W2V2_OPT_WGRAD_STREAM: return m->opt_wgrad_stream ? 1 : 0;
        case W2V2_OPT_DEFER_FOLDS: return m->opt_defer_folds ? 1 : 0;
        case W2V2_OPT_BF16_PACKED: return m->opt_bf16_packed ? 1 : 0;
        default: return W2V2_EINVAL;
    }
}

int w2v2_range_overflow(w2v2_model* m, int32_t* flag, void* stream) {
    W2V2_REQUIRE(m && flag, "range_overflow: null argument");
    *flag = 0;
    if (!m->range_flag) return W2V2_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int v = 0;
    W2V2_HIP_CHECK(hipMemcpyAsync(&v, m->range_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    W2V2_HIP_CHECK(hipStreamSynchronize(s));
    if (v) W2V2_HIP_CHECK(hipMemsetAsync(m->range_flag, 0, sizeof(int), s));
    *flag = v != 0;
    return W2V2_OK;
}

int w2v2_ctc_loss(const float* logits, int32_t B, int32_t T, int32_t V, const int32_t* labels, int32_t U,
                  const int32_t* label_length, const int32_t* logit_length, int32_t blank, float* nll,
                  float* grad, void* stream) {
    return launch_ctc(nullptr, logits, B, T, V, labels, U, label_length, logit_length, blank, nll, grad,
                      reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_loss_fused(const float* logits, int32_t B, int32_t T, int32_t V, const int32_t* labels, int32_t U, int32_t logit_length_all,
                        int32_t blank, float division_factor, float* nll, float* grad, float* loss_sum, void* stream) {
    W2V2_REQUIRE(logit_length_all > 0, "ctc_loss_fused: logit_length_all must be positive");
    W2V2_REQUIRE(division_factor > 0.f, "ctc_loss_fused: division_factor must be positive");
    return launch_ctc_x(w2v2::tl_step_prof, logits, B, T, V, labels, U, nullptr, nullptr, logit_length_all, blank, division_factor, nll, grad, loss_sum,
                        reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_align(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                   const int64_t* label0, const int32_t* nlabels, int32_t blank, int32_t* token, int32_t* label_index, float* frame_logp,
                   double* score, void* stream) {
    return launch_ctc_align(logits, V, n, row0, frames, labels, label0, nlabels, blank, token, label_index, frame_logp, score,
                            reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_align_star(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                        const int64_t* label0, const int32_t* nlabels, int32_t blank, float star_score, int32_t* token,
                        int32_t* label_index, float* frame_logp, double* score, void* stream) {
    return launch_ctc_align_star(logits, V, n, row0, frames, labels, label0, nlabels, blank, star_score, token, label_index, frame_logp,
                                 score, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_align_long(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                        const int64_t* label0, const int32_t* nlabels, int32_t blank, int32_t* token, int32_t* label_index,
                        float* frame_logp, double* score, int32_t strip_pairs, int32_t panel_frames, int64_t max_workspace_bytes,
                        void* stream) {
    return launch_ctc_align_long(logits, V, n, row0, frames, labels, label0, nlabels, blank, token, label_index, frame_logp, score,
                                 strip_pairs, panel_frames, max_workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

int64_t w2v2_ctc_align_long_workspace(int32_t n, const int32_t* frames, const int32_t* nlabels, int32_t strip_pairs,
                                      int32_t panel_frames) {
    return ctc_align_long_workspace(n, frames, nlabels, strip_pairs, panel_frames);
}

int w2v2_ctc_align_long_star(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames,
                             const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int32_t blank, float star_score,
                             int32_t* token, int32_t* label_index, float* frame_logp, double* score, int32_t strip_pairs,
                             int32_t panel_frames, int64_t max_workspace_bytes, void* stream) {
    return launch_ctc_align_long(logits, V, n, row0, frames, labels, label0, nlabels, blank, token, label_index, frame_logp, score,
                                 strip_pairs, panel_frames, max_workspace_bytes, reinterpret_cast<hipStream_t>(stream), true, star_score);
}

int64_t w2v2_ctc_align_long_star_workspace(int32_t n, const int32_t* frames, const int32_t* nlabels, int32_t strip_pairs,
                                           int32_t panel_frames) {
    return ctc_align_long_workspace(n, frames, nlabels, strip_pairs, panel_frames, true);
}

int w2v2_ctc_score(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t m, const int32_t* utt_of,
                   const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int32_t blank, double* logp, void* stream) {
    return launch_ctc_score(logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels, blank, false, 0.f, logp,
                            reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_score_grad(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t m,
                        const int32_t* utt_of, const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int32_t blank,
                        const double* coef, double* logp, float* grad, int64_t max_workspace_bytes, void* stream) {
    return launch_ctc_score_grad(logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels, blank, false, 0.f, coef, logp, grad,
                                 max_workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

int64_t w2v2_ctc_score_grad_workspace(int32_t n, const int32_t* frames, int32_t m, const int32_t* utt_of, const int32_t* nlabels,
                                      int32_t V) {
    return ctc_score_grad_workspace(n, frames, m, utt_of, nlabels, V, false);
}

int w2v2_ctc_score_star(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t m,
                        const int32_t* utt_of, const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int32_t blank,
                        float star_score, double* logp, void* stream) {
    return launch_ctc_score(logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels, blank, true, star_score, logp,
                            reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_score_grad_star(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t m,
                             const int32_t* utt_of, const int32_t* labels, const int64_t* label0, const int32_t* nlabels,
                             int32_t blank, float star_score, const double* coef, double* logp, float* grad,
                             int64_t max_workspace_bytes, void* stream) {
    return launch_ctc_score_grad(logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels, blank, true, star_score, coef, logp,
                                 grad, max_workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

int64_t w2v2_ctc_score_grad_star_workspace(int32_t n, const int32_t* frames, int32_t m, const int32_t* utt_of,
                                           const int32_t* nlabels, int32_t V) {
    return ctc_score_grad_workspace(n, frames, m, utt_of, nlabels, V, true);
}

int w2v2_ctc_spot(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t m, const int32_t* utt_of,
                  const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int32_t blank, int32_t delim,
                  const double* min_score, int32_t max_hits, double* hit_score, int32_t* hit_begin, int32_t* hit_end, int32_t* count,
                  double* trace_score, int32_t* trace_begin, const int64_t* trace0, void* stream) {
    return launch_ctc_spot(logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels, blank, delim, min_score, max_hits, hit_score,
                           hit_begin, hit_end, count, trace_score, trace_begin, trace0, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_beam_search(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t blank,
                         int32_t beam_width, int32_t nbest, const float* lm_table, int32_t lm_order, float lm_alpha, float lm_beta,
                         int32_t max_len, int32_t* labels_out, int32_t* length, double* score, double* total, void* stream) {
    return launch_ctc_beam_search(logits, V, n, row0, frames, blank, beam_width, nbest, lm_table, lm_order, lm_alpha, lm_beta, max_len,
                                  labels_out, length, score, total, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_beam_search_words(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t blank,
                               int32_t beam_width, int32_t nbest, const w2v2_word_lm* lm, int32_t delim, float lm_alpha, float lm_beta,
                               float unk_penalty, int32_t score_eos, int32_t max_len, int32_t* labels_out, int32_t* length,
                               double* score, double* total, void* stream) {
    return launch_ctc_beam_search_words(logits, V, n, row0, frames, blank, beam_width, nbest, lm, delim, lm_alpha, lm_beta, unk_penalty,
                                        score_eos, max_len, labels_out, length, score, total, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_beam_search_biased(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t blank,
                                int32_t beam_width, int32_t nbest, const float* lm_table, int32_t lm_order, const w2v2_word_lm* word_lm,
                                int32_t delim, float lm_alpha, float lm_beta, float unk_penalty, int32_t score_eos,
                                const w2v2_ctc_bias* bias, int32_t max_len, int32_t* labels_out, int32_t* length, double* score,
                                double* total, void* stream) {
    return launch_ctc_beam_search_biased(logits, V, n, row0, frames, blank, beam_width, nbest, lm_table, lm_order, word_lm, delim, lm_alpha,
                                         lm_beta, unk_penalty, score_eos, bias, max_len, labels_out, length, score, total,
                                         reinterpret_cast<hipStream_t>(stream));
}

int64_t w2v2_ctc_beam_stream_state_bytes(void) { return ctc_beam_stream_state_bytes(); }

int w2v2_ctc_beam_search_stream(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames,
                                const int64_t* frames_done, int32_t blank, int32_t beam_width, int32_t nbest, const float* lm_table,
                                int32_t lm_order, const w2v2_word_lm* word_lm, int32_t delim, float lm_alpha, float lm_beta,
                                float unk_penalty, int32_t score_eos, const w2v2_ctc_bias* bias, void* state, uint64_t* nodes,
                                const int64_t* node0, const int64_t* node_cap, int32_t max_len, int32_t* labels_out, int32_t* length,
                                double* score, double* total, int32_t* stable_len, void* stream) {
    return launch_ctc_beam_search_stream(logits, V, n, row0, frames, frames_done, blank, beam_width, nbest, lm_table, lm_order, word_lm,
                                         delim, lm_alpha, lm_beta, unk_penalty, score_eos, bias, state, nodes, node0, node_cap, max_len,
                                         labels_out, length, score, total, stable_len, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_ctc_pause_cuts(const float* logits, int32_t V, int32_t n, const int64_t* row0, const int32_t* frames, int32_t blank,
                        int32_t delim, float margin, int32_t min_pause, int32_t max_cuts, int32_t* cut, int32_t* pause, int32_t* count,
                        void* stream) {
    return launch_ctc_pause_cuts(logits, V, n, row0, frames, blank, delim, margin, min_pause, max_cuts, cut, pause, count,
                                 reinterpret_cast<hipStream_t>(stream));
}

int w2v2_edit_distance(const int32_t* tokens, int64_t n_tokens, int32_t n_pairs, const int64_t* hyp0, const int32_t* hyp_len,
                       const int64_t* ref0, const int32_t* ref_len, int32_t* out, void* stream) {
    return launch_edit_distance(tokens, n_tokens, n_pairs, hyp0, hyp_len, ref0, ref_len, out, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_resample_design(int32_t rate_in, int32_t rate_out, int32_t zeros, double rolloff, double beta, int32_t* L, int32_t* M,
                         int32_t* K, int32_t* lead, float* table, int64_t table_capacity) {
    return resample_design(rate_in, rate_out, zeros, rolloff, beta, L, M, K, lead, table, table_capacity);
}

int64_t w2v2_resample_length(int64_t len, int32_t L, int32_t M) { return resample_length(len, L, M); }

int w2v2_resample(const float* in, int32_t n, const int64_t* in0, const int64_t* in_len, const int32_t* filter_of,
                  const w2v2_resample_filter* filters, int32_t n_filters, float* out, const int64_t* out0, void* stream) {
    return launch_resample(in, n, in0, in_len, filter_of, filters, n_filters, out, out0, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_fir(const float* in, int32_t n, const int64_t* in0, const int64_t* len, const float* taps, const int64_t* taps0, const int32_t* ntaps,
             const int32_t* delay, float* out, const int64_t* out0, int32_t match_power, float* gain, void* stream) {
    return launch_fir(in, n, in0, len, taps, taps0, ntaps, delay, out, out0, match_power, gain, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_mix(const float* in, int32_t n, const int64_t* in0, const int64_t* len, const float* noise, const int64_t* noise0,
             const int64_t* noise_len, const int64_t* offset, const double* scale, float* out, const int64_t* out0, float* gain, void* stream) {
    return launch_mix(in, n, in0, len, noise, noise0, noise_len, offset, scale, out, out0, gain, reinterpret_cast<hipStream_t>(stream));
}

int w2v2_activation_info(const w2v2_model* m, const char* name, int64_t shape[3]) {
    W2V2_REQUIRE(m && name && shape, "activation_info: null argument");
    auto it = m->acts.find(name);
    if (it == m->acts.end()) {
        set_error("activation `%s` does not exist (run a forward first)", name);
        return W2V2_ENOTFOUND;
    }
    for (int i = 0; i < 3; ++i) shape[i] = it->second.shape[i];
    return W2V2_OK;
}

int w2v2_copy_activation(w2v2_model* m, const char* name, float* host_dst, int64_t numel, void* stream) {
    W2V2_REQUIRE(m && name && host_dst, "copy_activation: null argument");
    auto it = m->acts.find(name);
    if (it == m->acts.end()) {
        set_error("activation `%s` does not exist (run a forward first)", name);
        return W2V2_ENOTFOUND;
    }
    const Act& a = it->second;
    W2V2_REQUIRE(numel == a.shape[0] * a.shape[1] * a.shape[2], "copy_activation: `%s` element count mismatch", name);
    for (const std::string& skipped : m->acts_skipped)
        if (skipped == name) {
            set_error("activation `%s` was written only as bf16 by the last forward (precision mode bf16: its one consumer reads the "
                      "shadow); w2v2_set_option(m, W2V2_OPT_KEEP_ACTIVATIONS, 1) keeps the fp32 copy", name);
            return W2V2_ESTATE;
        }
    W2V2_HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    W2V2_HIP_CHECK(hipMemcpy(host_dst, a.ptr, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return W2V2_OK;
}

int w2v2_profile_enable(w2v2_model* m, int enable) {
    W2V2_REQUIRE(m, "profile_enable: null model");
    profiler_enable(m->prof, enable != 0);
    return W2V2_OK;
}
int w2v2_profile_families(w2v2_model* m, uint32_t family_mask) {
    W2V2_REQUIRE(m, "profile_families: null model");
    profiler_set_mask(m->prof, family_mask);
    return W2V2_OK;
}
int w2v2_profile_sampling(w2v2_model* m, int32_t stride) {
    W2V2_REQUIRE(m && stride >= 1, "profile_sampling: bad argument");
    profiler_set_stride(m->prof, stride);
    return W2V2_OK;
}
int w2v2_profile_seen(w2v2_model* m, int index, int64_t* launches) {
    W2V2_REQUIRE(m && index >= 0 && index < FAM_COUNT && launches, "profile_seen: bad argument");
    *launches = profiler_seen(m->prof, index);
    return W2V2_OK;
}
int w2v2_profile_num_families(void) { return FAM_COUNT; }
int w2v2_profile_read(w2v2_model* m, int index, const char** name, int64_t* launches, double* total_ms,
                      double* flops, double* bytes) {
    W2V2_REQUIRE(m && index >= 0 && index < FAM_COUNT && launches && total_ms && flops && bytes, "profile_read: bad argument");
    if (name) *name = family_name(index);
    return profiler_read(m->prof, index, launches, total_ms, flops, bytes);
}
int w2v2_profile_kernel_launches(w2v2_model* m, int index, int64_t* launches) {
    W2V2_REQUIRE(m && launches, "profile_kernel_launches: null argument");
    W2V2_REQUIRE(index >= 0 && index < FAM_COUNT, "profile_kernel_launches: bad family index %d", index);
    *launches = profiler_kernel_launches(m->prof, index);
    return W2V2_OK;
}
int w2v2_profile_reset(w2v2_model* m) {
    W2V2_REQUIRE(m, "profile_reset: null model");
    profiler_reset(m->prof);
    return W2V2_OK;
}

// ---- single operators ---------------------------------------------------------
int w2v2_op_gemm(const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, float* C,
                 int64_t ldc, int64_t strideC, const float* bias, const float* residual, int32_t M,
                 int32_t N, int32_t K, int32_t nbatch, int32_t act, void* stream) {
    return launch_gemm(nullptr, A, lda, strideA, B, ldb, C, ldc, strideC, bias, residual, M, N, K, nbatch, act,
                       reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_variant(const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, float* C,
                         int64_t ldc, int64_t strideC, const float* bias, const float* residual, int32_t M,
                         int32_t N, int32_t K, int32_t nbatch, int32_t act, int32_t variant, void* stream) {
    W2V2_REQUIRE(variant >= -1 && variant <= 2, "op_gemm_variant: variant %d (-1 by shape, 0 double buffer, 1 ring, 2 persistent ring)", variant);
    gemm_f32_force_ring(variant);
    const int e = launch_gemm(nullptr, A, lda, strideA, B, ldb, C, ldc, strideC, bias, residual, M, N, K, nbatch, act,
                              reinterpret_cast<hipStream_t>(stream));
    gemm_f32_force_ring(-1);
    return e;
}
int w2v2_op_set_precision(int32_t mode) {
    W2V2_REQUIRE(mode >= W2V2_PRECISION_FP32 && mode <= W2V2_PRECISION_F16X2, "op_set_precision: unknown mode %d", mode);
    gemm_set_precision(mode);
    return W2V2_OK;
}
int w2v2_op_gemm_bf16(const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, float* C,
                      int64_t ldc, int64_t strideC, const float* bias, const float* residual, int32_t M,
                      int32_t N, int32_t K, int32_t nbatch, int32_t act, void* stream) {
    return launch_gemm_bf16(nullptr, A, lda, strideA, B, ldb, 0, C, ldc, strideC, bias, residual, M, N, K, nbatch, act,
                            reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_bf16_shadows(const uint16_t* A16, int64_t lda, int64_t strideA, const uint16_t* B16, float* C, uint16_t* C16, int64_t ldc,
                              int64_t strideC, const float* bias, const float* residual, int32_t M, int32_t N, int32_t K, int32_t nbatch,
                              int32_t act, int32_t variant, void* stream) {
    W2V2_REQUIRE(A16 && B16 && (C || C16), "op_gemm_bf16_shadows: null operand");
    W2V2_REQUIRE(variant >= 0 && variant <= 2, "op_gemm_bf16_shadows: variant %d (0 by shape, 1 = 128 x 128 tiles, 2 = 128 x 256 software-pipelined)", variant);
    W2V2_REQUIRE(variant != 2 || gemm_bf16_sw_ok(M, N, K, lda, K, strideA),
                 "op_gemm_bf16_shadows: variant 2 needs N %% 256 == 0, K %% 64 == 0, K >= 192 and 16-byte aligned rows");
    GemmShadows x;
    x.A16 = A16; x.B16 = B16; x.C16 = C16; x.ldb16 = K; x.force_kernel = variant;
    return launch_gemm_bf16_x(nullptr, nullptr, lda, strideA, nullptr, N, 0, C, ldc, strideC, bias, residual, M, N, K, nbatch, act, x,
                              reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_split(const float* A, int64_t lda, int64_t strideA, const float* B, float* C, int64_t ldc, int64_t strideC,
                       const float* bias, const float* residual, int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act,
                       void* stream) {
    W2V2_REQUIRE(A && B && C && N > 0 && K > 0, "op_gemm_split: null operand");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint16_t* planes = nullptr;
    W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&planes), (size_t)3 * K * N * sizeof(uint16_t)));
    int e = launch_split_weight(B, planes, K, N, s);
    if (!e) e = launch_gemm_split(nullptr, A, lda, strideA, planes, C, ldc, strideC, bias, residual, M, N, K, nbatch, act, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(planes);
    return e;
}
int w2v2_op_check_select_forms(uint64_t* mismatches, void* stream) {
    return launch_check_select_forms(reinterpret_cast<unsigned long long*>(mismatches), reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_check_gelu_epilogue(uint64_t* mismatches, void* stream) {
    return launch_check_gelu_epilogue(reinterpret_cast<unsigned long long*>(mismatches), reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gelu_reference(const float* x, float* y, int64_t n, void* stream) {
    return launch_gelu_reference(x, y, n, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_ring_launches(int64_t* counts) {
    W2V2_REQUIRE(counts, "op_gemm_ring_launches: null argument");
    gemm_f32_ring_launches(counts);
    return W2V2_OK;
}
int w2v2_op_gemm_f32_route(int32_t M, int32_t N, int32_t K, int32_t nbatch, int64_t lda, int64_t ldb, int64_t ldc, int64_t strideA, int64_t strideB,
                           int32_t act, int32_t has_bias, int32_t has_residual, int32_t ab_aligned, int32_t c_aligned, int32_t variant, int32_t* out) {
    W2V2_REQUIRE(out && M > 0 && N > 0 && K > 0 && nbatch > 0 && variant >= -1 && variant <= 2, "op_gemm_f32_route: bad argument");
    const GemmF32Route r = gemm_f32_route(GemmF32Problem{M, N, K, nbatch, lda, ldb, ldc, strideA, strideB, act, has_bias != 0, has_residual != 0,
                                                         ab_aligned != 0, c_aligned != 0, variant});
    const int32_t v[8] = {r.kind, r.kernel[0], r.kernel[1], r.S, (int32_t)r.main_tiles, r.main_rows, r.persist, r.kind == GR_ONE ? 1 : 2};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return W2V2_OK;
}
int w2v2_op_gemm_bf16_route(const int64_t* q, int32_t* out) {
    W2V2_REQUIRE(q && out && q[0] > 0 && q[1] > 0 && q[2] > 0 && q[3] > 0, "op_gemm_bf16_route: bad argument");
    GemmBf16Problem p;
    p.M = (int)q[0]; p.N = (int)q[1]; p.K = (int)q[2]; p.nbatch = (int)q[3];
    p.lda = q[4]; p.ldb = q[5]; p.strideA = q[6]; p.strideB = q[7]; p.ldb16 = q[8] ? q[8] : q[2];
    p.A = (int)q[9]; p.B = (int)q[10]; p.A16 = (int)q[11]; p.B16 = (int)q[12]; p.B16p = (int)q[13];
    p.C = q[14] != 0; p.C16 = q[15] != 0;
    p.transA = q[16] != 0; p.zmod = (int)q[17]; p.colsum = q[18] != 0; p.overlapA = q[19] != 0;
    p.validK = q[20]; p.kextra = (int)q[21]; p.b_zero_row = q[22] != 0; p.force_kernel = (int)q[23];
    const GemmBf16Route r = gemm_bf16_route(p);
    const int32_t v[5] = {r.kernel, r.krag, r.refusal, r.a_bytes, r.b_bytes};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
    return W2V2_OK;
}
static WgProblem wg_problem(const int64_t* q) {
    return WgProblem{(int)q[0], (int)q[1], (int)q[2], (int)q[3], q[4] != 0, q[5] != 0, q[6] != 0, q[7] != 0, q[8] != 0, q[9] != 0, q[10] != 0, q[11] != 0,
                     q[12], q[13], q[14], (int)q[15], (int)q[16]};
}
int w2v2_op_weight_grad_plan(const int64_t* q, int64_t* out) {
    W2V2_REQUIRE(q && out && q[0] > 0 && q[1] > 0 && q[2] > 0 && q[0] <= INT32_MAX && q[1] <= INT32_MAX && q[2] <= INT32_MAX && q[12] >= 0 && q[13] >= 0 &&
                     q[14] >= 0 && q[15] > 0,
                 "op_weight_grad_plan: bad argument");
    const WgPlan p = weight_grad_plan(wg_problem(q));
    const int64_t v[18] = {p.refusal, p.form, p.kernel, p.kq, p.cap, p.S, p.Kp, p.kextra, p.validK, p.b_zero_row, p.Mq, p.R, p.tail, p.nslabs, p.dst, p.fold,
                           p.bias, wg_max_slabs(q[1], q[2])};
    for (int i = 0; i < 18; ++i) out[i] = v[i];
    return W2V2_OK;
}
int w2v2_op_weight_grad(const int64_t* problem, const float* A, const float* dY, const uint16_t* A16, const uint16_t* dY16, float* dW, float* db,
                        float* slabs, float* at, int64_t at_floats, float* cs_ws, float* red_ws, int64_t red_ws_floats, void* stream) {
    int64_t unused[18];
    if (int e = w2v2_op_weight_grad_plan(problem, unused)) return e;
    const WgProblem q = wg_problem(problem);
    W2V2_REQUIRE(q.precision == gemm_get_precision(), "op_weight_grad: the problem says precision %d, w2v2_op_set_precision set %d", q.precision, gemm_get_precision());
    W2V2_REQUIRE(q.A == (A != nullptr) && q.dY == (dY != nullptr) && q.A16 == (A16 != nullptr) && q.dY16 == (dY16 != nullptr) && q.want_dW == (dW != nullptr) &&
                     q.want_db == (db != nullptr) && !q.unpack,
                 "op_weight_grad: the problem's operand flags disagree with the pointers (and the unpacking fold is the training step's)");
    const WgPlan p = weight_grad_plan(q);
    W2V2_REQUIRE(p.refusal == WGR_NONE, "%s", weight_grad_refusal_text(p.refusal));
    W2V2_REQUIRE(p.dst != WG_TO_SLABS || slabs, "op_weight_grad: this plan writes slabs");
    const bool copies = p.form == WG_DIV_F32_COPY || p.tail == WG_TAIL_COPY;
    W2V2_REQUIRE(!copies || (at && at_floats >= (int64_t)q.Kin * q.M), "op_weight_grad: this plan needs Kin M floats for the transposed copy");
    W2V2_REQUIRE(p.bias != WG_BIAS_FUSED || cs_ws, "op_weight_grad: this plan writes per-slab column sums");
    W2V2_REQUIRE(p.bias == WG_BIAS_NONE || (red_ws && red_ws_floats >= colsum_ws_floats(q.M, q.Nout)), "op_weight_grad: reduction scratch too small");
    return launch_weight_grad(nullptr, q, p, A, dY, A16, dY16, dW, db, WgScratch{slabs, at, cs_ws, red_ws}, nullptr, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_bf16_launches(int64_t* counts) {
    W2V2_REQUIRE(counts, "op_gemm_bf16_launches: null argument");
    gemm_bf16_launches(counts);
    return W2V2_OK;
}
int w2v2_op_attention_route(const int32_t* q, int32_t* out) {
    W2V2_REQUIRE(q && out && q[0] >= AP_INFER && q[0] <= AP_BWD && q[2] > 0 && q[3] > 0 && q[4] > 0 && q[5] > 0 && q[4] % q[5] == 0,
                 "op_attention_route: bad argument");
    const AttnRoute r = attention_route(AttnProblem{q[0], q[1], q[2], q[3], q[4], q[5], q[6] != 0, q[7] != 0, q[8] != 0, q[9] != 0, q[10] != 0, q[11] != 0});
    const int32_t v[10] = {r.kernel, r.refusal, r.family, r.fmt, r.dh, r.waves, r.rows, r.lse_log2, r.writes_b16, r.writes_planes};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return W2V2_OK;
}
int w2v2_op_attention_launches(int64_t* counts) {
    W2V2_REQUIRE(counts, "op_attention_launches: null argument");
    attention_launches(counts);
    return W2V2_OK;
}
int w2v2_op_split_planes(const float* x, uint16_t* planes, int64_t plane_stride, int64_t n, int32_t fmt, int32_t* range_flag, void* stream) {
    W2V2_REQUIRE(fmt == PF_BF16X3 || fmt == PF_F16X2, "op_split_planes: unknown plane format %d", fmt);
    return launch_split_planes(x, planes, plane_stride, n, fmt, range_flag, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_split_weight(const float* B, uint16_t* images, float* scale_ws, int32_t K, int32_t N, int32_t fmt, void* stream) {
    W2V2_REQUIRE(fmt == PF_BF16X3 || fmt == PF_F16X2, "op_split_weight: unknown plane format %d", fmt);
    return launch_split_weight_sw(B, images, K, N, fmt, scale_ws, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_split_planes(int32_t fmt, const uint16_t* A16, int64_t planeA, int64_t lda, int64_t strideA, const uint16_t* Bimg,
                              const float* out_scale, float* C, uint16_t* C16, int64_t planeC, int64_t ldc, int64_t strideC,
                              const float* bias, const float* residual, int32_t M, int32_t N, int32_t K, int32_t nbatch, int32_t act,
                              int32_t* range_flag, void* stream) {
    return launch_gemm_split_sw(nullptr, fmt, A16, planeA, lda, strideA, Bimg, out_scale, C, C16, planeC, ldc, strideC, bias, residual, M, N, K,
                                nbatch, act, range_flag, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_gemm_bf16_at(const float* At, int64_t lda, int64_t strideA, const float* B, int64_t ldb, int64_t strideB,
                         float* C, int64_t ldc, int64_t strideC, int32_t M, int32_t N, int32_t K, int32_t nbatch, void* stream) {
    GemmShadows x;
    x.transA = true;
    return launch_gemm_bf16_x(nullptr, At, lda, strideA, B, ldb, strideB, C, ldc, strideC, nullptr, nullptr, M, N, K, nbatch, 0, x,
                              reinterpret_cast<hipStream_t>(stream));
}
// slicing-by-8 CRC-32C (reflected polynomial 0x82F63B78): ~1 GB/s on the host, a base checkpoint is 0.38 GB
uint32_t w2v2_crc32c_extend(uint32_t crc, const void* data, uint64_t n) {
    static uint32_t T[8][256];
    static std::atomic<bool> ready{false};
    static std::mutex mu;
    if (!ready) {
        std::lock_guard<std::mutex> lk(mu);
        if (!ready) {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
                T[0][i] = c;
            }
            for (uint32_t i = 0; i < 256; ++i)
                for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFFu];
            ready = true;
        }
    }
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint32_t c = crc ^ 0xFFFFFFFFu;
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T[7][lo & 0xFFu] ^ T[6][(lo >> 8) & 0xFFu] ^ T[5][(lo >> 16) & 0xFFu] ^ T[4][lo >> 24] ^ T[3][hi & 0xFFu] ^
            T[2][(hi >> 8) & 0xFFu] ^ T[1][(hi >> 16) & 0xFFu] ^ T[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
int w2v2_op_weight_grad_bf16(const uint16_t* x16, const uint16_t* dy16, float* slabs, int64_t rows, int32_t Kin, int32_t Nout,
                             int32_t rows_per_slab, int32_t nslabs, int32_t variant, void* stream) {
    W2V2_REQUIRE(x16 && dy16 && slabs && rows > 0 && rows_per_slab > 0 && nslabs > 0 && Kin % 128 == 0 && Nout % 128 == 0 &&
                     rows_per_slab % 64 == 0 && variant >= 0 && variant <= 3, "op_weight_grad_bf16: bad argument");
    // variants 2 and 3 also take uneven slabs: with u = ceil(rows / 64) K tiles in all, u - nslabs (rows_per_slab / 64) = e, 0 <= e < nslabs,
    // gives the first e slabs one K tile more (GemmShadows::kextra -- how the training step cuts B T rows into any number of slabs).
    // variant 3 additionally promises that row `rows` of dy16 exists and is all-zero, which lets the last K tile be short.
    const bool sw = variant == 2 || variant == 3;
    const WgUneven u = wg_uneven_slabs(rows, nslabs);
    const bool shape_ok = sw && u.Kp == rows_per_slab && (u.validK == 0 || variant == 3);
    W2V2_REQUIRE(!sw || (shape_ok && gemm_bf16_swtr_ok(Kin, Nout, rows_per_slab, Kin, Nout, (int64_t)rows_per_slab * Kin, (int64_t)rows_per_slab * Nout)),
                 "op_weight_grad_bf16: variants 2 / 3 need whole 64-row K tiles (variant 3: a zero row behind dy16 instead), at most one extra K tile "
                 "per slab, Nout %% 256 == 0 and at least 192 rows per slab");
    GemmShadows x;
    x.transA = true; x.A16 = x16; x.B16p = dy16; x.force_kernel = sw ? 2 : variant;
    if (sw) {
        x.kextra = u.kextra;
        x.validK = u.validK;
        x.b_zero_row = variant == 3;
    } else {
        x.validK = rows == (int64_t)rows_per_slab * nslabs ? 0 : rows;
    }
    return launch_gemm_bf16_x(nullptr, nullptr, Kin, (int64_t)rows_per_slab * Kin, nullptr, Nout, (int64_t)rows_per_slab * Nout, slabs, Nout,
                              (int64_t)Kin * Nout, nullptr, nullptr, Kin, Nout, rows_per_slab, nslabs, 0, x, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_layer_norm(const float* x, float* y, const float* gamma, const float* beta, int64_t rows,
                       int32_t C, float eps, int32_t act, void* stream) {
    return launch_layer_norm(nullptr, x, y, gamma, beta, rows, C, eps, act, reinterpret_cast<hipStream_t>(stream));
}
int64_t w2v2_conv0_ws_floats(int32_t B, int64_t L, int32_t K, int32_t stride, int32_t C) {
    return conv0_ws_floats(B, L, K, stride, C);
}
int w2v2_op_conv0(const float* wave, const float* kernel, const float* bias, const float* gamma,
                  const float* beta, float* out, float* ws, int32_t B, int64_t L, int32_t K, int32_t stride,
                  int32_t C, float eps, int32_t norm_mode, int32_t act, void* stream) {
    return launch_conv0(nullptr, wave, kernel, bias, gamma, beta, out, ws, B, L, K, stride, C, eps, norm_mode, act,
                        reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_weight_norm_regroup(const float* wv, const float* wg, float* out, int32_t K, int32_t cg,
                                int32_t H, int32_t groups, void* stream) {
    return launch_weight_norm_regroup(nullptr, wv, wg, out, K, cg, H, groups, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_pos_conv(const float* x, const float* wg, const float* bias, const int32_t* frame_len, float* y,
                     int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, int32_t act, void* stream) {
    return launch_pos_conv(nullptr, x, wg, bias, frame_len, y, B, T, H, K, groups, act, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_attention(const float* qkv, const int32_t* frame_len, float* ctx, int32_t B, int32_t T,
                      int32_t H, int32_t num_heads, void* stream) {
    return launch_attention(nullptr, qkv, frame_len, ctx, B, T, H, num_heads, reinterpret_cast<hipStream_t>(stream));
}
}  // extern "C"
namespace {
// The tile table of a packed attention op -- one entry per `rows` queries of an utterance, utterances back to back as cu_frames
// cuts them -- staged on the device, handed to `launch` with an AttnIO that carries it, and freed.
template <class F>
int with_attention_tiles(const char* who, int32_t n, const int32_t* cu_frames, int rows, hipStream_t s, F&& launch) {
    W2V2_REQUIRE(n >= 1 && cu_frames[0] == 0, "%s: need n >= 1 utterances and cu_frames[0] == 0", who);
    std::vector<SegTile> tiles;
    AttnIO io;
    for (int i = 0; i < n; ++i) {
        const int nf = cu_frames[i + 1] - cu_frames[i];
        W2V2_REQUIRE(nf >= 1, "%s: utterance %d has %d frames (need at least one)", who, i, nf);
        for (int t0 = 0; t0 < nf; t0 += rows) tiles.push_back(SegTile{cu_frames[i], nf, t0, 0});
        io.sum_nf2 += (double)nf * (double)nf;
    }
    SegTile* dt = nullptr;
    W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dt), tiles.size() * sizeof(SegTile)));
    int e = hipMemcpyAsync(dt, tiles.data(), tiles.size() * sizeof(SegTile), hipMemcpyHostToDevice, s) == hipSuccess &&
                    hipStreamSynchronize(s) == hipSuccess ? W2V2_OK : W2V2_EHIP;
    if (e) set_error("%s: staging the tile table failed", who);
    io.tiles = dt; io.ntiles = (int)tiles.size(); io.frames = cu_frames[n];
    if (!e) e = launch(io);
    (void)hipStreamSynchronize(s);
    (void)hipFree(dt);
    return e;
}
}  // namespace
extern "C" {
int w2v2_op_attention_packed(const float* qkv, int32_t n, const int32_t* cu_frames, float* ctx, uint16_t* planes, int64_t plane_stride,
                             int32_t* range_flag, int32_t H, int32_t heads, void* stream) {
    W2V2_REQUIRE(qkv && cu_frames && (ctx || planes), "op_attention_packed: null operand");
    W2V2_REQUIRE(n >= 1 && cu_frames[0] == 0, "op_attention_packed: need n >= 1 utterances and cu_frames[0] == 0");
    W2V2_REQUIRE(heads > 0 && H % heads == 0, "op_attention_packed: bad sizes H=%d heads=%d", H, heads);
    const int mode = gemm_get_precision();
    W2V2_REQUIRE(mode != W2V2_PRECISION_BF16, "op_attention_packed: precision mode bf16 is not supported (fp32, bf16x3, f16x2)");
    W2V2_REQUIRE(!planes || mode >= W2V2_PRECISION_BF16X3, "op_attention_packed: planes are written in precision modes bf16x3 / f16x2 only");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the split kernel writes the planes itself; the fp32 segment kernel needs ctx, and (modes 2 / 3) the planes are split off its
    // output, as the packed forward does
    const AttnRoute r = attention_route(attention_problem(AP_INFER, mode, 1, cu_frames[n], H, heads, true, ctx != nullptr, false, false,
                                                          ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(ctx)) & 15) == 0));
    W2V2_REQUIRE(r.family == AF_SPLIT || ctx, "op_attention_packed: this mode and head size run the fp32 kernel, which needs ctx");
    W2V2_REQUIRE(!r.refusal, attention_refusal_text(r), r.dh);
    const int fmt = mode == W2V2_PRECISION_F16X2 ? PF_F16X2 : PF_BF16X3;
    PlaneOut pl;
    pl.p = planes; pl.plane = plane_stride; pl.fmt = fmt; pl.range_flag = range_flag;
    return with_attention_tiles("op_attention_packed", n, cu_frames, r.rows, s, [&](AttnIO& io) {
        io.qkv = qkv; io.ctx = ctx;
        if (r.family == AF_SPLIT) io.planes = &pl;
        int e = launch_attention_routed(nullptr, r, io, s);
        if (!e && r.family != AF_SPLIT && planes) e = launch_split_planes(ctx, planes, plane_stride, io.frames * H, fmt, range_flag, s);
        return e;
    });
}
int w2v2_op_attention_packed_bf16(const float* qkv, const uint16_t* qkv16, int32_t n, const int32_t* cu_frames, float* ctx, uint16_t* ctx16,
                                  int32_t H, int32_t heads, void* stream) {
    W2V2_REQUIRE((qkv || qkv16) && cu_frames && (ctx || ctx16), "op_attention_packed_bf16: null operand");
    W2V2_REQUIRE(n >= 1 && cu_frames[0] == 0, "op_attention_packed_bf16: need n >= 1 utterances and cu_frames[0] == 0");
    W2V2_REQUIRE(heads > 0 && H % heads == 0, "op_attention_packed_bf16: bad sizes H=%d heads=%d (head size 64)", H, heads);
    // (whatever w2v2_op_set_precision says: this op is mode 1's route)
    const AttnRoute r = attention_route(attention_problem(AP_INFER, W2V2_PRECISION_BF16, 1, cu_frames[n], H, heads, true, ctx != nullptr, ctx16 != nullptr));
    W2V2_REQUIRE(r.family == AF_BF16, "op_attention_packed_bf16: bad sizes H=%d heads=%d (head size 64)", H, heads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return with_attention_tiles("op_attention_packed_bf16", n, cu_frames, r.rows, s, [&](AttnIO& io) {
        io.qkv = qkv; io.qkv16 = qkv16; io.ctx = ctx; io.ctx16 = ctx16;
        return launch_attention_routed(nullptr, r, io, s);
    });
}
int w2v2_op_pos_conv_packed_bf16(const float* x, const uint16_t* w16, const float* bias, int32_t n, const int32_t* cu_frames, float* y, int32_t H,
                                 int32_t K, int32_t groups, int32_t act, void* stream) {
    W2V2_REQUIRE(x && w16 && cu_frames && y, "op_pos_conv_packed_bf16: null operand");
    W2V2_REQUIRE(n >= 1 && cu_frames[0] == 0, "op_pos_conv_packed_bf16: need n >= 1 utterances and cu_frames[0] == 0");
    W2V2_REQUIRE(act >= 0 && act <= 2, "op_pos_conv_packed_bf16: bad activation %d", act);
    std::vector<PackSeg> segs((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int nf = cu_frames[i + 1] - cu_frames[i];
        W2V2_REQUIRE(nf >= 1, "op_pos_conv_packed_bf16: utterance %d has %d frames (need at least one)", i, nf);
        segs[i] = PackSeg{0, 0, 0, cu_frames[i], nf, cu_frames[i], 0};
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PackSeg* ds = nullptr;
    W2V2_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ds), segs.size() * sizeof(PackSeg)));
    int e = hipMemcpyAsync(ds, segs.data(), segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice, s) == hipSuccess &&
                    hipStreamSynchronize(s) == hipSuccess ? W2V2_OK : W2V2_EHIP;
    if (e) set_error("op_pos_conv_packed_bf16: staging the utterance table failed");
    if (!e) e = launch_pos_conv_bf16_packed(nullptr, x, w16, bias, y, ds, n, cu_frames[n], H, K, groups, act, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(ds);
    return e;
}
int w2v2_op_frame_lengths(const int32_t* mask, int32_t* frame_len, int32_t B, int64_t L,
                          const int32_t* kernal_sizes, const int32_t* strides, int32_t num_layers, void* stream) {
    return launch_frame_lengths(nullptr, mask, frame_len, B, L, kernal_sizes, strides, num_layers,
                                reinterpret_cast<hipStream_t>(stream));
}
// ---- op-level entry points of the training kernels (train.h): the tests drive them one kernel at a time ----
int64_t w2v2_ln_bwd_ws_floats(int64_t rows, int32_t C) { return ln_bwd_ws_floats(rows, C); }
int w2v2_op_layer_norm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma,
                           float* dbeta, int64_t rows, int32_t C, float eps, float* ws, void* stream) {
    return launch_ln_bwd(x, gamma, dy, dx, dgamma, dbeta, rows, C, eps, ws, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_attention_train(const float* qkv, const int32_t* frame_len, float* ctx, float* lse, int32_t B, int32_t T,
                            int32_t H, int32_t heads, float p, uint64_t seed, uint32_t stream_id, void* stream) {
    AttnTrain tr{p, seed, stream_id, lse};
    return launch_attention_train(nullptr, qkv, frame_len, ctx, B, T, H, heads, tr, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_attention_bwd(const float* qkv, const int32_t* frame_len, const float* ctx, const float* lse,
                          const float* dctx, float* dqkv, float* dvec_ws, int32_t B, int32_t T, int32_t H,
                          int32_t heads, float p, uint64_t seed, uint32_t stream_id, void* stream) {
    AttnTrain tr{p, seed, stream_id, const_cast<float*>(lse)};
    return launch_attention_bwd(nullptr, qkv, frame_len, ctx, dctx, dqkv, dvec_ws, B, T, H, heads, tr,
                                reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_layer_norm_dropout(const float* x, const float* residual, float* t1, float* y, uint16_t* y16, const float* gamma, const float* beta,
                               int64_t rows, int32_t C, float eps, float p, uint64_t seed, uint32_t stream_id, void* stream) {
    return launch_layer_norm_drop(nullptr, x, residual, t1, y, y16, gamma, beta, rows, C, eps, p, seed, stream_id, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_dropout(const float* x, const float* residual, float* y, int64_t n, int32_t act, float p,
                    uint64_t seed, uint32_t stream_id, void* stream) {
    return launch_dropout_fwd(x, residual, y, n, act, p, seed, stream_id, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_pos_conv_ex(const float* x, const float* wg, const float* bias, const int32_t* frame_len, float* y, float* pre_act,
                        int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, int32_t act, int32_t pad_left, int32_t add_residual,
                        void* stream) {
    return launch_pos_conv_ex(nullptr, x, wg, bias, frame_len, y, pre_act, B, T, H, K, groups, act, pad_left, add_residual,
                              reinterpret_cast<hipStream_t>(stream));
}
int64_t w2v2_op_pos_conv_bf16_pack_elems(int32_t B, int32_t T, int32_t H, int32_t K) { return pos_conv_bf16_pack_elems(B, T, H, K); }
int w2v2_op_pos_conv_weight_shadow(const float* wg, uint16_t* w16, int32_t K, int32_t cg, int32_t groups, void* stream) {
    return launch_pos_conv_weight_shadow(wg, w16, K, cg, groups, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_pos_conv_bf16(const float* x, const uint16_t* w16, const float* bias, const int32_t* frame_len, float* y, float* pre_act,
                          uint16_t* pack16, float* xz_ws, int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, int32_t act,
                          int32_t pad_left, int32_t add_residual, void* stream) {
    return launch_pos_conv_bf16(nullptr, x, w16, bias, frame_len, y, pre_act, pack16, xz_ws, B, T, H, K, groups, act, pad_left, add_residual,
                                reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_pos_conv_flip_regroup(const float* wg, float* wg_t, int32_t K, int32_t cg, int32_t groups, void* stream) {
    return launch_pos_conv_flip_regroup(wg, wg_t, K, cg, groups, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_pos_conv_dw(const float* xz, const float* dc, float* dwg, int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups,
                        void* stream) {
    return launch_pos_conv_dw(nullptr, xz, dc, dwg, nullptr, B, T, H, K, groups, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_pos_conv_dw_bf16_ws_floats(int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, int64_t* sizes4, int32_t* slabs_S) {
    W2V2_REQUIRE(sizes4 && B > 0 && T > 0 && K > 0 && groups > 0 && H > 0 && H % groups == 0, "pos_conv_dw_bf16_ws_floats: bad argument");
    int S = 0;
    pos_conv_dw_bf16_ws_floats(B, T, H, K, groups, sizes4, &S);
    if (slabs_S) *slabs_S = S;
    return W2V2_OK;
}
int w2v2_op_pos_conv_dw_bf16(const float* xz, const float* dc, float* dwg, float* pack32, float* slabs, float* red_ws, float* dc_pad,
                             int32_t B, int32_t T, int32_t H, int32_t K, int32_t groups, void* stream) {
    return launch_pos_conv_dw_bf16(nullptr, xz, dc, dwg, pack32, slabs, red_ws, B, T, H, K, groups, reinterpret_cast<hipStream_t>(stream), dc_pad);
}
int w2v2_op_weight_norm_bwd(const float* weight_v, const float* weight_g, const float* dwg, float* dweight_v, float* dweight_g, int32_t K,
                            int32_t cg, int32_t H, int32_t groups, void* stream) {
    return launch_weight_norm_bwd(weight_v, weight_g, dwg, dweight_v, dweight_g, K, cg, H, groups, reinterpret_cast<hipStream_t>(stream));
}
int w2v2_op_grad_norm(const float* g, int64_t n, float max_norm, int32_t skip_nonfinite, w2v2_opt_stats* stats_out, void* stream) {
    W2V2_REQUIRE(g && stats_out && n > 0 && n <= ((int64_t)OPT_CHUNK << 28), "op_grad_norm: bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nchunks = (int)((n + OPT_CHUNK - 1) / OPT_CHUNK);
    void* ws = nullptr;
    W2V2_HIP_CHECK(hipMalloc(&ws, (size_t)nchunks * (sizeof(double) + sizeof(int32_t))));
    int e = W2V2_OK;
    if (hipMemsetAsync(stats_out, 0, sizeof(w2v2_opt_stats), s) != hipSuccess) {
        set_error("op_grad_norm: cannot clear the record");
        e = W2V2_EHIP;
    }
    if (!e)
        e = launch_grad_norm(nullptr, nchunks, g, n, reinterpret_cast<double*>(ws), reinterpret_cast<int32_t*>(reinterpret_cast<double*>(ws) + nchunks),
                             max_norm, skip_nonfinite ? 1 : 0, stats_out, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(ws);
    return e;
}

}  // extern "C"
