// Waveform augmentation for fine-tuning (w2v2_fir, w2v2_mix): reverberation as a long FIR convolution with a
// private filter per segment, and additive noise at a gain derived from the two signals' powers.
//
// Definitions (include/w2v2.h; tests/augment_reference.py is the same in numpy).  Segment i is x[0, len), zero outside.
//   w2v2_fir   y[n] = sum_{k < K} h[k] x[n + d - k], n in [0, len): ONE fp32 chain in ascending k from +0.0f, one fmaf per tap, zero
//              pads included.  match_power: g = (float)sqrt(Px / Py) (1 when either is 0), out = g * y; otherwise out = y, g = 1.
//   w2v2_mix   v[n] = noise[(offset + n) mod noise_len]; g = (float)(sqrt(Px / Pv) * scale) (0 when either is 0);
//              out[n] = fmaf(g, v[n], x[n]), and x[n] itself where g == 0.
// Px, Py, Pv are fp64 sums of squares over the segment's len samples in an order fixed by the segment alone (below).
//
// The FIR kernel.  Write n = 32 a + b.  Then Y[a][b] = sum_j X[a][j] T[j][b] with X[a][j] = x[32 a + 31 + d - j] -- a strided,
// overlapping, reversed view of the signal -- and the Toeplitz block T[j][b] = h[j - 31 + b], zero out of range, j in [0, K + 31).
// For a fixed output ascending j is ascending k, and v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain, so every output is
// the chain of the definition whatever block, wave or lane computes it.  A structural zero of T (or a zero pad of x) adds +-0 to an
// accumulator that started from +0 and can therefore never be -0: it leaves the bits unchanged.  The contraction is never split.
//   - a block owns W2V2_FIR_TILE = 8192 consecutive outputs of one segment, counted from the segment's first sample; each of its four
//     waves owns two 32 x 32 tiles (a in 32 row blocks, b in 32 columns) whose accumulators stay in registers over all of j;
//   - j runs in chunks of W2V2_FIR_CHUNK = 2048.  Per chunk the block stages the signal span the tile needs (tile - 32 + chunk
//     samples, zero by SELECTION outside [0, len): no neighbour's sample is read, and a NaN between segments never enters a product)
//     and the chunk's taps with 31 zeros' room on either side.  A chunk whose whole span lies outside the segment is skipped;
//   - lanes that differ in a read the signal 32 words apart, so the staged signal is skewed by one pad word per 32 (word p lies at
//     p + p / 32): the 32 lanes of a ds_read_b32 group then hit 32 different banks.  The taps are read at consecutive words.
// The sums of squares: chunks of 4096 samples counted from the segment's start; thread t of 256 adds samples t, t + 256, ... of its
// chunk in fp64, a tree folds the 256 sums, and one block per segment folds the chunks the same way.  No atomics.
#include <cmath>
#include <vector>

#include "common.h"

namespace w2v2 {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int FIR_NT = 256;
constexpr int FIR_WT = 2;                                              // 32 x 32 tiles per wave
constexpr int FIR_TILE = W2V2_FIR_TILE;
constexpr int FIR_CHUNK = W2V2_FIR_CHUNK;
constexpr int FIR_SPAN = FIR_TILE - 32 + FIR_CHUNK;                    // staged samples per chunk
constexpr int FIR_XS = FIR_SPAN + FIR_SPAN / 32 + 2;                   // ... skewed
constexpr int FIR_HS = FIR_CHUNK + 32;
static_assert(FIR_TILE == (FIR_NT / 64) * FIR_WT * 1024 && FIR_CHUNK % 32 == 0, "a wave owns FIR_WT tiles of 1024 outputs");

constexpr int AUG_NT = 256;
constexpr int AUG_CHUNK = 4096;                                        // samples per block of the element-wise kernels

struct FirSeg {
    int64_t in0, out0, taps0;
    int64_t tile0;             // first block of the segment
    int32_t len, K, d, pad;
};

// a segment of the element-wise kernels: A(n) = a[a0 + n], B(n) = b[b0 + (b_off + n) mod b_period]
struct AugSeg {
    int64_t a0, b0, b_off, b_period, out0;
    int64_t chunk0;            // first chunk of the segment
    double scale;
    int32_t len, pad;
};

template <class S, class F>
__device__ __forceinline__ int seg_of(const S* segs, int nseg, int64_t b, F first) {
    int lo = 0, hi = nseg - 1;                 // the last segment whose first block is not behind b (uniform over the block)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(segs[mid]) <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(FIR_NT) void fir_kernel(const float* __restrict__ in, const float* __restrict__ taps, float* __restrict__ out,
                                                     const FirSeg* __restrict__ segs, int nseg) {
    __shared__ float xs[FIR_XS];
    __shared__ float hs[FIR_HS];
    const int tid = threadIdx.x, lane = tid & 63, bl = lane & 31, half = lane >> 5;
    const int wt0 = (tid >> 6) * FIR_WT;       // the wave's first tile
    const int64_t b = blockIdx.x;
    const FirSeg sg = segs[seg_of(segs, nseg, b, [](const FirSeg& s) { return s.tile0; })];
    const int64_t n0 = (b - sg.tile0) * FIR_TILE;
    const int len = sg.len, K = sg.K;
    const int cnt = (int)min((int64_t)FIR_TILE, (int64_t)len - n0);
    const float* __restrict__ x = in + sg.in0;
    const float* __restrict__ h = taps + sg.taps0;
    const bool active = cnt > wt0 * 1024;      // (wave-uniform) the wave has outputs at all
    const int J = K + 31;

    f32x16 acc[FIR_WT];
#pragma unroll
    for (int t = 0; t < FIR_WT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    for (int j0 = 0; j0 < J; j0 += FIR_CHUNK) {
        const int nblk = min(FIR_CHUNK, (J - j0 + 31) & ~31) >> 5;      // 32-wide steps of j in this chunk
        const int p_lo = FIR_CHUNK - 32 * nblk;                         // staged word p is x[base + p]; words below p_lo are not read
        const int64_t base = n0 + 31 + sg.d - (int64_t)(j0 + FIR_CHUNK - 1);
        if (base + p_lo >= len || base + FIR_SPAN - 1 < 0) continue;    // (block-uniform) every sample of the chunk is a zero pad
        __syncthreads();
        for (int p = p_lo + tid; p < FIR_SPAN; p += FIR_NT) {
            const int64_t g = base + p;
            xs[p + (p >> 5)] = (g >= 0 && g < len) ? x[g] : 0.0f;
        }
        for (int i = tid; i < 32 * nblk + 31; i += FIR_NT) {
            const int k = j0 - 31 + i;
            hs[i] = (k >= 0 && k < K) ? h[k] : 0.0f;
        }
        __syncthreads();
        if (!active) continue;
        // j = j0 + 32 u + 2 s + half.  A: word p = 32 a + (FIR_CHUNK - 1 - (j - j0)) = 32 (a + m) + r with m = FIR_CHUNK / 32 - 1 - u
        // and r = 31 - 2 s - half, at 33 (a + m) + r of the skewed image; B: hs[(j - j0) + b]
        const float* xa = xs + 33 * (32 * wt0 + bl + FIR_CHUNK / 32 - 1) + (1 - half);
        const float* hb = hs + bl + half;
        for (int u = 0; u < nblk; ++u) {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float bv = hb[2 * s];
#pragma unroll
                for (int t = 0; t < FIR_WT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[33 * 32 * t + 30 - 2 * s], bv, acc[t], 0, 0, 0);
            }
            xa -= 33;
            hb += 32;
        }
    }
    if (!active) return;
    float* __restrict__ y = out + sg.out0 + n0;
#pragma unroll
    for (int t = 0; t < FIR_WT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = 32 * (wt0 + t) + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int nl = 32 * a + bl;
            if (nl < cnt) y[nl] = acc[t][r];
        }
}

// fold 256 fp64 values of a block in a fixed tree; the sum is in red[0] afterwards
__device__ __forceinline__ void fold256(double* red) {
    __syncthreads();
    for (int w = AUG_NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
}

// partial[2 c], partial[2 c + 1]: the sums of A^2 and B^2 over chunk c
__global__ __launch_bounds__(AUG_NT) void aug_power_kernel(const float* __restrict__ a, const float* __restrict__ bsig,
                                                           const AugSeg* __restrict__ segs, int nseg, double* __restrict__ partial) {
    __shared__ double red[AUG_NT];
    const int64_t c = blockIdx.x;
    const AugSeg sg = segs[seg_of(segs, nseg, c, [](const AugSeg& s) { return s.chunk0; })];
    const int64_t m0 = (c - sg.chunk0) * AUG_CHUNK;
    const int cnt = (int)min((int64_t)AUG_CHUNK, (int64_t)sg.len - m0);
    const float* __restrict__ pa = a + sg.a0 + m0;
    const float* __restrict__ pb = bsig + sg.b0;
    const int64_t step = AUG_NT % sg.b_period;
    int64_t q = (sg.b_off + m0 + threadIdx.x) % sg.b_period;
    double sa = 0.0, sb = 0.0;
    for (int i = threadIdx.x; i < cnt; i += AUG_NT) {
        const double va = (double)pa[i], vb = (double)pb[q];
        sa += va * va;
        sb += vb * vb;
        q += step;
        if (q >= sg.b_period) q -= sg.b_period;
    }
    red[threadIdx.x] = sa;
    fold256(red);
    if (threadIdx.x == 0) partial[2 * c] = red[0];
    __syncthreads();
    red[threadIdx.x] = sb;
    fold256(red);
    if (threadIdx.x == 0) partial[2 * c + 1] = red[0];
}

// one block per segment: its chunks' sums in index order per thread, the same tree, then the gain.  mix == 0: sqrt(Pa / Pb), 1 when
// either is 0; mix == 1: sqrt(Pa / Pb) scale, 0 when either is 0
__global__ __launch_bounds__(AUG_NT) void aug_gain_kernel(const AugSeg* __restrict__ segs, const double* __restrict__ partial, int mix,
                                                          float* __restrict__ gains, float* __restrict__ gain_out) {
    __shared__ double red[AUG_NT];
    const AugSeg sg = segs[blockIdx.x];
    const int64_t nch = ((int64_t)sg.len + AUG_CHUNK - 1) / AUG_CHUNK;
    const double* __restrict__ p = partial + 2 * sg.chunk0;
    double sa = 0.0, sb = 0.0;
    for (int64_t i = threadIdx.x; i < nch; i += AUG_NT) {
        sa += p[2 * i];
        sb += p[2 * i + 1];
    }
    red[threadIdx.x] = sa;
    fold256(red);
    const double Pa = red[0];
    __syncthreads();
    red[threadIdx.x] = sb;
    fold256(red);
    const double Pb = red[0];
    if (threadIdx.x == 0) {
        float g;
        if (Pa == 0.0 || Pb == 0.0) g = mix ? 0.0f : 1.0f;
        else g = mix ? (float)(sqrt(Pa / Pb) * sg.scale) : (float)sqrt(Pa / Pb);
        gains[blockIdx.x] = g;
        if (gain_out) gain_out[blockIdx.x] = g;
    }
}

// mix == 0: out[n] = g B(n) (B is the unscaled result, in place); mix == 1: out[n] = fmaf(g, B(n), A(n)), A(n) where g == 0
__global__ __launch_bounds__(AUG_NT) void aug_apply_kernel(const float* __restrict__ a, const float* bsig, float* out,
                                                           const AugSeg* __restrict__ segs, int nseg, const float* __restrict__ gains, int mix) {
    const int64_t c = blockIdx.x;
    const int si = seg_of(segs, nseg, c, [](const AugSeg& s) { return s.chunk0; });
    const AugSeg sg = segs[si];
    const float g = gains[si];
    const int64_t m0 = (c - sg.chunk0) * AUG_CHUNK;
    const int cnt = (int)min((int64_t)AUG_CHUNK, (int64_t)sg.len - m0);
    const float* __restrict__ pa = a + sg.a0 + m0;
    const float* pb = bsig + sg.b0;
    float* y = out + sg.out0 + m0;
    const int64_t step = AUG_NT % sg.b_period;
    int64_t q = (sg.b_off + m0 + threadIdx.x) % sg.b_period;
    for (int i = threadIdx.x; i < cnt; i += AUG_NT) {
        const float vb = pb[q];
        if (mix) {
            const float va = pa[i];
            y[i] = g == 0.0f ? va : fmaf(g, vb, va);
        } else {
            y[i] = g * vb;
        }
        q += step;
        if (q >= sg.b_period) q -= sg.b_period;
    }
}

__global__ void aug_ones_kernel(float* g, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = 1.0f;
}

// the workspace of the element-wise part: the table | n gains | 2 * chunks partial sums
struct ElementWs {
    AugSeg* segs;
    float* gains;
    double* partial;
};
size_t element_ws_bytes(int n, int64_t chunks) {
    return up256((size_t)n * sizeof(AugSeg)) + up256((size_t)n * sizeof(float)) + (size_t)chunks * 2 * sizeof(double);
}
ElementWs element_ws(char* p, int n) {
    const size_t seg_bytes = up256((size_t)n * sizeof(AugSeg));
    return ElementWs{reinterpret_cast<AugSeg*>(p), reinterpret_cast<float*>(p + seg_bytes),
                     reinterpret_cast<double*>(p + seg_bytes + up256((size_t)n * sizeof(float)))};
}

// the element-wise part of both calls, the table already on its way: powers -> gains -> apply
int power_gain_apply(const float* a, const float* bsig, float* out, const ElementWs& w, int n, int64_t chunks, int mix, float* gain_dev,
                     hipStream_t s) {
    W2V2_LAUNCH(aug_power_kernel, dim3((unsigned)chunks), dim3(AUG_NT), 0, s, a, bsig, w.segs, n, w.partial);
    W2V2_LAUNCH(aug_gain_kernel, dim3((unsigned)n), dim3(AUG_NT), 0, s, w.segs, w.partial, mix, w.gains, gain_dev);
    W2V2_LAUNCH(aug_apply_kernel, dim3((unsigned)chunks), dim3(AUG_NT), 0, s, a, bsig, out, w.segs, n, w.gains, mix);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace

int launch_fir(const float* in, int n, const int64_t* in0, const int64_t* len, const float* taps, const int64_t* taps0, const int32_t* ntaps,
               const int32_t* delay, float* out, const int64_t* out0, int match_power, float* gain, hipStream_t s) {
    W2V2_REQUIRE(in && in0 && len && taps && taps0 && ntaps && delay && out && out0,
                 "fir: null argument (in_dev, in0_host, len_host, taps_dev, taps0_host, ntaps_host, delay_host, out_dev or out0_host)");
    W2V2_REQUIRE(n >= 1, "fir: n = %d segments (need at least one)", n);
    std::vector<FirSeg> segs((size_t)n);
    std::vector<AugSeg> esegs((size_t)(match_power ? n : 0));
    int64_t tiles = 0, chunks = 0;
    double flops = 0.0, floats = 0.0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(len[i] >= 1 && len[i] < ((int64_t)1 << 31), "fir: len_host[%d] = %lld outside [1, 2^31)", i, (long long)len[i]);
        W2V2_REQUIRE(ntaps[i] >= 1 && ntaps[i] <= W2V2_FIR_MAX_TAPS, "fir: ntaps_host[%d] = %d outside [1, %d]", i, ntaps[i], W2V2_FIR_MAX_TAPS);
        W2V2_REQUIRE(delay[i] >= 0 && delay[i] < ntaps[i], "fir: delay_host[%d] = %d outside [0, ntaps = %d)", i, delay[i], ntaps[i]);
        W2V2_REQUIRE(in0[i] >= 0, "fir: in0_host[%d] = %lld is negative", i, (long long)in0[i]);
        W2V2_REQUIRE(taps0[i] >= 0, "fir: taps0_host[%d] = %lld is negative", i, (long long)taps0[i]);
        W2V2_REQUIRE(out0[i] >= 0, "fir: out0_host[%d] = %lld is negative", i, (long long)out0[i]);
        segs[i] = FirSeg{in0[i], out0[i], taps0[i], tiles, (int32_t)len[i], ntaps[i], delay[i], 0};
        if (match_power) esegs[i] = AugSeg{in0[i], out0[i], 0, len[i], out0[i], chunks, 1.0, (int32_t)len[i], 0};
        tiles += (len[i] + FIR_TILE - 1) / FIR_TILE;
        chunks += (len[i] + AUG_CHUNK - 1) / AUG_CHUNK;
        W2V2_REQUIRE(chunks < ((int64_t)1 << 31), "fir: more than 2^31 - 1 chunks of %d samples", AUG_CHUNK);
        flops += 2.0 * (double)len[i] * ntaps[i];
        floats += 2.0 * (double)len[i] + ntaps[i];
    }
    // workspace: the FIR segments | the element-wise segments, the gains, the partial sums
    const size_t fir_bytes = up256((size_t)n * sizeof(FirSeg));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_AUGMENT, s, fir_bytes + (match_power ? element_ws_bytes(n, chunks) : 0), &raw)) return e;
    if (int e = staged_upload(SCRATCH_AUGMENT, s, raw,
                              {{segs.data(), (size_t)n * sizeof(FirSeg), 0}, {esegs.data(), esegs.size() * sizeof(AugSeg), fir_bytes}},
                              (size_t)16 << 10))
        return e;
    // (work for the profile: one fused multiply-add per tap and output; with match_power x once more, y read twice and written again)
    ProfScope ps(nullptr, FAM_MISC, flops, 4.0 * floats + (match_power ? 16.0 * (floats / 2.0) : 0.0), s);
    W2V2_LAUNCH(fir_kernel, dim3((unsigned)tiles), dim3(FIR_NT), 0, s, in, taps, out, reinterpret_cast<const FirSeg*>(raw), n);
    W2V2_HIP_CHECK(hipGetLastError());
    if (match_power) return power_gain_apply(in, out, out, element_ws(static_cast<char*>(raw) + fir_bytes, n), n, chunks, 0, gain, s);
    if (gain) {
        W2V2_LAUNCH(aug_ones_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gain, n);
        W2V2_HIP_CHECK(hipGetLastError());
    }
    return W2V2_OK;
}

int launch_mix(const float* in, int n, const int64_t* in0, const int64_t* len, const float* noise, const int64_t* noise0,
               const int64_t* noise_len, const int64_t* offset, const double* scale, float* out, const int64_t* out0, float* gain,
               hipStream_t s) {
    W2V2_REQUIRE(in && in0 && len && noise && noise0 && noise_len && offset && scale && out && out0,
                 "mix: null argument (in_dev, in0_host, len_host, noise_dev, noise0_host, noise_len_host, offset_host, scale_host, out_dev or "
                 "out0_host)");
    W2V2_REQUIRE(n >= 1, "mix: n = %d segments (need at least one)", n);
    std::vector<AugSeg> segs((size_t)n);
    int64_t chunks = 0;
    double floats = 0.0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(len[i] >= 1 && len[i] < ((int64_t)1 << 31), "mix: len_host[%d] = %lld outside [1, 2^31)", i, (long long)len[i]);
        W2V2_REQUIRE(noise_len[i] >= 1 && noise_len[i] < ((int64_t)1 << 31), "mix: noise_len_host[%d] = %lld outside [1, 2^31)", i,
                     (long long)noise_len[i]);
        W2V2_REQUIRE(offset[i] >= 0 && offset[i] < noise_len[i], "mix: offset_host[%d] = %lld outside [0, noise_len = %lld)", i,
                     (long long)offset[i], (long long)noise_len[i]);
        W2V2_REQUIRE(std::isfinite(scale[i]) && scale[i] >= 0.0, "mix: scale_host[%d] = %g (need a finite value >= 0)", i, scale[i]);
        W2V2_REQUIRE(in0[i] >= 0, "mix: in0_host[%d] = %lld is negative", i, (long long)in0[i]);
        W2V2_REQUIRE(noise0[i] >= 0, "mix: noise0_host[%d] = %lld is negative", i, (long long)noise0[i]);
        W2V2_REQUIRE(out0[i] >= 0, "mix: out0_host[%d] = %lld is negative", i, (long long)out0[i]);
        segs[i] = AugSeg{in0[i], noise0[i], offset[i], noise_len[i], out0[i], chunks, scale[i], (int32_t)len[i], 0};
        chunks += (len[i] + AUG_CHUNK - 1) / AUG_CHUNK;
        W2V2_REQUIRE(chunks < ((int64_t)1 << 31), "mix: more than 2^31 - 1 chunks of %d samples", AUG_CHUNK);
        floats += (double)len[i];
    }
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_AUGMENT, s, element_ws_bytes(n, chunks), &raw)) return e;
    // (work for the profile: x and the noise read twice, the output written once)
    ProfScope ps(nullptr, FAM_MISC, 6.0 * floats, 20.0 * floats, s);
    if (int e = staged_upload(SCRATCH_AUGMENT, s, raw, {{segs.data(), (size_t)n * sizeof(AugSeg), 0}}, (size_t)16 << 10)) return e;
    return power_gain_apply(in, noise, out, element_ws(static_cast<char*>(raw), n), n, chunks, 1, gain, s);
}

}  // namespace w2v2
