// Glue of the packed variable-length forward (w2v2_forward_packed, w2v2_forward_windows; forward.hip): the caller's utterances
// -- back to back, or windows anywhere in one recording -- into the aligned stream the forward runs on, and the kept frames of
// the stream's output back to the caller's rows.  Layout and the three stages that see utterance boundaries: DESIGN.md
// section 10; windows and their normalisation: section 14.
#include <algorithm>

#include "common.h"

namespace w2v2 {
namespace {

// stream sample p: its utterance's sample, or zero in the gap behind the utterance.  With `stats` (mean and sqrt(var + eps) per
// utterance, fp64) the sample is normalised as it is written: the quotient in fp64, rounded once to fp32.
__global__ __launch_bounds__(256) void pack_scatter_kernel(const float* __restrict__ src, float* __restrict__ stream, int64_t L,
                                                           const PackSeg* __restrict__ segs, int nseg,
                                                           const double* __restrict__ stats) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < L; p += (int64_t)gridDim.x * 256) {
        const int i = pack_seg_of_sample(segs, nseg, p);
        const PackSeg sg = segs[i];
        const int64_t j = p - sg.s0;
        float v = 0.f;
        if (j < sg.len) {
            v = src[sg.src0 + j];
            if (stats) v = (float)(((double)v - stats[2 * i]) / stats[2 * i + 1]);
        }
        stream[p] = v;
    }
}

// one block per utterance: (mean, sqrt(population variance + eps)) of its samples in fp64.  Two passes (the mean, then the
// squared deviations from it); each thread adds its samples in index order and the 256 partial sums fold in a fixed tree, so the
// result does not depend on the launch or on the other utterances.
__global__ __launch_bounds__(256) void pack_stats_kernel(const float* __restrict__ src, const PackSeg* __restrict__ segs,
                                                         double eps, double* __restrict__ stats) {
    __shared__ double red[256];
    const PackSeg sg = segs[blockIdx.x];
    const float* __restrict__ x = src + sg.src0;
    const int tid = threadIdx.x;
    double mean = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double acc = 0.0;
        for (int64_t j = tid; j < sg.len; j += 256) {
            const double d = (double)x[j] - mean;
            acc += pass ? d * d : d;
        }
        red[tid] = acc;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) red[tid] += red[tid + off];
            __syncthreads();
        }
        const double r = red[0] / (double)sg.len;
        __syncthreads();
        if (pass == 0) mean = r;
        else if (tid == 0) {
            stats[2 * blockIdx.x] = mean;
            stats[2 * blockIdx.x + 1] = sqrt(r + eps);
        }
    }
}

// one block per output row: the row's utterance by its first output row, then a copy of `width` floats from the kept rows
// (those from local frame keep0 on; the packed forward keeps every frame, keep0 = 0)
__global__ __launch_bounds__(256) void pack_gather_kernel(const float* __restrict__ rows, float* __restrict__ out, int width,
                                                          const PackSeg* __restrict__ segs, int nseg) {
    const int64_t r = blockIdx.x;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].out0 <= r) lo = mid; else hi = mid - 1;
    }
    const PackSeg sg = segs[lo];
    const float* __restrict__ src = rows + (sg.f0 + sg.keep0 + (r - sg.out0)) * (int64_t)width;
    float* __restrict__ dst = out + r * (int64_t)width;
    for (int c = threadIdx.x; c < width; c += 256) dst[c] = src[c];
}

// one block per utterance: the rows behind it that no utterance owns, in fp32, in every plane and in the bf16 shadow
__global__ __launch_bounds__(256) void pack_zero_gaps_kernel(float* __restrict__ x, PlaneOut pl, int np, int64_t frames, int width,
                                                             const PackSeg* __restrict__ segs, int nseg, uint16_t* __restrict__ x16) {
    const int i = blockIdx.x;
    const int64_t r0 = (int64_t)segs[i].f0 + segs[i].nf, r1 = min(i + 1 < nseg ? (int64_t)segs[i + 1].f0 : frames, frames);
    const int64_t n = (r1 > r0 ? r1 - r0 : 0) * width, e0 = r0 * width;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        if (x) x[e0 + e] = 0.f;
        if (x16) x16[e0 + e] = 0;
        for (int p = 0; p < np; ++p) pl.p[p * pl.plane + e0 + e] = 0;
    }
}

}  // namespace

int launch_pack_scatter(const float* src, float* stream, int64_t L, const PackSeg* segs, int nseg, hipStream_t s,
                        const double* stats) {
    W2V2_REQUIRE(src && stream && segs && nseg > 0 && L > 0, "pack_scatter: bad argument");
    const int64_t blocks = std::min<int64_t>((L + 255) / 256, 65536);
    W2V2_LAUNCH(pack_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, stream, L, segs, nseg, stats);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

int launch_pack_stats(const float* src, const PackSeg* segs, int nseg, double eps, double* stats, hipStream_t s) {
    W2V2_REQUIRE(src && segs && stats && nseg > 0, "pack_stats: bad argument");
    W2V2_LAUNCH(pack_stats_kernel, dim3((unsigned)nseg), dim3(256), 0, s, src, segs, eps, stats);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

int launch_pack_gather(const float* stream_rows, float* out, int64_t out_rows, int width, const PackSeg* segs, int nseg,
                       hipStream_t s) {
    W2V2_REQUIRE(stream_rows && out && segs && nseg > 0 && out_rows > 0 && out_rows < INT32_MAX && width > 0,
                 "pack_gather: bad argument");
    W2V2_LAUNCH(pack_gather_kernel, dim3((unsigned)out_rows), dim3(256), 0, s, stream_rows, out, width, segs, nseg);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

int launch_pack_zero_gaps(float* x, const PlaneOut* pl, int64_t frames, int width, const PackSeg* segs, int nseg, hipStream_t s,
                          uint16_t* x16) {
    const PlaneOut p = pl ? *pl : PlaneOut{};
    W2V2_REQUIRE((x || p.p || x16) && segs && nseg > 0 && frames > 0 && width > 0 && (!p.p || p.plane >= frames * width),
                 "pack_zero_gaps: bad argument");
    W2V2_LAUNCH(pack_zero_gaps_kernel, dim3((unsigned)nseg), dim3(256), 0, s, x, p, p.p ? plane_count(p.fmt) : 0, frames, width, segs, nseg, x16);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
