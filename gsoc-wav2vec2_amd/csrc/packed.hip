// Glue of the packed variable-length forward (w2v2_forward_packed, w2v2_api.hip): the caller's utterances, back to back,
// into the aligned stream the forward runs on, and the utterances' frames of the stream's output back to the caller's rows.
// Layout and the three stages that see utterance boundaries: DESIGN.md section 10.
#include <algorithm>

#include "common.h"

namespace w2v2 {
namespace {

// stream sample p: its utterance's sample, or zero in the gap behind the utterance
__global__ __launch_bounds__(256) void pack_scatter_kernel(const float* __restrict__ src, float* __restrict__ stream, int64_t L,
                                                           const PackSeg* __restrict__ segs, int nseg) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < L; p += (int64_t)gridDim.x * 256) {
        const PackSeg sg = segs[pack_seg_of_sample(segs, nseg, p)];
        const int64_t j = p - sg.s0;
        stream[p] = j < sg.len ? src[sg.src0 + j] : 0.f;
    }
}

// one block per output row: the row's utterance by its first output row, then a copy of `width` floats
__global__ __launch_bounds__(256) void pack_gather_kernel(const float* __restrict__ rows, float* __restrict__ out, int width,
                                                          const PackSeg* __restrict__ segs, int nseg) {
    const int64_t r = blockIdx.x;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].out0 <= r) lo = mid; else hi = mid - 1;
    }
    const PackSeg sg = segs[lo];
    const float* __restrict__ src = rows + (sg.f0 + (r - sg.out0)) * (int64_t)width;
    float* __restrict__ dst = out + r * (int64_t)width;
    for (int c = threadIdx.x; c < width; c += 256) dst[c] = src[c];
}

}  // namespace

int launch_pack_scatter(const float* src, float* stream, int64_t L, const PackSeg* segs, int nseg, hipStream_t s) {
    W2V2_REQUIRE(src && stream && segs && nseg > 0 && L > 0, "pack_scatter: bad argument");
    const int64_t blocks = std::min<int64_t>((L + 255) / 256, 65536);
    W2V2_LAUNCH(pack_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, stream, L, segs, nseg);
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

}  // namespace w2v2
