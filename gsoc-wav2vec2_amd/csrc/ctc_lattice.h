// The pieces of the CTC lattice that align.hip, align_long.hip, score.hip and beam.hip share: one definition of
// each contract whose bits must agree across those families.  Device pieces are __device__ __forceinline__ functions; every
// __global__ kernel stays in its own file.  NOT here: the Viterbi step and the windowed backtrace of align.hip and
// align_long.hip, and the per-thread label loops of align.hip, align_long.hip and score.hip.  As shared functions they compile to
// another instruction order in the latency-bound sweeps (1.4 % and 1.5 % of align_long.hip's two kernels, 1 % of align.hip's:
// profiles/ctc_lattice.md), so each file keeps its copy; tests/test_align_long_gpu.py pins align_long against align.
#pragma once

#include "common.h"

#include <type_traits>

namespace w2v2 {

constexpr int LATTICE_MAX_THREADS = 1024;    // threads of a sweep block at P = 8
constexpr int LATTICE_CHUNK = 128;           // frames per backtrace window of the aligners
constexpr int LATTICE_WIN_WORDS = 2304;      // >= ((C - 1) / G + 2) ((C - 1) / P + 2) <= 2193 for C = 128, any P

// ---- host: pairs per thread ----
// the fewest pairs per thread with which `pairs` state pairs need at most 256 threads, else 8 (up to 1024 threads)
inline int pairs_per_thread(int64_t pairs) { return pairs <= 256 ? 1 : pairs <= 512 ? 2 : pairs <= 1024 ? 4 : 8; }
// f(std::integral_constant<int, P>) for P in {1, 2, 4, 8}
template <class F>
void dispatch_pairs(int P, F&& f) {
    if (P == 1) f(std::integral_constant<int, 1>());
    else if (P == 2) f(std::integral_constant<int, 2>());
    else if (P == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 8>());
}

// Barrier of a recursion's steps: what must be visible across the block are the LDS exchange entries, so the wave waits for its LDS
// traffic only.  __syncthreads() also drains vmcnt -- the step's fire-and-forget stores to the workspace -- and a store's round
// trip (~1 us) then becomes the step time (the training recursion of ctc.hip once paid exactly that: 0.73 us per step).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The frame log-sum-exp, the body of every *_lse_kernel: blocks of 256 threads, one wave per frame, grid.x covers the frames.
// lse[t] of frame t < T of the utterance whose logits begin at row0: the fp32 max over lane-strided columns and a butterfly, then
// lane-strided fp64 sums of exp(x - max) and a butterfly, then max + log(sum).  One order of operations, so one set of bits,
// whatever else a caller asks for.  Returns the wave's frame t (-1: none) and, in every lane, m = the fp32 maximum of the frame's
// V logits (fmaxf: a NaN logit is ignored; -inf when all are NaN) and, with ARG, a = the lowest column index whose logit equals m
// (V when none compares equal: a frame of NaN only, whose lse is not finite anyway).
template <bool ARG>
__device__ __forceinline__ int frame_lse_body(const float* logits, int V, int64_t row0, int T, double* lse, float& m, int& a) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    m = -INFINITY;
    a = V;
    if (t >= T) return -1;
    const int lane = threadIdx.x & 63;
    const float* __restrict__ r = logits + (row0 + t) * V;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, r[v]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    double acc = 0.0;
    for (int v = lane; v < V; v += 64) acc += exp((double)r[v] - (double)m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) lse[t] = (double)m + log(acc);
    if constexpr (ARG) {
        for (int v = lane; v < V; v += 64) a = min(a, r[v] == m ? v : V);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a = min(a, __shfl_xor(a, off, 64));
    }
    return t;
}
// lse[t] alone (the aligners without a star, the scorer, the beam search, the phrase search)
__device__ __forceinline__ void frame_lse(const float* logits, int V, int64_t row0, int T, double* lse) {
    float m;
    int a;
    frame_lse_body<false>(logits, V, row0, T, lse, m, a);
}
// ... and the frame's maximum (the star emission of the aligners)
__device__ __forceinline__ int frame_lse_max(const float* logits, int V, int64_t row0, int T, double* lse, float& m) {
    int a;
    return frame_lse_body<false>(logits, V, row0, T, lse, m, a);
}
// ... and the frame's top token (the star of the exact scorer and its gradient)
__device__ __forceinline__ int frame_lse_max_arg(const float* logits, int V, int64_t row0, int T, double* lse, float& m, int& a) {
    return frame_lse_body<true>(logits, V, row0, T, lse, m, a);
}

// number of threads of the block for which pred holds (wave ballots, then the waves in order)
__device__ __forceinline__ int block_count(bool pred, int* red) {
    const unsigned long long b = __ballot(pred);
    __syncthreads();                                    // (red may still be read by the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    int c = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) c += red[i];
    return c;
}

// lse of two / three values that are finite or -inf (never NaN, never +inf); -inf when all are
__device__ __forceinline__ double lse2(double a, double b) {
    const double hi = fmax(a, b), lo = fmin(a, b);
    const double r = hi + log(1.0 + exp(lo - hi));
    return hi > -__builtin_inf() ? r : -__builtin_inf();
}
__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double hi = fmax(a, b), lo = fmin(a, b);
    const double m = fmax(hi, c), y = fmin(hi, c);
    const double r = m + log(1.0 + exp(y - m) + exp(lo - m));
    return m > -__builtin_inf() ? r : -__builtin_inf();
}

}  // namespace w2v2
