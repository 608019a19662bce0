// Pause cuts of CTC logits (w2v2_ctc_pause_cuts): where a long recording's stitched logits can be cut into
// utterance-sized pieces for the beam search and the aligner.
//
// Definition (tests/longform_reference.py is the same in numpy).  For the rows x_t of one utterance, t in [0, T):
//   a_t     = argmax of x_t, the lowest index on ties; -1 for a row that holds a NaN
//   quiet_t = a_t == blank and x_t[blank] - max_{v != blank} x_t[v] >= margin   (one fp32 subtraction; V == 1: quiet)
//   a pause = a maximal run [a, b) of quiet frames with b - a >= min_pause, a > 0 and b < T; with delim >= 0 only if the last frame
//             before a with a_t != blank exists and has a_t == delim
//   its cut = a + (b - a) / 2
//
// Structure.  cuts_frame_kernel: one wave per frame (as beam_lse_kernel) writes a_t and quiet_t as one int32 code.  The rest works
// on the codes in chunks of CUTS_CHUNK frames, one block each, so that one recording of 2^24 frames spreads over the device.  A
// pause is found at its END, the first frame b that is not quiet: what it needs from the frames before b is the length of the
// quiet run that ends at b - 1 and the last label that is not the blank (the frames of the run are blanks, so "before a" and
// "before b" name the same frame).  Both are associative carries:
//   phase 0  every chunk's summary (Carry of its frames)                            cuts_chunk_kernel<0>
//   scan     exclusive scan of the summaries per utterance, one block each          cuts_carry_kernel
//   phase 1  every chunk's count of pauses, given the carry that enters it          cuts_chunk_kernel<1>
//   scan     exclusive prefix sum of the counts per utterance, and the total        cuts_offset_kernel
//   phase 2  the pauses again, each stored at its rank                              cuts_chunk_kernel<2>
// Every output element is written by exactly one thread with a plain store and the scans fold in a fixed order: no atomics, and a
// repeated call gives the same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace w2v2 {
namespace {

constexpr int CUTS_NT = 256;
constexpr int CUTS_PER_THREAD = W2V2_CUTS_CHUNK / CUTS_NT;
static_assert(CUTS_PER_THREAD * CUTS_NT == W2V2_CUTS_CHUNK, "segment.hip: the chunk is a whole number of frames per thread");
constexpr int CODE_QUIET = 1 << 30;        // code = (a_t + 1) | (quiet_t ? CODE_QUIET : 0)
constexpr int LABEL_NONE = -2;             // no frame with a_t != blank yet (a_t itself is >= -1)

struct CutSeg {
    int64_t row0;      // first logits row
    int64_t code0;     // first code
    int64_t chunk0;    // first chunk
    int32_t T, pad;
};

// what the frames so far hand to the frame after them
struct Carry {
    int run;       // quiet frames at the end
    int allq;      // every frame is quiet
    int label;     // the last a_t != blank, or LABEL_NONE
};

struct CarryOp {
    __device__ __forceinline__ Carry operator()(const Carry& l, const Carry& r) const {
        return Carry{r.allq ? l.run + r.run : r.run, l.allq & r.allq, r.label != LABEL_NONE ? r.label : l.label};
    }
};
struct AddOp {
    __device__ __forceinline__ int operator()(int l, int r) const { return l + r; }
};

struct CutArgs {
    const float* logits;
    const CutSeg* segs;
    int32_t* codes;
    Carry* summary;        // per chunk: the chunk's frames
    Carry* carry_in;       // per chunk: everything before it in its utterance
    int32_t* counts;       // per chunk: pauses that end in it
    int32_t* offsets;      // per chunk: pauses that end before it in its utterance
    int32_t* cut;
    int32_t* pause;
    int32_t* count;
    float margin;
    int V, blank, delim, min_pause, max_cuts;
};

// exclusive scan over the block's 256 values in thread order (Hillis-Steele in LDS); *total: the fold of all of them
template <class T, class Op>
__device__ __forceinline__ T block_scan_excl(T v, T ident, T* lds, Op op, T* total) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < CUTS_NT; off <<= 1) {
        const T x = tid >= off ? op(lds[tid - off], lds[tid]) : lds[tid];
        __syncthreads();
        lds[tid] = x;
        __syncthreads();
    }
    *total = lds[CUTS_NT - 1];
    const T excl = tid ? lds[tid - 1] : ident;
    __syncthreads();
    return excl;
}

__global__ __launch_bounds__(256) void cuts_frame_kernel(CutArgs a) {
    const CutSeg sg = a.segs[blockIdx.y];
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= sg.T) return;
    const int lane = threadIdx.x & 63;
    const float* __restrict__ r = a.logits + (sg.row0 + t) * a.V;
    float best = -INFINITY, other = -INFINITY;      // the lane's maximum and its maximum over v != blank
    int arg = INT32_MAX, nan = 0;
    for (int v = lane; v < a.V; v += 64) {
        const float x = r[v];
        nan |= x != x;
        if (arg == INT32_MAX || x > best) {
            best = x;
            arg = v;
        }
        if (v != a.blank) other = fmaxf(other, x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float b2 = __shfl_xor(best, off, 64);
        const int a2 = __shfl_xor(arg, off, 64);
        if (b2 > best || (b2 == best && a2 < arg) || arg == INT32_MAX) {
            best = b2;
            arg = a2;
        }
        other = fmaxf(other, __shfl_xor(other, off, 64));
        nan |= __shfl_xor(nan, off, 64);
    }
    if (lane == 0) {
        int code = 0;
        if (!nan) {
            const bool quiet = arg == a.blank && (a.V == 1 || r[a.blank] - other >= a.margin);
            code = (arg + 1) | (quiet ? CODE_QUIET : 0);
        }
        a.codes[sg.code0 + t] = code;
    }
}

template <int PHASE>
__global__ __launch_bounds__(CUTS_NT) void cuts_chunk_kernel(CutArgs a) {
    __shared__ Carry lds[CUTS_NT];
    __shared__ int ldi[CUTS_NT];
    const CutSeg sg = a.segs[blockIdx.y];
    const int64_t f0 = (int64_t)blockIdx.x * W2V2_CUTS_CHUNK;
    if (f0 >= sg.T) return;                                   // (uniform over the block)
    const int tid = threadIdx.x;
    const int64_t chunk = sg.chunk0 + blockIdx.x;
    const int t0 = (int)f0 + tid * CUTS_PER_THREAD;
    int code[CUTS_PER_THREAD];
    Carry mine{0, 1, LABEL_NONE};
#pragma unroll
    for (int j = 0; j < CUTS_PER_THREAD; ++j) {
        code[j] = -1;                                         // past the end
        if (t0 + j < sg.T) {
            code[j] = a.codes[sg.code0 + t0 + j];
            const int at = (code[j] & ~CODE_QUIET) - 1;
            const Carry f{(code[j] & CODE_QUIET) ? 1 : 0, (code[j] & CODE_QUIET) ? 1 : 0, at != a.blank ? at : LABEL_NONE};
            mine = CarryOp()(mine, f);
        }
    }
    Carry total;
    const Carry before = block_scan_excl(mine, Carry{0, 1, LABEL_NONE}, lds, CarryOp(), &total);
    if (PHASE == 0) {
        if (tid == 0) a.summary[chunk] = total;
        return;
    }
    // the thread's frames again, from the state that enters them
    const Carry in = CarryOp()(a.carry_in[chunk], before);
    int run = in.run, label = in.label, found = 0;
    int cut[CUTS_PER_THREAD], len[CUTS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < CUTS_PER_THREAD; ++j) {
        if (code[j] < 0) break;
        if (code[j] & CODE_QUIET) {
            ++run;
            continue;
        }
        const int t = t0 + j;
        if (run >= a.min_pause && t - run > 0 && (a.delim < 0 || label == a.delim)) {
            cut[found] = t - run + run / 2;
            len[found] = run;
            ++found;
        }
        run = 0;
        const int at = (code[j] & ~CODE_QUIET) - 1;
        if (at != a.blank) label = at;
    }
    int sum;
    const int rank0 = block_scan_excl(found, 0, ldi, AddOp(), &sum);
    if (PHASE == 1) {
        if (tid == 0) a.counts[chunk] = sum;
        return;
    }
    const int base = a.offsets[chunk] + rank0;
    for (int k = 0; k < found; ++k)
        if (base + k < a.max_cuts) {
            a.cut[(int64_t)blockIdx.y * a.max_cuts + base + k] = cut[k];
            a.pause[(int64_t)blockIdx.y * a.max_cuts + base + k] = len[k];
        }
}

// one block per utterance: the exclusive scan of its chunks' summaries, 256 chunks at a time in chunk order
__global__ __launch_bounds__(CUTS_NT) void cuts_carry_kernel(CutArgs a) {
    __shared__ Carry lds[CUTS_NT];
    const CutSeg sg = a.segs[blockIdx.x];
    const int nchunk = (sg.T + W2V2_CUTS_CHUNK - 1) / W2V2_CUTS_CHUNK;
    Carry running{0, 1, LABEL_NONE};
    for (int c0 = 0; c0 < nchunk; c0 += CUTS_NT) {
        const int c = c0 + threadIdx.x;
        const Carry v = c < nchunk ? a.summary[sg.chunk0 + c] : Carry{0, 1, LABEL_NONE};
        Carry total;
        const Carry before = block_scan_excl(v, Carry{0, 1, LABEL_NONE}, lds, CarryOp(), &total);
        if (c < nchunk) a.carry_in[sg.chunk0 + c] = CarryOp()(running, before);
        running = CarryOp()(running, total);
    }
}

// one block per utterance: the exclusive prefix sum of its chunks' counts, and the utterance's count
__global__ __launch_bounds__(CUTS_NT) void cuts_offset_kernel(CutArgs a) {
    __shared__ int ldi[CUTS_NT];
    const CutSeg sg = a.segs[blockIdx.x];
    const int nchunk = (sg.T + W2V2_CUTS_CHUNK - 1) / W2V2_CUTS_CHUNK;
    int running = 0;
    for (int c0 = 0; c0 < nchunk; c0 += CUTS_NT) {
        const int c = c0 + threadIdx.x;
        const int v = c < nchunk ? a.counts[sg.chunk0 + c] : 0;
        int total;
        const int before = block_scan_excl(v, 0, ldi, AddOp(), &total);
        if (c < nchunk) a.offsets[sg.chunk0 + c] = running + before;
        running += total;
    }
    if (threadIdx.x == 0) a.count[blockIdx.x] = running;
}

}  // namespace

int launch_ctc_pause_cuts(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank, int delim,
                          float margin, int min_pause, int max_cuts, int32_t* cut, int32_t* pause, int32_t* count, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && cut && pause && count, "ctc_pause_cuts: null argument");
    W2V2_REQUIRE(n >= 1, "ctc_pause_cuts: %d utterances (need at least one)", n);
    W2V2_REQUIRE(V >= 1, "ctc_pause_cuts: vocabulary of %d entries", V);
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_pause_cuts: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(delim >= -1 && delim < V && delim != blank, "ctc_pause_cuts: delimiter %d; -1 (none) or a label of the vocabulary %d that is not the blank", delim, V);
    W2V2_REQUIRE(!std::isnan(margin), "ctc_pause_cuts: margin is NaN");
    W2V2_REQUIRE(min_pause >= 1, "ctc_pause_cuts: min_pause %d (need at least one frame)", min_pause);
    W2V2_REQUIRE(max_cuts >= 1 && (int64_t)n * max_cuts < ((int64_t)1 << 31), "ctc_pause_cuts: max_cuts %d for %d utterances", max_cuts, n);
    std::vector<CutSeg> segs((size_t)n);
    int64_t codes = 0, chunks = 0;
    int Tmax = 0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(frames[i] >= 1, "ctc_pause_cuts: utterance %d has %d frames (need at least one)", i, frames[i]);
        W2V2_REQUIRE(frames[i] <= W2V2_CUTS_MAX_FRAMES, "ctc_pause_cuts: utterance %d has too many frames (%d; at most %d)", i, frames[i],
                     W2V2_CUTS_MAX_FRAMES);
        W2V2_REQUIRE(row0[i] >= 0, "ctc_pause_cuts: utterance %d has a negative offset", i);
        segs[i] = CutSeg{row0[i], codes, chunks, frames[i], 0};
        codes += frames[i];
        chunks += (frames[i] + W2V2_CUTS_CHUNK - 1) / W2V2_CUTS_CHUNK;
        Tmax = std::max(Tmax, (int)frames[i]);
    }
    // workspace: the table | codes (sum T_i) | summary, carry_in (chunks) | counts, offsets (chunks)
    const size_t tab_bytes = up256((size_t)n * sizeof(CutSeg)), code_bytes = up256((size_t)codes * sizeof(int32_t));
    const size_t carry_bytes = up256((size_t)chunks * sizeof(Carry)), int_bytes = up256((size_t)chunks * sizeof(int32_t));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_CUTS, s, tab_bytes + code_bytes + 2 * carry_bytes + 2 * int_bytes, &raw)) return e;
    char* p = static_cast<char*>(raw);
    CutArgs a{};
    a.logits = logits;
    a.segs = reinterpret_cast<const CutSeg*>(p);
    a.codes = reinterpret_cast<int32_t*>(p += tab_bytes);
    a.summary = reinterpret_cast<Carry*>(p += code_bytes);
    a.carry_in = reinterpret_cast<Carry*>(p += carry_bytes);
    a.counts = reinterpret_cast<int32_t*>(p += carry_bytes);
    a.offsets = reinterpret_cast<int32_t*>(p += int_bytes);
    a.cut = cut;
    a.pause = pause;
    a.count = count;
    a.margin = margin;
    a.V = V;
    a.blank = blank;
    a.delim = delim;
    a.min_pause = min_pause;
    a.max_cuts = max_cuts;
    if (int e = staged_upload(SCRATCH_CUTS, s, raw, {{segs.data(), (size_t)n * sizeof(CutSeg), 0}}, (size_t)16 << 10)) return e;
    // (work for the profile: the logits read once by the frame pass; a comparison or two per logit)
    ProfScope ps(nullptr, FAM_CTC, 2.0 * (double)codes * V, 4.0 * (double)codes * V, s);
    // slots behind an utterance's pauses hold -1
    W2V2_HIP_CHECK(hipMemsetAsync(cut, 0xff, (size_t)n * max_cuts * sizeof(int32_t), s));
    W2V2_HIP_CHECK(hipMemsetAsync(pause, 0xff, (size_t)n * max_cuts * sizeof(int32_t), s));
    const dim3 chunk_grid((unsigned)((Tmax + W2V2_CUTS_CHUNK - 1) / W2V2_CUTS_CHUNK), (unsigned)n);
    W2V2_LAUNCH(cuts_frame_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
    W2V2_LAUNCH(cuts_chunk_kernel<0>, chunk_grid, dim3(CUTS_NT), 0, s, a);
    W2V2_LAUNCH(cuts_carry_kernel, dim3((unsigned)n), dim3(CUTS_NT), 0, s, a);
    W2V2_LAUNCH(cuts_chunk_kernel<1>, chunk_grid, dim3(CUTS_NT), 0, s, a);
    W2V2_LAUNCH(cuts_offset_kernel, dim3((unsigned)n), dim3(CUTS_NT), 0, s, a);
    W2V2_LAUNCH(cuts_chunk_kernel<2>, chunk_grid, dim3(CUTS_NT), 0, s, a);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
