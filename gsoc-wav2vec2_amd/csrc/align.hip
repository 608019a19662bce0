// CTC forced alignment: the single best frame-level path (Viterbi) that spells a given label string, for n utterances at once.
//
// Definition (tests/align_reference.py implements exactly this).  x_t(v) is the fp32 logit widened to fp64; ext is the label
// string with blanks interleaved, S = 2U + 1 states, ext[2k] = blank, ext[2k + 1] = l_k.
//   delta_0(0) = x_0(blank); delta_0(1) = x_0(l_0) if U >= 1; every other state -inf.
//   t >= 1: delta_t(s) = m + x_t(ext[s]), m and the backpointer bp picked in this order, every comparison a strict `>` done as
//   compare and select (no fmax: it treats NaN differently):
//     m = delta_{t-1}(s), bp = 0;
//     if s >= 1 and delta_{t-1}(s-1) > m:                                          m = delta_{t-1}(s-1), bp = 1;
//     if s >= 2, ext[s] != blank, ext[s] != ext[s-2] and delta_{t-1}(s-2) > m:     m = delta_{t-1}(s-2), bp = 2.
//   Ties prefer staying, then advancing by one.  End state: U >= 1: S-1 if delta_{T-1}(S-1) > delta_{T-1}(S-2), else S-2;
//   U = 0: state 0 (all blank).  The path follows the backpointers down to t = 0.
// The recursion runs on raw logits (sum_t lse_t is common to every path); every step is one IEEE fp64 compare-select and add in a
// fixed order, so the decisions are bit-identical to an fp64 numpy loop on every input, ties and NaN included.
// Outputs per frame (sum T_i, back to back): token[t] = ext[s_t]; label_index[t] = k for state 2k+1, -1 for a blank;
// frame_logp[t] = x_t(token[t]) - lse_t as fp32, lse_t the fp64 log-sum-exp of the frame (ctc_lattice.h: frame_lse).  Per
// utterance: score = delta_{T-1}(s_end) - sum_t lse_t (fp64).
// An utterance is feasible only if T >= U + R, R = #{k >= 1: l_k = l_{k-1}}: otherwise score = -inf, token = label_index = -1 and
// frame_logp = NaN.  A label outside [0, V) or equal to the blank (labels are on the device): score = NaN, the same -1 / NaN rows.
//
// The star (w2v2_ctc_align_star; tests/align_star_reference.py): a wildcard label that absorbs whatever is spoken
// where the transcript has a gap.  Its id is V, as if the logits had one more column, with the raw-logit emission
//   xs_t = (double)m_t + (double)star_score,   m_t = the fp32 maximum of the frame's V logits (the blank included; fmaxf, so a NaN
//   logit is ignored: ctc_lattice.h, frame_lse_max), star_score <= 0 an fp32 argument in nats per frame.
// Nothing in the recursion changes: ext[2k + 1] = V is a state like any other, the skip rule and R treat V like any id, the star
// takes at least one frame, and the comparison order, the ties, the end state and T >= U + R stay.  On a star frame token[t] = V,
// label_index[t] = k, frame_logp[t] = (float)(xs_t - lse_t).  score = delta_end - sum_t lse_t as before: with a star it is the
// score of a path, no longer the log-probability of a label string.  A label < 0, > V or equal to the blank: the NaN utterance.
//
// Structure.  lds_barrier, frame_lse and block_count are ctc_lattice.h's; the step and the backtrace below have a copy in
// align_long.hip, which must stay the same operations in the same order.  align_lse_kernel: one wave per frame, lse_t into the
// workspace (align_lse_star_kernel: and xs_t beside it).  align_viterbi_kernel: one block per utterance.
// A thread owns P consecutive state pairs in registers as fp64; per step the only value that crosses threads is the odd state of
// a thread's last pair, through a double-buffered LDS array behind ONE lds_barrier (the step's fire-and-forget backpointer stores
// are not drained).  The P + 1 emissions a step needs are loaded PF steps ahead.  Backpointers: a thread collects its 4P bits of
// G = 8 / P steps in one 32-bit word and stores it (a plain vector store) to the workspace: word (g, tid) of an utterance holds
// steps 1 + gG .. gG + G, i.e. T S / 4 bytes per utterance, rounded up to the block's thread count.  P comes from the largest U
// at launch (pairs_per_thread: 1, 2, 4 up to 1023 labels on 256 threads; 8 beyond, up to 1024 threads: 8191 labels).  After the
// sweep the same block backtracks: the state moves down by at most 2 per step, so the backpointer words of the next C frames lie
// in a window of C frames x C pairs; the block loads that window into LDS, one lane walks it, and the block writes the C frames'
// outputs (token, label index, frame_logp) in parallel.  No atomics: two identical calls give identical bits.
// STAR is a compile-time flag of the sweep kernel; the STAR = false instantiation is the star-free code.  With it a thread keeps a
// bit mask of its pairs that hold the star, xs_t is loaded PF steps ahead like x_t(blank) (one block-uniform fp64), an odd state
// adds xs_t where the mask is set, and a star pair's per-lane logits load reads the blank's column and is discarded, so that no
// address leaves the row.
#include "ctc_lattice.h"

#include <algorithm>
#include <vector>

namespace w2v2 {
namespace {

struct AlignSeg {
    int64_t row0;      // first logits row
    int64_t label0;    // first label
    int64_t out0;      // first output frame
    int64_t bp0;       // first backpointer word
    int32_t T, U;
};

struct AlignArgs {
    const float* logits;
    const int32_t* labels;
    const AlignSeg* segs;
    double* lse;            // (sum T_i), indexed like the outputs
    uint32_t* bp;           // backpointer words
    int32_t* token;
    int32_t* label_index;
    float* frame_logp;
    double* score;
    int V, blank, nt;       // nt: threads per block (= backpointer words per step group)
};

// lse_t of frame t of utterance blockIdx.y: one wave per frame, grid.x covers the longest utterance
__global__ __launch_bounds__(256) void align_lse_kernel(AlignArgs a) {
    const AlignSeg sg = a.segs[blockIdx.y];
    frame_lse(a.logits, a.V, sg.row0, sg.T, a.lse + sg.out0);
}

// ... and xs_t = m_t + star_score into xs, indexed like lse
__global__ __launch_bounds__(256) void align_lse_star_kernel(AlignArgs a, double* xs, float star_score) {
    const AlignSeg sg = a.segs[blockIdx.y];
    float m;
    const int t = frame_lse_max(a.logits, a.V, sg.row0, sg.T, a.lse + sg.out0, m);
    if (t >= 0 && (threadIdx.x & 63) == 0) xs[sg.out0 + t] = (double)m + (double)star_score;
}

template <int P, bool STAR>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void align_viterbi_kernel(AlignArgs a, const double* xs) {
    // (xs: the star's emission per frame, indexed like a.lse; read only with STAR)
    constexpr int G = 8 / P;                 // steps per backpointer word
    constexpr int PF = P == 8 ? 2 : 8;       // steps the emissions are loaded ahead (a multiple of G; P = 8: registers)
    constexpr double NEG = -__builtin_inf();
    __shared__ double xv[2][LATTICE_MAX_THREADS + 1];    // exchange: entry i + 1 = thread i's last odd state; entry 0 = "state -1"
    __shared__ uint32_t win[LATTICE_WIN_WORDS];          // backtrace window of backpointer words
    __shared__ int path[LATTICE_CHUNK + 1];
    __shared__ int red[LATTICE_MAX_THREADS / 64];
    __shared__ double fin[2];
    __shared__ int s_cur;

    const AlignSeg sg = a.segs[blockIdx.x];
    const int tid = threadIdx.x, NT = a.nt, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const int k0 = tid * P;                  // this thread's pairs: k0 .. k0 + P - 1

    // labels of the thread's pairs (the blank past U), the skip flags, and the two per-utterance checks
    int lj[P];
    unsigned skipm = 0, starm = 0;                       // starm (STAR): the pairs whose label is the star
    bool bad = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = k0 + j;
        lj[j] = blank;
        if (k < U) {
            const int l = lab[k];
            if constexpr (STAR) bad |= l < 0 || l > V || l == blank;
            else bad |= l < 0 || l >= V || l == blank;
            if (k >= 1 && l != lab[k - 1]) skipm |= 1u << j;
            lj[j] = l;
            if constexpr (STAR) {
                if (l == V) {
                    starm |= 1u << j;
                    lj[j] = blank;                       // (the column this pair loads and discards)
                }
            }
        }
    }
    const int nbad = block_count(bad, red);
    int R = 0;                                           // repeats l_k = l_{k-1}
#pragma unroll
    for (int j = 0; j < P; ++j) R += block_count(k0 + j >= 1 && k0 + j < U && !(skipm >> j & 1u), red);
    if (nbad || T < U + R) {
        const double sc = nbad ? __builtin_nan("") : NEG;
        for (int t = tid; t < T; t += NT) {
            a.token[sg.out0 + t] = -1;
            a.label_index[sg.out0 + t] = -1;
            a.frame_logp[sg.out0 + t] = __builtin_nanf("");
        }
        if (tid == 0) a.score[blockIdx.x] = sc;
        return;                                          // (block-uniform)
    }

    // ---- sweep ----
    double ev[P], od[P];                                 // delta(2k), delta(2k + 1) of the thread's pairs
#pragma unroll
    for (int j = 0; j < P; ++j) {
        ev[j] = NEG;
        od[j] = NEG;
    }
    if (tid == 0) {
        ev[0] = (double)lg[blank];
        if (U >= 1) od[0] = (double)lg[lj[0]];
        if constexpr (STAR) {
            if (starm & 1u) od[0] = xs[sg.out0];
        }
    }
    for (int i = tid; i < 2 * (LATTICE_MAX_THREADS + 1); i += NT) (&xv[0][0])[i] = NEG;
    __syncthreads();
    xv[0][tid + 1] = od[P - 1];
    uint32_t* __restrict__ bpw = a.bp + sg.bp0 + tid;
    float qb[PF], ql[PF][P];                             // x_t(blank), x_t(l_k) of the next PF steps
    const double* __restrict__ xsr = STAR ? xs + sg.out0 : nullptr;
    double qs[STAR ? PF : 1];                            // xs_t of the next PF steps (STAR)
    qs[0] = 0.0;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const float* __restrict__ row = lg + (int64_t)min(1 + i, T - 1) * V;
        qb[i] = row[blank];
        if constexpr (STAR) qs[i] = xsr[min(1 + i, T - 1)];
#pragma unroll
        for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
    }
    uint32_t word = 0;
    auto step = [&](int t, float yb, const float* yl, double ys, int slot) {
        lds_barrier();
        const double nb = xv[(t - 1) & 1][tid];          // delta_{t-1}(2 k0 - 1)
        const double xb = (double)yb;
        uint32_t bits = 0;
#pragma unroll
        for (int j = P - 1; j >= 0; --j) {               // downwards: od[j - 1] is still the previous step's
            const double po = j ? od[j - 1] : nb;
            double me = ev[j];
            uint32_t be = 0;
            if (po > me) { me = po; be = 1; }
            double mo = od[j];
            uint32_t bo = 0;
            if (ev[j] > mo) { mo = ev[j]; bo = 1; }
            if ((skipm >> j & 1u) && po > mo) { mo = po; bo = 2; }
            const int k = k0 + j;
            if constexpr (STAR) od[j] = k < U ? mo + ((starm >> j & 1u) ? ys : (double)yl[j]) : NEG;
            else od[j] = k < U ? mo + (double)yl[j] : NEG;
            ev[j] = k <= U ? me + xb : NEG;
            bits |= (be | bo << 2) << (4 * j);
        }
        xv[t & 1][tid + 1] = od[P - 1];
        word |= bits << (slot * 4 * P);
    };
    // whole groups of PF steps without a branch between them (the compiler's wait counts then stay exact), then the tail
    int t0 = 1;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            step(t0 + i, qb[i], ql[i], qs[STAR ? i : 0], i % G);
            if (i % G == G - 1) {
                bpw[(int64_t)((t0 + i - 1) / G) * NT] = word;
                word = 0;
            }
            const float* __restrict__ row = lg + (int64_t)min(t0 + i + PF, T - 1) * V;      // (block-uniform row, per-lane column)
            qb[i] = row[blank];
            if constexpr (STAR) qs[i] = xsr[min(t0 + i + PF, T - 1)];
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (t0 + i < T) {                                // (block-uniform)
            step(t0 + i, qb[i], ql[i], qs[STAR ? i : 0], i % G);
            if (i % G == G - 1 || t0 + i == T - 1) {
                bpw[(int64_t)((t0 + i - 1) / G) * NT] = word;
                word = 0;
            }
        }
    }
    // end state
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (k0 + j == U) fin[0] = ev[j];                 // delta(S - 1)
        if (k0 + j + 1 == U) fin[1] = od[j];             // delta(S - 2)
    }
    __syncthreads();                                     // (also makes the backpointer stores visible to the block)
    const bool last_odd = U >= 1 && !(fin[0] > fin[1]);
    const double dend = last_odd ? fin[1] : fin[0];
    if (tid == 0) s_cur = last_odd ? 2 * U - 1 : 2 * U;

    // score: sum_t lse_t by wave 0 in a fixed order (lane l: frames l, l + 64, ...; then a butterfly), independent of P and NT
    if (tid < 64) {
        const double* __restrict__ ls = a.lse + sg.out0;
        double acc = 0.0;
#pragma unroll 8
        for (int t = tid; t < T; t += 64) acc += ls[t];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (tid == 0) a.score[blockIdx.x] = dend - acc;
    }

    // ---- backtrace, LATTICE_CHUNK frames per window ----
    const uint32_t* __restrict__ bpg = a.bp + sg.bp0;
    int t_hi = T - 1;
    __syncthreads();
    while (true) {
        const int t_lo = max(0, t_hi - LATTICE_CHUNK);
        const int s_hi = s_cur;
        // frames (t_lo, t_hi] read the words of step groups (t - 1) / G and of pairs (s_hi >> 1) - C + 1 .. s_hi >> 1
        const int ph = s_hi >> 1, pl = max(0, ph - LATTICE_CHUNK + 1);
        const int w_lo = pl / P, ncol = ph / P - w_lo + 1;
        const int g_lo = t_lo / G, nrow = t_hi > t_lo ? (t_hi - 1) / G - g_lo + 1 : 0;
        for (int i = tid; i < nrow * ncol; i += NT) {
            const int r = i / ncol, c = i - r * ncol;
            win[i] = bpg[(int64_t)(g_lo + r) * NT + w_lo + c];
        }
        __syncthreads();
        if (tid == 0) {
            int s = s_hi;
            for (int t = t_hi; t > t_lo; --t) {
                path[t - t_lo] = s;
                const int p = s >> 1, g = (t - 1) / G;
                const uint32_t w = win[(g - g_lo) * ncol + p / P - w_lo];
                s -= (int)(w >> (((t - 1) % G) * 4 * P + 4 * (p % P) + 2 * (s & 1)) & 3u);
            }
            path[0] = s;
            s_cur = s;
        }
        __syncthreads();
        for (int t = t_lo + (t_lo > 0) + tid; t <= t_hi; t += NT) {
            const int s = path[t - t_lo];
            const int tok = (s & 1) ? lab[s >> 1] : blank;
            const int64_t o = sg.out0 + t;
            a.token[o] = tok;
            a.label_index[o] = (s & 1) ? (s >> 1) : -1;
            if constexpr (STAR) a.frame_logp[o] = (float)((tok == V ? xsr[t] : (double)lg[(int64_t)t * V + tok]) - a.lse[o]);
            else a.frame_logp[o] = (float)((double)lg[(int64_t)t * V + tok] - a.lse[o]);
        }
        if (t_lo == 0) break;
        t_hi = t_lo;
    }
}

}  // namespace

namespace {

int align_launch(bool star, float star_score, const float* logits, int V, int n, const int64_t* row0, const int32_t* frames,
                 const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, int32_t* token, int32_t* label_index,
                 float* frame_logp, double* score, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && labels && label0 && nlabels && token && label_index && frame_logp && score,
                 "ctc_align: null argument");
    W2V2_REQUIRE(n >= 1, "ctc_align: %d utterances (need at least one)", n);
    W2V2_REQUIRE(V >= 1, "ctc_align: vocabulary of %d entries", V);
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_align: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(!star || star_score <= 0.f, "ctc_align: star_score %g (a log-domain penalty per frame: <= 0, not NaN)", (double)star_score);
    int Umax = 0, Tmax = 0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(frames[i] >= 1, "ctc_align: utterance %d has %d frames (need at least one)", i, frames[i]);
        W2V2_REQUIRE(row0[i] >= 0 && label0[i] >= 0, "ctc_align: utterance %d has a negative offset", i);
        W2V2_REQUIRE(nlabels[i] >= 0, "ctc_align: utterance %d has %d labels", i, nlabels[i]);
        W2V2_REQUIRE(nlabels[i] <= W2V2_ALIGN_MAX_LABELS, "ctc_align: utterance %d has %d labels; at most %d per utterance", i,
                     nlabels[i], W2V2_ALIGN_MAX_LABELS);
        Umax = std::max(Umax, (int)nlabels[i]);
        Tmax = std::max(Tmax, (int)frames[i]);
    }
    // pairs per thread from the largest label count
    const int pairs = Umax + 1;
    const int P = pairs_per_thread(pairs), G = 8 / P;
    const int nt = (((pairs + P - 1) / P + 63) / 64) * 64;
    std::vector<AlignSeg> segs((size_t)n);
    int64_t out = 0, words = 0;
    for (int i = 0; i < n; ++i) {
        segs[i] = AlignSeg{row0[i], label0[i], out, words, frames[i], nlabels[i]};
        out += frames[i];
        words += (int64_t)((frames[i] - 1 + G - 1) / G) * nt;
    }
    // workspace: the table | lse (fp64, sum T_i) | xs (the same, star calls only) | backpointer words
    const size_t tab_bytes = up256((size_t)n * sizeof(AlignSeg)), lse_bytes = up256((size_t)out * sizeof(double));
    const size_t xs_bytes = star ? lse_bytes : 0;
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_ALIGN, s, tab_bytes + lse_bytes + xs_bytes + (size_t)std::max<int64_t>(words, 1) * sizeof(uint32_t), &raw))
        return e;
    AlignArgs a;
    a.logits = logits;
    a.labels = labels;
    a.segs = static_cast<const AlignSeg*>(raw);
    a.lse = reinterpret_cast<double*>(static_cast<char*>(raw) + tab_bytes);
    double* xs = star ? reinterpret_cast<double*>(static_cast<char*>(raw) + tab_bytes + lse_bytes) : nullptr;
    a.bp = reinterpret_cast<uint32_t*>(static_cast<char*>(raw) + tab_bytes + lse_bytes + xs_bytes);
    a.token = token;
    a.label_index = label_index;
    a.frame_logp = frame_logp;
    a.score = score;
    a.V = V;
    a.blank = blank;
    a.nt = nt;
    if (int e = staged_upload(SCRATCH_ALIGN, s, raw, {{segs.data(), (size_t)n * sizeof(AlignSeg), 0}}, (size_t)16 << 10)) return e;
    // (work for the profile: the sweep's ~12 fp64 operations per state and step; the logits read once by the lse pass)
    ProfScope ps(nullptr, FAM_CTC, 12.0 * (double)out * (2.0 * Umax + 1.0), 4.0 * (double)out * V, s);
    if (star) {
        W2V2_LAUNCH(align_lse_star_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a, xs, star_score);
        dispatch_pairs(P, [&](auto p) {
            W2V2_LAUNCH((align_viterbi_kernel<decltype(p)::value, true>), dim3((unsigned)n), dim3((unsigned)a.nt), 0, s, a, (const double*)xs);
        });
    } else {
        W2V2_LAUNCH(align_lse_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
        dispatch_pairs(P, [&](auto p) {
            W2V2_LAUNCH((align_viterbi_kernel<decltype(p)::value, false>), dim3((unsigned)n), dim3((unsigned)a.nt), 0, s, a, (const double*)xs);
        });
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace

int launch_ctc_align(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                     const int64_t* label0, const int32_t* nlabels, int blank, int32_t* token, int32_t* label_index,
                     float* frame_logp, double* score, hipStream_t s) {
    return align_launch(false, 0.f, logits, V, n, row0, frames, labels, label0, nlabels, blank, token, label_index, frame_logp, score, s);
}

int launch_ctc_align_star(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                          const int64_t* label0, const int32_t* nlabels, int blank, float star_score, int32_t* token,
                          int32_t* label_index, float* frame_logp, double* score, hipStream_t s) {
    return align_launch(true, star_score, logits, V, n, row0, frames, labels, label0, nlabels, blank, token, label_index, frame_logp, score, s);
}

}  // namespace w2v2
