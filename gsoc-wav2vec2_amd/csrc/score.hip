// Exact CTC scoring: the log-probability of a label string given an utterance's logits, summed over ALL frame paths that spell
// it (the CTC forward recursion), for m (utterance, label string) pairs at once (w2v2_ctc_score).
//
// Definition (tests/score_reference.py implements exactly this in fp64 numpy).  x_t(v) is the fp32 logit widened to fp64;
// lp_t(v) = x_t(v) - lse_t, lse_t the fp64 log-sum-exp of the frame (ctc_lattice.h: frame_lse, the one the aligners and the beam
// search use).  ext is the label string with blanks interleaved, S = 2U + 1 states,
// ext[2k] = blank, ext[2k + 1] = l_k.  lse() below is the log-sum-exp of its finite arguments, -inf when all are -inf.
//   alpha_0(0) = lp_0(blank); alpha_0(1) = lp_0(l_0) if U >= 1; every other state -inf.
//   alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [ext[s] != blank and ext[s] != ext[s-2]] alpha_{t-1}(s-2)) + lp_t(ext[s]).
//   logp = lse(alpha_{T-1}(S-1), alpha_{T-1}(S-2)); U = 0: alpha_{T-1}(0).
// Conventions, as w2v2_ctc_align: T < U + R, R = #{k >= 1: l_k = l_{k-1}}, has no path: logp = -inf (a result, no error).  A label
// outside [0, V) or equal to the blank (labels are on the device): NaN.  An utterance with a NaN or +inf logit (or a frame of
// -inf only) has a frame whose lse_t is not finite: NaN for each of its pairs.  -inf logits are legal: a path through one has
// probability 0.
//
// Arithmetic: fp64 log space throughout.  An emission of e^-2000 is the number -2000, so nothing underflows and no path is
// flushed; the price is two or three transcendentals per state and step on the serial chain.  lse(a, b) is evaluated as
// hi + log(1 + exp(lo - hi)) and lse(a, b, c) as m + log(1 + exp(y - m) + exp(lo - m)) with m >= y >= lo, so the largest term
// costs no exp; the per-step error is a few ulp of max(1, |alpha|), which is what the tests' 16 T 2^-52 max(1, |logp|) bounds.
//
// Structure.  score_lse_kernel: one wave per frame, lse_t of every UTTERANCE (not pair) into the workspace.
// score_alpha_kernel: one block per pair.  A thread owns P consecutive state pairs (2k blank, 2k + 1 label k) in registers; per
// step the only value that crosses threads is the odd state of a thread's last pair, through a double-buffered LDS array behind
// ONE lds_barrier, and the P + 1 emissions and lse_t of a step are loaded PF steps ahead (8, 8, 4, 1 for P = 1, 2, 4, 8: what
// 128 registers at 1024 threads leave) -- align.hip's sweep without the backpointers, on lse2 and lse3 of ctc_lattice.h.
// P is chosen from the pair's OWN label count (pairs_per_thread: 1, 2, 4 up to 255, 511, 1023
// labels on 256 threads; 8 beyond, up to 1024 threads), the call launches one grid per P that occurs, and within a grid the pairs
// are ordered by utterance so that an utterance's rows stay in L2 for its hypotheses.  A state's value is the same sequence of
// fp64 operations whatever P, the block size or the neighbours: each pair is computed as if alone, and its bits do not depend
// on the other pairs of the call, their order or repetition.  No atomics.
#include "ctc_lattice.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace w2v2 {
namespace {

struct ScoreUtt {
    int64_t row0;      // first logits row
    int64_t lse0;      // first entry of the utterance's lse
    int32_t T, pad;
};

struct ScorePair {
    int64_t row0;      // first logits row of the pair's utterance
    int64_t lse0;      // first entry of its lse
    int64_t label0;    // first label
    int32_t T, U;
    int32_t out, pad;  // index of the pair in the caller's order
};

struct ScoreArgs {
    const float* logits;
    const int32_t* labels;
    const ScoreUtt* utts;
    const ScorePair* pairs;     // sorted by (P, utterance, caller's index)
    double* lse;                // (sum T_i over the utterances)
    double* logp;
    int V, blank;
};

// lse_t of frame t of utterance blockIdx.y: one wave per frame, grid.x covers the longest utterance
__global__ __launch_bounds__(256) void score_lse_kernel(ScoreArgs a) {
    const ScoreUtt u = a.utts[blockIdx.y];
    frame_lse(a.logits, a.V, u.row0, u.T, a.lse + u.lse0);
}

template <int P>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_alpha_kernel(ScoreArgs a, int pair0) {
    constexpr int PF = P == 8 ? 1 : P == 4 ? 4 : 8;      // steps the emissions are loaded ahead (registers)
    constexpr double NEG = -__builtin_inf();
    __shared__ double xv[2][LATTICE_MAX_THREADS + 1];    // exchange: entry i + 1 = thread i's last odd state; entry 0 = "state -1"
    __shared__ int red[LATTICE_MAX_THREADS / 64];
    __shared__ double fin[2];

    const ScorePair sg = a.pairs[pair0 + blockIdx.x];
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const double* __restrict__ ls = a.lse + sg.lse0;
    const int k0 = tid * P;                  // this thread's pairs: k0 .. k0 + P - 1

    // labels of the thread's pairs (the blank past U), the skip flags, and the per-pair checks
    int lj[P];
    unsigned skipm = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = k0 + j;
        lj[j] = blank;
        if (k < U) {
            const int l = lab[k];
            bad |= l < 0 || l >= V || l == blank;
            if (k >= 1 && l != lab[k - 1]) skipm |= 1u << j;
            lj[j] = bad ? blank : l;                     // (never an address outside the row)
        }
    }
    // a frame whose lse is not finite: the utterance holds a NaN or +inf logit, or a frame of -inf only
    bool nonfinite = false;
    for (int t = tid; t < T; t += NT) {
        const double v = ls[t];
        nonfinite |= !(v - v == 0.0);
    }
    const int nbad = block_count(bad || nonfinite, red);
    int R = 0;                                           // repeats l_k = l_{k-1}
#pragma unroll
    for (int j = 0; j < P; ++j) R += block_count(k0 + j >= 1 && k0 + j < U && !(skipm >> j & 1u), red);
    if (nbad || T < U + R) {
        if (tid == 0) a.logp[sg.out] = nbad ? __builtin_nan("") : NEG;
        return;                                          // (block-uniform)
    }

    double ev[P], od[P];                                 // alpha(2k), alpha(2k + 1) of the thread's pairs
#pragma unroll
    for (int j = 0; j < P; ++j) {
        ev[j] = NEG;
        od[j] = NEG;
    }
    if (tid == 0) {
        const double l0 = ls[0];
        ev[0] = (double)lg[blank] - l0;
        if (U >= 1) od[0] = (double)lg[lj[0]] - l0;
    }
    for (int i = tid; i < 2 * (LATTICE_MAX_THREADS + 1); i += NT) (&xv[0][0])[i] = NEG;
    __syncthreads();
    xv[0][tid + 1] = od[P - 1];
    float qb[PF], ql[PF][P];                             // x_t(blank), x_t(l_k) of the next PF steps
    double qs[PF];                                       // lse_t
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int tt = min(1 + i, T - 1);
        const float* __restrict__ row = lg + (int64_t)tt * V;
        qb[i] = row[blank];
        qs[i] = ls[tt];
#pragma unroll
        for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
    }
    auto step = [&](int t, float yb, const float* yl, double lt) {
        lds_barrier();
        const double nb = xv[(t - 1) & 1][tid];          // alpha_{t-1}(2 k0 - 1)
        const double lb = (double)yb - lt;
#pragma unroll
        for (int j = P - 1; j >= 0; --j) {               // downwards: od[j - 1] is still the previous step's
            const double po = j ? od[j - 1] : nb;
            const double ne = lse2(ev[j], po);
            const double no = lse3(od[j], ev[j], (skipm >> j & 1u) ? po : NEG);
            const int k = k0 + j;
            od[j] = k < U ? no + ((double)yl[j] - lt) : NEG;
            ev[j] = k <= U ? ne + lb : NEG;
            if (P == 8) __builtin_amdgcn_sched_barrier(0);       // (one pair's exp / log chains at a time: 128 registers at 1024 threads)
        }
        xv[t & 1][tid + 1] = od[P - 1];
    };
    // whole groups of PF steps without a branch between them, then the tail
    int t0 = 1;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            step(t0 + i, qb[i], ql[i], qs[i]);
            const int tt = min(t0 + i + PF, T - 1);      // (block-uniform row, per-lane column)
            const float* __restrict__ row = lg + (int64_t)tt * V;
            qb[i] = row[blank];
            qs[i] = ls[tt];
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (t0 + i < T) step(t0 + i, qb[i], ql[i], qs[i]);       // (block-uniform)
    }
    // end states
    if (tid == 0) fin[1] = NEG;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (k0 + j == U) fin[0] = ev[j];                 // alpha(S - 1)
        if (k0 + j + 1 == U) fin[1] = od[j];             // alpha(S - 2)
    }
    __syncthreads();
    if (tid == 0) a.logp[sg.out] = U >= 1 ? lse2(fin[0], fin[1]) : fin[0];
}

inline int score_pairs_per_thread(int U) { return pairs_per_thread(U + 1); }

}  // namespace

int launch_ctc_score(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                     const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, double* logp, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && utt_of && labels && label0 && nlabels && logp, "ctc_score: null argument");
    W2V2_REQUIRE(n >= 1, "ctc_score: %d utterances (need at least one)", n);
    W2V2_REQUIRE(m >= 1, "ctc_score: %d pairs (need at least one)", m);
    W2V2_REQUIRE(V >= 2, "ctc_score: vocabulary of %d entries (need the blank and a label)", V);
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_score: blank index %d outside vocabulary %d", blank, V);
    int Tmax = 0;
    std::vector<ScoreUtt> utts((size_t)n);
    int64_t out = 0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(frames[i] >= 1, "ctc_score: utterance %d has %d frames (need at least one)", i, frames[i]);
        W2V2_REQUIRE(row0[i] >= 0, "ctc_score: utterance %d has a negative offset", i);
        utts[i] = ScoreUtt{row0[i], out, frames[i], 0};
        out += frames[i];
        Tmax = std::max(Tmax, (int)frames[i]);
    }
    double work = 0.0;
    for (int j = 0; j < m; ++j) {
        W2V2_REQUIRE(utt_of[j] >= 0 && utt_of[j] < n, "ctc_score: pair %d scores utterance %d of %d", j, utt_of[j], n);
        W2V2_REQUIRE(label0[j] >= 0, "ctc_score: pair %d has a negative offset", j);
        W2V2_REQUIRE(nlabels[j] >= 0, "ctc_score: pair %d has %d labels", j, nlabels[j]);
        W2V2_REQUIRE(nlabels[j] <= W2V2_SCORE_MAX_LABELS, "ctc_score: pair %d has %d labels; at most %d per pair", j, nlabels[j],
                     W2V2_SCORE_MAX_LABELS);
        work += (double)frames[utt_of[j]] * (2.0 * nlabels[j] + 1.0);
    }
    // the pairs by (pairs per thread, utterance, caller's index): one grid per P, an utterance's hypotheses adjacent
    std::vector<int> order((size_t)m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const int px = score_pairs_per_thread(nlabels[x]), py = score_pairs_per_thread(nlabels[y]);
        return px != py ? px < py : utt_of[x] < utt_of[y];
    });
    std::vector<ScorePair> pairs((size_t)m);
    for (int i = 0; i < m; ++i) {
        const int j = order[i];
        const ScoreUtt& u = utts[utt_of[j]];
        pairs[i] = ScorePair{u.row0, u.lse0, label0[j], u.T, nlabels[j], j, 0};
    }
    // workspace: the utterance table | the pair table | lse (fp64, sum T_i)
    const size_t utt_bytes = up256((size_t)n * sizeof(ScoreUtt)), pair_bytes = up256((size_t)m * sizeof(ScorePair));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_SCORE, s, utt_bytes + pair_bytes + (size_t)out * sizeof(double), &raw)) return e;
    ScoreArgs a;
    a.logits = logits;
    a.labels = labels;
    a.utts = static_cast<const ScoreUtt*>(raw);
    a.pairs = reinterpret_cast<const ScorePair*>(static_cast<char*>(raw) + utt_bytes);
    a.lse = reinterpret_cast<double*>(static_cast<char*>(raw) + utt_bytes + pair_bytes);
    a.logp = logp;
    a.V = V;
    a.blank = blank;
    if (int e = staged_upload(SCRATCH_SCORE, s, raw,
                              {{utts.data(), (size_t)n * sizeof(ScoreUtt), 0}, {pairs.data(), (size_t)m * sizeof(ScorePair), utt_bytes}},
                              (size_t)64 << 10))
        return e;
    // (work for the profile: ~100 fp64 operations per state and step, the exp and log included; the logits read once by the lse pass)
    ProfScope ps(nullptr, FAM_CTC, 100.0 * work, 4.0 * (double)out * V, s);
    W2V2_LAUNCH(score_lse_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
    for (int i = 0; i < m;) {
        const int P = score_pairs_per_thread(pairs[i].U);
        int e = i, Umax = 0;
        for (; e < m && score_pairs_per_thread(pairs[e].U) == P; ++e) Umax = std::max(Umax, (int)pairs[e].U);
        const int nt = (((Umax + 1 + P - 1) / P + 63) / 64) * 64;
        dispatch_pairs(P, [&](auto p) {
            W2V2_LAUNCH(score_alpha_kernel<decltype(p)::value>, dim3((unsigned)(e - i)), dim3((unsigned)nt), 0, s, a, i);
        });
        i = e;
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
