// Exact CTC scoring, its gradient, and both with a star (w2v2_ctc_score, w2v2_ctc_score_grad, w2v2_ctc_score_star,
// w2v2_ctc_score_grad_star): one scorer, whose kernels take the star and the stored plane as template
// parameters; its host code is a template on the star and takes the gradient as a flag.
//
// 1. The score (tests/score_reference.py implements exactly this in fp64 numpy): the log-probability of a label string given an
// utterance's logits, summed over ALL frame paths that spell it, for m (utterance, label string) pairs at once.  x_t(v) is the
// fp32 logit widened to fp64; lp_t(v) = x_t(v) - lse_t, lse_t the fp64 log-sum-exp of the frame (ctc_lattice.h: frame_lse, the one
// the aligners and the beam search use).  ext is the label string with blanks interleaved, S = 2U + 1 states, ext[2k] = blank,
// ext[2k + 1] = l_k.  lse() below is the log-sum-exp of its finite arguments, -inf when all are -inf.
//   alpha_0(0) = lp_0(blank); alpha_0(1) = lp_0(l_0) if U >= 1; every other state -inf.
//   alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [ext[s] != blank and ext[s] != ext[s-2]] alpha_{t-1}(s-2)) + lp_t(ext[s]).
//   logp = lse(alpha_{T-1}(S-1), alpha_{T-1}(S-2)); U = 0: alpha_{T-1}(0).
// Conventions, as w2v2_ctc_align: T < U + R, R = #{k >= 1: l_k = l_{k-1}}, has no path: logp = -inf (a result, no error).  A label
// outside [0, V) or equal to the blank (labels are on the device): NaN.  An utterance with a NaN or +inf logit (or a frame of
// -inf only) has a frame whose lse_t is not finite: NaN for each of its pairs.  -inf logits are legal: a path through one has
// probability 0.
// Arithmetic: fp64 log space throughout.  An emission of e^-2000 is the number -2000, so nothing underflows and no path is
// flushed; the price is two or three transcendentals per state and step on the serial chain.  lse(a, b) is evaluated as
// hi + log(1 + exp(lo - hi)) and lse(a, b, c) as m + log(1 + exp(y - m) + exp(lo - m)) with m >= y >= lo, so the largest term
// costs no exp; the per-step error is a few ulp of max(1, |alpha|), which is what the tests' 16 T 2^-52 max(1, |logp|) bounds.
//
// 2. The gradient (tests/score_grad_reference.py): G = sum_j c_j d logp_j / d logits over pairs that share logits rows.  With
// c = -1 and one pair per utterance this is the gradient of the CTC loss in fp64 log space; with c_j = P_j (W_j - L) that of an
// expected risk over an n-best list (minimum word error rate training).  The backward variable EXCLUDES the frame's own emission,
// so no lp is ever subtracted and no inf - inf can form:
//   beta_{T-1}(S-1) = 0; beta_{T-1}(S-2) = 0 if U >= 1; every other state -inf.
//   beta_t(s) = lse(beta_{t+1}(s) + lp_{t+1}(ext[s]), beta_{t+1}(s+1) + lp_{t+1}(ext[s+1]),
//                   [s+2 < S and ext[s+2] != blank and ext[s+2] != ext[s]] (beta_{t+1}(s+2) + lp_{t+1}(ext[s+2]))).
//   gamma_t(s) = exp(alpha_t(s) + beta_t(s) - logp), 0 where alpha_t(s) or beta_t(s) is -inf.
//   Gamma_j(t, v) = sum over s with ext[s] = v of gamma_t(s);  y_t(v) = exp(lp_t(v));  d logp_j / d x_t(v) = Gamma_j(t, v) - y_t(v).
//   Utterance i over its pairs: G_i(t, v) = sum_j c_j Gamma_j(t, v) - (sum_j c_j) y_t(v), rounded once to fp32.
// A pair whose logp is -inf (too few frames, or every path through a -inf logit) or NaN (bad label, non-finite utterance)
// contributes nothing to either sum and reports that value in logp.  Every row of every utterance of the call is written, zeros
// where no pair contributes; rows of the buffer outside the utterances are not touched.
//
// 3. The star (tests/score_star_reference.py), the wildcard label of the aligners: the score of a partial transcript.
//   The label.  Label id V is the star, "as if the logits had one more column": the aligner's definition (align.hip).
//   Its emission.  lp_t(V) = ((double)m_t + (double)star_score) - lse_t.  m_t is the fp32 frame maximum (ctc_lattice.h:
//   frame_lse_max), blank included, NaN ignored; star_score <= 0 is an fp32 argument in nats per frame; lse_t is over the V real
//   columns only.
//   The recursion.  ext[2k + 1] = V is a state like any other.  The skip rule and R treat V like any id, so a star takes at least
//   one frame, and T < U + R gives -inf.  A label < 0, > V or equal to the blank gives NaN.
//   The value.  With a star, logp is a score of a set of paths, not a log-probability: the star's column is not part of the
//   softmax.  It may exceed 0.  It is never below the aligner's path score for the same input (a sum of non-negative terms that
//   holds the aligner's maximum).
//   The gradient.  a_t is the lowest column index with x_t(a_t) == m_t.  Then d lp_t(V) / d x_t(v) = [v = a_t] - y_t(v): the star
//   state emits the frame's top token.  Gamma_j(t, v) sums gamma over the states with ext[s] = v; for v = a_t it also sums the star
//   states.  G is unchanged, and sum_s gamma_t(s) = 1 still holds, so the fixed-point reduce below keeps its overflow argument.
//   What a loss built on this does on star frames: in proportion to the star's occupancy it sharpens the model's own top token;
//   it does not supervise which token.
//
// Structure.  STAR is a template parameter of every kernel: without it no xs_t or a_t is loaded or allocated, the mask below is
// the constant 0, and the select on it in a step is not compiled (if constexpr; the comment there says what it costs otherwise).
// score_lse_kernel<STAR>: one wave per frame; lse_t of every UTTERANCE (not pair) into the workspace, with the star also
// xs_t = m_t + star_score (fp64) and, for the gradient, a_t (int32).
// score_alpha_kernel<P, PLANE, STAR>: one block per pair.  A thread owns P consecutive state pairs (2k blank, 2k + 1 label k) in
// registers; per step the only value that crosses threads is the odd state of a thread's last pair, through a double-buffered LDS
// array behind ONE lds_barrier, and the P + 1 emissions, lse_t and xs_t of a step are loaded PF steps ahead (8, 8, 4, 1 for
// P = 1, 2, 4, 8: what 128 registers at 1024 threads leave) -- align.hip's sweep without the backpointers, on lse2 and lse3 of
// ctc_lattice.h, with align.hip's star scheme: a per-thread bit mask of the pairs that hold the star; an odd state adds
// xs_t - lse_t where the mask is set and x_t(l_k) - lse_t otherwise; a star pair's per-lane logits load reads the blank's column
// and is discarded, so no address leaves the row.  PLANE (the gradient): every step's states are stored to the pair's plane,
// fire-and-forget double2 stores behind lds_barrier, which does not wait for them.  P is chosen from the pair's OWN label count
// (pairs_per_thread: 1, 2, 4 up to 255, 511, 1023 labels on 256 threads; 8 beyond, up to 1024 threads), a pass launches one grid
// per P that occurs, and within a grid the pairs are ordered by utterance so that an utterance's rows stay in L2 for its
// hypotheses.
// score_beta_kernel<P, STAR>: the same thread layout run from the last frame to the first on b_t(s) = beta_t(s) + lp_t(ext[s]);
// what crosses threads is the FIRST pair of the next thread (two values); alpha_t is loaded one step ahead (P = 8: under the
// pair's own chains) and the plane entry is overwritten with gamma_t(s).
// score_reduce_kernel<STAR>: one block per (utterance, frame, 256 vocabulary columns); per pair, in the caller's order, gamma is
// gathered into columns as 2^-61 fixed point with integer adds in LDS (sum_s gamma_t(s) = 1, so 64 bits cannot overflow, and
// integer adds are exact whatever their order), then G += c_j Gamma_j in fp64, and (sum c) y_t(v) is subtracted at the end.  A
// star state's gamma is summed in registers like the blank's and added -- as an integer, before the one conversion to fp64 -- to
// column a_t.  No float atomics anywhere.
// A state's value is the same sequence of fp64 operations whatever P, PLANE, STAR, the block size or the neighbours: each pair is
// computed as if alone.  Its bits do not depend on the other pairs or utterances of the call, their order or repetition, the
// position in the buffer or the grouping below; w2v2_ctc_score_grad's logp carries w2v2_ctc_score's bits, and a pair without a
// star carries the star-free entry points' bits through the star ones, alone or mixed with star pairs (tests/test_score_bits_gpu.py
// pins all of it against the three separate files this one replaced; profiles/score_unify.md has the times).
//
// Workspace of a pass: tables | lse (fp64 per frame) | star: xs (fp64 per frame) | star and gradient: a (int32 per frame) |
// gradient: per pair T (2U + 2) fp64.  A gradient call that needs more than max_workspace_bytes runs the utterances in
// consecutive groups that fit, stream-ordered in the same scratch buffer.
#include "ctc_lattice.h"

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

namespace w2v2 {
namespace {

struct ScoreUtt {
    int64_t row0;      // first logits / gradient row
    int64_t lse0;      // first entry of the utterance's lse, xs and a
    int32_t T;
    int32_t q0, q1;    // its pairs: by_utt[q0 .. q1), in the caller's order
    int32_t pad;
};

struct ScorePair {
    int64_t row0;      // first logits row of the pair's utterance
    int64_t lse0;      // first entry of its lse, xs and a
    int64_t label0;    // first label
    int64_t plane0;    // first fp64 of its plane, T rows of 2 (U + 1) (gradient only; none when T < U: such a pair has no path)
    int32_t T, U;
    int32_t out, pad;  // index of the pair in the caller's order
};

// The kernels' arguments.  The star's three members exist with STAR only, and stand where they stand, so that every gradient
// kernel is instruction for instruction what it was when the star had a file of its own: as members of one struct for both, the
// star-free sweeps see other argument offsets, come out under another register numbering and run up to 2 % slower
// (score_alpha_kernel<1, true, false> +1.9 %, <4, true, false> +0.4 %, score_beta_kernel<2, false> +1.4 %, <4, false> +0.6 %:
// profiles/score_unify.md).
template <bool STAR>
struct ScoreArgs;
template <>
struct ScoreArgs<false> {
    const float* logits;
    const int32_t* labels;
    const ScoreUtt* utts;
    const ScorePair* pairs;     // sorted by (P, utterance, caller's index)
    const int32_t* by_utt;      // gradient: indices into pairs, sorted by (utterance, caller's index)
    double* lse;                // (sum T_i over the utterances of the pass)
    double* plane;              // gradient
    const double* coef;         // gradient
    double* logp;
    float* grad;                // gradient
    int V, blank;
};
template <>
struct ScoreArgs<true> {        // (the same, and)
    const float* logits;
    const int32_t* labels;
    const ScoreUtt* utts;
    const ScorePair* pairs;
    const int32_t* by_utt;
    double* lse;
    double* xs;                 // the star's raw emission m_t + star_score, indexed like lse
    int32_t* amax;              // gradient: a_t, indexed like lse
    double* plane;
    const double* coef;
    double* logp;
    float* grad;
    int V, blank;
    float star_score;
};

// lse_t, and with the star xs_t and (gradient) a_t, of frame t of utterance blockIdx.y: one wave per frame, grid.x covers the
// longest utterance
template <bool STAR>
__global__ __launch_bounds__(256) void score_lse_kernel(ScoreArgs<STAR> a) {
    const ScoreUtt u = a.utts[blockIdx.y];
    if constexpr (STAR) {
        float m;
        int am;
        const int t = frame_lse_max_arg(a.logits, a.V, u.row0, u.T, a.lse + u.lse0, m, am);
        if (t >= 0 && (threadIdx.x & 63) == 0) {
            a.xs[u.lse0 + t] = (double)m + (double)a.star_score;
            if (a.amax) a.amax[u.lse0 + t] = min(am, a.V - 1);      // (V: a frame of NaN only, whose utterance contributes nothing)
        }
    } else {
        frame_lse(a.logits, a.V, u.row0, u.T, a.lse + u.lse0);
    }
}

template <int P, bool PLANE, bool STAR>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_alpha_kernel(ScoreArgs<STAR> a, int pair0) {
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
    const double* __restrict__ xsr = nullptr;
    if constexpr (STAR) xsr = a.xs + sg.lse0;
    const int k0 = tid * P;                  // this thread's pairs: k0 .. k0 + P - 1

    // labels of the thread's pairs (the blank past U), the skip flags, the star mask, and the per-pair checks
    int lj[P];
    unsigned skipm = 0, starm = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = k0 + j;
        lj[j] = blank;
        if (k < U) {
            const int l = lab[k];
            bad |= l < 0 || (STAR ? l > V : l >= V) || l == blank;
            if (k >= 1 && l != lab[k - 1]) skipm |= 1u << j;
            if (STAR && l == V) starm |= 1u << j;
            lj[j] = (bad || (STAR && l == V)) ? blank : l;           // (never an address outside the row: a star pair loads the blank's column)
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
        return;                                          // (block-uniform; T >= U from here on, so a gradient pair has a plane)
    }
    double2* __restrict__ plane = PLANE ? reinterpret_cast<double2*>(a.plane + sg.plane0) + k0 : nullptr;
    const int64_t W = U + 1;                             // double2 per plane row

    double ev[P], od[P];                                 // alpha(2k), alpha(2k + 1) of the thread's pairs
#pragma unroll
    for (int j = 0; j < P; ++j) {
        ev[j] = NEG;
        od[j] = NEG;
    }
    if (tid == 0) {
        const double l0 = ls[0];
        ev[0] = (double)lg[blank] - l0;
        if (U >= 1) od[0] = ((starm & 1u) ? xsr[0] : (double)lg[lj[0]]) - l0;
    }
    if constexpr (PLANE) {
#pragma unroll
        for (int j = 0; j < P; ++j)
            if (k0 + j <= U) plane[j] = make_double2(ev[j], od[j]);
    }
    for (int i = tid; i < 2 * (LATTICE_MAX_THREADS + 1); i += NT) (&xv[0][0])[i] = NEG;
    __syncthreads();
    xv[0][tid + 1] = od[P - 1];
    float qb[PF], ql[PF][P];                             // x_t(blank), x_t(l_k) of the next PF steps
    double qs[PF], qx[PF];                               // lse_t, xs_t
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int tt = min(1 + i, T - 1);
        const float* __restrict__ row = lg + (int64_t)tt * V;
        qb[i] = row[blank];
        qs[i] = ls[tt];
        qx[i] = STAR ? xsr[tt] : 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
    }
    auto step = [&](int t, float yb, const float* yl, double lt, double ys) {
        lds_barrier();
        const double nb = xv[(t - 1) & 1][tid];          // alpha_{t-1}(2 k0 - 1)
        const double lb = (double)yb - lt;
        double2* __restrict__ prow = PLANE ? plane + (int64_t)t * W : nullptr;
#pragma unroll
        for (int j = P - 1; j >= 0; --j) {               // downwards: od[j - 1] is still the previous step's
            const double po = j ? od[j - 1] : nb;
            const double ne = lse2(ev[j], po);
            const double no = lse3(od[j], ev[j], (skipm >> j & 1u) ? po : NEG);
            const int k = k0 + j;
            // (without STAR the mask test is not compiled: left to the optimiser, the constant mask folds only after the sweeps at
            // 8 pairs per thread have taken another shape, 102 and 107 registers for 121 and 128, in which they run 31 % (no plane)
            // and 8 % (plane) slower: profiles/score_unify.md)
            if constexpr (STAR) od[j] = k < U ? no + (((starm >> j & 1u) ? ys : (double)yl[j]) - lt) : NEG;
            else od[j] = k < U ? no + ((double)yl[j] - lt) : NEG;
            ev[j] = k <= U ? ne + lb : NEG;
            if constexpr (PLANE) {
                if (k <= U) prow[j] = make_double2(ev[j], od[j]);
            }
            if (P == 8) __builtin_amdgcn_sched_barrier(0);       // (one pair's exp / log chains at a time: 128 registers at 1024 threads)
        }
        xv[t & 1][tid + 1] = od[P - 1];
    };
    // whole groups of PF steps without a branch between them, then the tail
    int t0 = 1;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            step(t0 + i, qb[i], ql[i], qs[i], qx[i]);
            const int tt = min(t0 + i + PF, T - 1);      // (block-uniform row, per-lane column)
            const float* __restrict__ row = lg + (int64_t)tt * V;
            qb[i] = row[blank];
            qs[i] = ls[tt];
            qx[i] = STAR ? xsr[tt] : 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (t0 + i < T) step(t0 + i, qb[i], ql[i], qs[i], qx[i]);       // (block-uniform)
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

// The beta sweep: frames T - 1 down to 0 on b_t(s) = beta_t(s) + lp_t(ext[s]); the plane's alpha_t(s) becomes gamma_t(s)
template <int P, bool STAR>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_beta_kernel(ScoreArgs<STAR> a, int pair0) {
    constexpr int PF = P == 8 ? 1 : P == 4 ? 4 : 8;
    constexpr double NEG = -__builtin_inf();
    __shared__ double xe[2][LATTICE_MAX_THREADS + 1];    // entry i = thread i's first even state; entry NT = "state S"
    __shared__ double xo[2][LATTICE_MAX_THREADS + 1];    // its first odd state

    const ScorePair sg = a.pairs[pair0 + blockIdx.x];
    const double logp = a.logp[sg.out];                  // (the alpha sweep's, earlier on the stream)
    if (!(logp - logp == 0.0)) return;                   // -inf or NaN: no contribution, and no plane to touch (block-uniform)
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const double* __restrict__ ls = a.lse + sg.lse0;
    const double* __restrict__ xsr = nullptr;
    if constexpr (STAR) xsr = a.xs + sg.lse0;
    const int k0 = tid * P;
    double2* __restrict__ plane = reinterpret_cast<double2*>(a.plane + sg.plane0) + k0;
    const int64_t W = U + 1;

    // labels of the thread's pairs (all valid: logp is finite), the star mask, and whether state 2k + 1 may skip to 2k + 3
    int lj[P];
    unsigned skipn = 0, starm = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = k0 + j;
        const int l = k < U ? lab[k] : blank;
        if (k + 1 < U && lab[k + 1] != l) skipn |= 1u << j;
        if (STAR && l == V) starm |= 1u << j;
        lj[j] = (STAR && l == V) ? blank : l;                        // (a star pair loads the blank's column and discards it)
    }
    for (int i = tid; i < 2 * (LATTICE_MAX_THREADS + 1); i += NT) {
        (&xe[0][0])[i] = NEG;
        (&xo[0][0])[i] = NEG;
    }
    // frame T - 1
    double be[P], bo[P];
    double2 av[P];                                       // alpha of the frame the next step handles
    {
        const float* __restrict__ row = lg + (int64_t)(T - 1) * V;
        const double lt = ls[T - 1];
        const double ys = STAR ? xsr[T - 1] : 0.0;
        const double lb = (double)row[blank] - lt;
        double2* __restrict__ prow = plane + (int64_t)(T - 1) * W;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int k = k0 + j;
            const bool e_end = k == U, o_end = k + 1 == U;
            if (k <= U) {
                const double2 al = prow[j];
                prow[j] = make_double2(e_end ? exp(al.x - logp) : 0.0, o_end ? exp(al.y - logp) : 0.0);
            }
            be[j] = e_end ? lb : NEG;
            bo[j] = o_end ? ((starm >> j & 1u) ? ys : (double)row[lj[j]]) - lt : NEG;
            av[j] = make_double2(NEG, NEG);
            if (P != 8 && T >= 2 && k <= U) av[j] = (prow - W)[j];
        }
    }
    __syncthreads();
    xe[(T - 1) & 1][tid] = be[0];
    xo[(T - 1) & 1][tid] = bo[0];
    float qb[PF], ql[PF][P];                             // x_t(blank), x_t(l_k) of the next PF steps (frames T - 2, T - 3, ...)
    double qs[PF], qx[PF];                               // lse_t, xs_t
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int tt = max(T - 2 - i, 0);
        const float* __restrict__ row = lg + (int64_t)tt * V;
        qb[i] = row[blank];
        qs[i] = ls[tt];
        qx[i] = STAR ? xsr[tt] : 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
    }
    auto step = [&](int t, float yb, const float* yl, double lt, double ys) {
        lds_barrier();
        const double e_nx = xe[(t + 1) & 1][tid + 1], o_nx = xo[(t + 1) & 1][tid + 1];      // b_{t+1}(2 (k0 + P)), (2 (k0 + P) + 1)
        const double lb = (double)yb - lt;
        double2* __restrict__ prow = plane + (int64_t)t * W;
#pragma unroll
        for (int j = 0; j < P; ++j) {                    // upwards: be[j + 1], bo[j + 1] are still the next frame's
            const int k = k0 + j;
            // P = 8: alpha_t is loaded here, under this pair's two lse chains (128 registers at 1024 threads hold no second set)
            if (P == 8 && k <= U) av[0] = prow[j];
            const double2 al = av[P == 8 ? 0 : j];
            const double e1 = j + 1 < P ? be[j + 1] : e_nx;
            const double o1 = j + 1 < P ? bo[j + 1] : o_nx;
            const double bev = lse2(be[j], bo[j]);
            const double bod = lse3(bo[j], e1, (skipn >> j & 1u) ? o1 : NEG);
            if (k <= U) {
                prow[j] = make_double2(exp(al.x + bev - logp), k < U ? exp(al.y + bod - logp) : 0.0);
                if (P != 8 && t > 0) av[j] = (prow - W)[j];
            }
            be[j] = k <= U ? bev + lb : NEG;
            if constexpr (STAR) bo[j] = k < U ? bod + (((starm >> j & 1u) ? ys : (double)yl[j]) - lt) : NEG;       // (as the alpha sweep's)
            else bo[j] = k < U ? bod + ((double)yl[j] - lt) : NEG;
            if (P == 8) __builtin_amdgcn_sched_barrier(0);
        }
        xe[t & 1][tid] = be[0];
        xo[t & 1][tid] = bo[0];
    };
    // step i handles frame T - 2 - i
    const int steps = T - 1;
    int i0 = 0;
    for (; i0 + PF <= steps; i0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            step(T - 2 - (i0 + i), qb[i], ql[i], qs[i], qx[i]);
            const int tt = max(T - 2 - (i0 + i + PF), 0);
            const float* __restrict__ row = lg + (int64_t)tt * V;
            qb[i] = row[blank];
            qs[i] = ls[tt];
            qx[i] = STAR ? xsr[tt] : 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (i0 + i < steps) step(T - 2 - (i0 + i), qb[i], ql[i], qs[i], qx[i]);       // (block-uniform)
    }
}

constexpr int REDUCE_COLS = 256;
constexpr double FIX_SCALE = 2305843009213693952.0;      // 2^61

// one block per (frame, utterance, 256 vocabulary columns)
template <bool STAR>
__global__ __launch_bounds__(REDUCE_COLS) void score_reduce_kernel(ScoreArgs<STAR> a) {
    __shared__ unsigned long long acc[REDUCE_COLS];
    __shared__ unsigned long long accb, accs;
    const ScoreUtt u = a.utts[blockIdx.y];
    const int t = blockIdx.x;
    if (t >= u.T) return;
    const int tid = threadIdx.x, V = a.V, blank = a.blank;
    const int v0 = blockIdx.z * REDUCE_COLS, v = v0 + tid;
    int am = -1;
    if constexpr (STAR) am = a.amax[u.lse0 + t];       // a_t: the column the star states' gamma goes to (block-uniform)
    double G = 0.0, csum = 0.0;
    bool any = false;
    for (int q = u.q0; q < u.q1; ++q) {
        const ScorePair pr = a.pairs[a.by_utt[q]];
        const double lp = a.logp[pr.out];
        if (!(lp - lp == 0.0)) continue;                 // (block-uniform)
        const double c = a.coef[pr.out];
        acc[tid] = 0ull;
        if (tid == 0) {
            accb = 0ull;
            accs = 0ull;
        }
        __syncthreads();
        const double* __restrict__ row = a.plane + pr.plane0 + (int64_t)t * (2 * ((int64_t)pr.U + 1));
        const int32_t* __restrict__ lab = a.labels + pr.label0;
        const int S = 2 * pr.U + 1;
        unsigned long long bsum = 0ull;                  // even states: the blank's column, summed in registers
        unsigned long long ssum = 0ull;                  // star states: column a_t, likewise
        for (int s = tid; s < S; s += REDUCE_COLS) {     // (the stride is even: a thread sees states of one parity)
            const unsigned long long fx = (unsigned long long)(row[s] * FIX_SCALE);
            if (s & 1) {
                const int lv = lab[s >> 1];
                const int l = lv - v0;
                if (STAR && lv == V) ssum += fx;
                else if (l >= 0 && l < REDUCE_COLS && fx) atomicAdd(&acc[l], fx);
            } else {
                bsum += fx;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bsum += __shfl_xor(bsum, off, 64);
            if constexpr (STAR) ssum += __shfl_xor(ssum, off, 64);
        }
        if ((tid & 63) == 0 && bsum) atomicAdd(&accb, bsum);
        if (STAR && (tid & 63) == 0 && ssum) atomicAdd(&accs, ssum);
        __syncthreads();
        // (integer sum before the one conversion: without a star state accs is 0 and the bits are the star-free kernel's)
        const unsigned long long fx = (v == blank ? accb : acc[tid]) + (STAR && v == am ? accs : 0ull);
        const double Gam = (double)fx * (1.0 / FIX_SCALE);
        G += c * Gam;
        csum += c;
        any = true;
        __syncthreads();                                 // (acc is cleared for the next pair)
    }
    if (v < V) {
        float g = 0.f;
        if (any) {
            const double y = exp((double)a.logits[(u.row0 + t) * V + v] - a.lse[u.lse0 + t]);
            g = (float)(G - csum * y);
        }
        a.grad[(u.row0 + t) * V + v] = g;
    }
}

inline int score_pairs_per_thread(int U) { return pairs_per_thread(U + 1); }
inline int64_t plane_doubles(int T, int U) { return T >= U ? (int64_t)T * 2 * ((int64_t)U + 1) : 0; }

// where the parts of one pass over ng utterances with mg pairs, frames frames in all and planes fp64 of planes begin; end = its bytes
struct PassLayout {
    size_t pairs, by_utt, lse, xs, amax, plane;          // (the utterance table at 0)
    int64_t end;
};
inline PassLayout pass_layout(int64_t ng, int64_t mg, int64_t frames, int64_t planes, bool grad, bool star) {
    PassLayout o;
    o.pairs = up256((size_t)ng * sizeof(ScoreUtt));
    o.by_utt = o.pairs + up256((size_t)mg * sizeof(ScorePair));
    o.lse = o.by_utt + (grad ? up256((size_t)mg * sizeof(int32_t)) : 0);
    o.xs = o.lse + up256((size_t)frames * sizeof(double));
    o.amax = o.xs + (star ? up256((size_t)frames * sizeof(double)) : 0);
    o.plane = o.amax + (star && grad ? up256((size_t)frames * sizeof(int32_t)) : 0);
    o.end = (int64_t)o.plane + planes * (int64_t)sizeof(double);
    return o;
}

int check_shapes(const char* who, int V, int n, const int32_t* frames, int m, const int32_t* utt_of, const int32_t* nlabels) {
    W2V2_REQUIRE(frames && utt_of && nlabels, "%s: null argument", who);
    W2V2_REQUIRE(n >= 1, "%s: %d utterances (need at least one)", who, n);
    W2V2_REQUIRE(m >= 1, "%s: %d pairs (need at least one)", who, m);
    W2V2_REQUIRE(V >= 2, "%s: vocabulary of %d entries (need the blank and a label)", who, V);
    for (int i = 0; i < n; ++i) W2V2_REQUIRE(frames[i] >= 1, "%s: utterance %d has %d frames (need at least one)", who, i, frames[i]);
    for (int j = 0; j < m; ++j) {
        W2V2_REQUIRE(utt_of[j] >= 0 && utt_of[j] < n, "%s: pair %d scores utterance %d of %d", who, j, utt_of[j], n);
        W2V2_REQUIRE(nlabels[j] >= 0, "%s: pair %d has %d labels", who, j, nlabels[j]);
        W2V2_REQUIRE(nlabels[j] <= W2V2_SCORE_MAX_LABELS, "%s: pair %d has %d labels; at most %d per pair", who, j, nlabels[j],
                     W2V2_SCORE_MAX_LABELS);
    }
    return W2V2_OK;
}

// the sweeps of pairs [i, i + blocks) of a pass, which share P
template <int P, bool STAR>
void launch_sweeps(const ScoreArgs<STAR>& a, bool with_grad, int i, int blocks, int nt, hipStream_t s) {
    if (with_grad) {
        W2V2_LAUNCH((score_alpha_kernel<P, true, STAR>), dim3((unsigned)blocks), dim3((unsigned)nt), 0, s, a, i);
        W2V2_LAUNCH((score_beta_kernel<P, STAR>), dim3((unsigned)blocks), dim3((unsigned)nt), 0, s, a, i);
    } else {
        W2V2_LAUNCH((score_alpha_kernel<P, false, STAR>), dim3((unsigned)blocks), dim3((unsigned)nt), 0, s, a, i);
    }
}

constexpr int64_t DEFAULT_CAP = (int64_t)8 << 30;
constexpr int MAX_GROUP_UTTS = 65535;                    // grid.y of the lse and reduce kernels

// All four entry points.  coef, grad and max_workspace_bytes belong to the gradient (with_grad), star_score to the star; slot is
// the entry point's own scratch buffer per stream.
template <bool STAR>
int score_run(const char* who, int slot, bool with_grad, const float* logits, int V, int n, const int64_t* row0,
              const int32_t* frames, int m, const int32_t* utt_of, const int32_t* labels, const int64_t* label0, const int32_t* nlabels,
              int blank, float star_score, const double* coef, double* logp, float* grad, int64_t max_workspace_bytes, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && utt_of && labels && label0 && nlabels && logp && (!with_grad || (coef && grad)),
                 "%s: null argument", who);
    if (int e = check_shapes(who, V, n, frames, m, utt_of, nlabels)) return e;
    W2V2_REQUIRE(blank >= 0 && blank < V, "%s: blank index %d outside vocabulary %d", who, blank, V);
    W2V2_REQUIRE(!STAR || star_score <= 0.f, "%s: star_score %g (a log-domain penalty per frame: <= 0, not NaN)", who, (double)star_score);
    W2V2_REQUIRE(max_workspace_bytes >= 0, "%s: max_workspace_bytes %lld is negative (0: the default of 8 GiB)", who,
                 (long long)max_workspace_bytes);
    for (int i = 0; i < n; ++i) W2V2_REQUIRE(row0[i] >= 0, "%s: utterance %d has a negative offset", who, i);
    for (int j = 0; j < m; ++j) W2V2_REQUIRE(label0[j] >= 0, "%s: pair %d has a negative offset", who, j);
    // (the scorer alone has no planes and no cap, and runs as ONE group, whatever the number of utterances)
    const int64_t cap = !with_grad ? std::numeric_limits<int64_t>::max() : max_workspace_bytes ? max_workspace_bytes : DEFAULT_CAP;

    // the pairs of each utterance, in the caller's order
    std::vector<int> first((size_t)n + 1, 0), of_utt((size_t)m);
    for (int j = 0; j < m; ++j) ++first[utt_of[j] + 1];
    for (int i = 0; i < n; ++i) first[i + 1] += first[i];
    {
        std::vector<int> fill(first.begin(), first.end() - 1);
        for (int j = 0; j < m; ++j) of_utt[fill[utt_of[j]]++] = j;
    }
    auto bytes = [&](int64_t ng, int64_t mg, int64_t fr, int64_t planes) { return pass_layout(ng, mg, fr, planes, with_grad, STAR).end; };
    // consecutive utterances in groups that fit; a single utterance that does not fit fails the call before anything is allocated
    struct Group { int u0, u1; int64_t bytes; };
    std::vector<Group> groups;
    double work = 0.0, rows = 0.0;                       // (for the profile: states x steps, and logits rows)
    {
        int u0 = 0;
        int64_t fr = 0, planes = 0, mg = 0;
        for (int i = 0; i < n; ++i) {
            int64_t pl = 0;
            for (int q = first[i]; q < first[i + 1]; ++q) {
                if (with_grad) pl += plane_doubles(frames[i], nlabels[of_utt[q]]);
                work += (double)frames[i] * (2.0 * nlabels[of_utt[q]] + 1.0);
            }
            rows += frames[i];
            const int64_t mi = first[i + 1] - first[i];
            const int64_t alone = bytes(1, mi, frames[i], pl);
            W2V2_REQUIRE(alone <= cap, "%s: utterance %d (%d frames, %lld pairs) needs %lld bytes of workspace; max_workspace_bytes is %lld",
                         who, i, frames[i], (long long)mi, (long long)alone, (long long)cap);
            if (with_grad && i > u0 && (bytes(i - u0 + 1, mg + mi, fr + frames[i], planes + pl) > cap || i - u0 >= MAX_GROUP_UTTS)) {
                groups.push_back(Group{u0, i, bytes(i - u0, mg, fr, planes)});
                u0 = i;
                fr = planes = mg = 0;
            }
            fr += frames[i];
            planes += pl;
            mg += mi;
        }
        groups.push_back(Group{u0, n, bytes(n - u0, mg, fr, planes)});
    }
    int64_t need = 0;
    for (const Group& g : groups) need = std::max(need, g.bytes);
    void* raw = nullptr;
    if (int e = stream_scratch(slot, s, (size_t)need, &raw)) return e;
    char* base = static_cast<char*>(raw);

    std::vector<ScoreUtt> utts;
    std::vector<ScorePair> pairs;
    std::vector<int32_t> by_utt;
    std::vector<int> order;
    std::vector<int64_t> plane0;
    for (const Group& g : groups) {
        const int ng = g.u1 - g.u0, mg = first[g.u1] - first[g.u0];
        const int* mine = of_utt.data() + first[g.u0];  // the group's pairs, q = position in (utterance, caller's index) order
        utts.resize((size_t)ng);
        int64_t fr = 0;
        int Tmax = 0;
        for (int i = g.u0; i < g.u1; ++i) {
            utts[i - g.u0] = ScoreUtt{row0[i], fr, frames[i], first[i] - first[g.u0], first[i + 1] - first[g.u0], 0};
            fr += frames[i];
            Tmax = std::max(Tmax, (int)frames[i]);
        }
        // sorted by (P, utterance, caller's index) for the sweeps: one grid per P, an utterance's hypotheses adjacent
        order.resize((size_t)mg);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(),
                         [&](int x, int y) { return score_pairs_per_thread(nlabels[mine[x]]) < score_pairs_per_thread(nlabels[mine[y]]); });
        plane0.resize((size_t)mg);
        int64_t pl = 0;
        for (int q = 0; q < mg; ++q) {
            plane0[q] = pl;
            if (with_grad) pl += plane_doubles(frames[utt_of[mine[q]]], nlabels[mine[q]]);
        }
        pairs.resize((size_t)std::max(mg, 1));           // (utterances without pairs: zero rows, from the reduce kernel alone)
        by_utt.resize((size_t)std::max(mg, 1));             // (by_utt and plane0 cost a pass over the pairs; only the gradient uploads them)
        for (int i = 0; i < mg; ++i) {
            const int q = order[i], j = mine[q];
            const ScoreUtt& u = utts[utt_of[j] - g.u0];
            pairs[i] = ScorePair{u.row0, u.lse0, label0[j], plane0[q], u.T, nlabels[j], j, 0};
            by_utt[q] = i;
        }
        const PassLayout at = pass_layout(ng, mg, fr, pl, with_grad, STAR);
        ScoreArgs<STAR> a{};
        a.logits = logits;
        a.labels = labels;
        a.utts = reinterpret_cast<const ScoreUtt*>(base);
        a.pairs = reinterpret_cast<const ScorePair*>(base + at.pairs);
        if (with_grad) a.by_utt = reinterpret_cast<const int32_t*>(base + at.by_utt);
        a.lse = reinterpret_cast<double*>(base + at.lse);
        if constexpr (STAR) {
            a.xs = reinterpret_cast<double*>(base + at.xs);
            if (with_grad) a.amax = reinterpret_cast<int32_t*>(base + at.amax);
            a.star_score = star_score;
        }
        if (with_grad) a.plane = reinterpret_cast<double*>(base + at.plane);
        a.coef = coef;
        a.logp = logp;
        a.grad = grad;
        a.V = V;
        a.blank = blank;
        if (int e = staged_upload(slot, s, raw,
                                  {{utts.data(), (size_t)ng * sizeof(ScoreUtt), 0},
                                   {pairs.data(), (size_t)mg * sizeof(ScorePair), at.pairs},
                                   {by_utt.data(), with_grad ? (size_t)mg * sizeof(int32_t) : 0, at.by_utt}},
                                  (size_t)64 << 10))
            return e;
        // the family of the launches below, opened behind the upload (no profiler: no interval is timed).  Work of the scorer:
        // ~100 fp64 operations per state and step, the exp and log included; the logits read once by the lse pass
        ProfScope ps(nullptr, FAM_CTC, with_grad ? 0.0 : 100.0 * work, with_grad ? 0.0 : 4.0 * rows * V, s);
        const dim3 lse_grid((unsigned)((Tmax + 3) / 4), (unsigned)ng);
        W2V2_LAUNCH(score_lse_kernel<STAR>, lse_grid, dim3(256), 0, s, a);
        for (int i = 0; i < mg;) {
            const int P = score_pairs_per_thread(pairs[i].U);
            int e = i, Umax = 0;
            for (; e < mg && score_pairs_per_thread(pairs[e].U) == P; ++e) Umax = std::max(Umax, (int)pairs[e].U);
            const int nt = (((Umax + 1 + P - 1) / P + 63) / 64) * 64;
            dispatch_pairs(P, [&](auto p) { launch_sweeps<decltype(p)::value, STAR>(a, with_grad, i, e - i, nt, s); });
            i = e;
        }
        if (with_grad) {
            const dim3 grid((unsigned)Tmax, (unsigned)ng, (unsigned)((V + REDUCE_COLS - 1) / REDUCE_COLS));
            W2V2_LAUNCH(score_reduce_kernel<STAR>, grid, dim3(REDUCE_COLS), 0, s, a);
        }
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace

int launch_ctc_score(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                     const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, bool star, float star_score,
                     double* logp, hipStream_t s) {
    if (star)
        return score_run<true>("ctc_score_star", SCRATCH_SCORE_STAR, false, logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels,
                               blank, star_score, nullptr, logp, nullptr, 0, s);
    return score_run<false>("ctc_score", SCRATCH_SCORE, false, logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels, blank, 0.f,
                            nullptr, logp, nullptr, 0, s);
}

int launch_ctc_score_grad(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                          const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, bool star, float star_score,
                          const double* coef, double* logp, float* grad, int64_t max_workspace_bytes, hipStream_t s) {
    if (star)
        return score_run<true>("ctc_score_grad_star", SCRATCH_SCORE_GRAD_STAR, true, logits, V, n, row0, frames, m, utt_of, labels, label0,
                               nlabels, blank, star_score, coef, logp, grad, max_workspace_bytes, s);
    return score_run<false>("ctc_score_grad", SCRATCH_SCORE_GRAD, true, logits, V, n, row0, frames, m, utt_of, labels, label0, nlabels,
                            blank, 0.f, coef, logp, grad, max_workspace_bytes, s);
}

int64_t ctc_score_grad_workspace(int n, const int32_t* frames, int m, const int32_t* utt_of, const int32_t* nlabels, int V, bool star) {
    if (int e = check_shapes(star ? "ctc_score_grad_star_workspace" : "ctc_score_grad_workspace", V, n, frames, m, utt_of, nlabels)) return e;
    int64_t fr = 0, planes = 0;
    for (int i = 0; i < n; ++i) fr += frames[i];
    for (int j = 0; j < m; ++j) planes += plane_doubles(frames[utt_of[j]], nlabels[j]);
    return pass_layout(n, m, fr, planes, true, star).end;
}

}  // namespace w2v2
