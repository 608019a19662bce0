// The gradient of a weighted sum of exact CTC log-probabilities, G = sum_j c_j d logp_j / d logits, over m (utterance, label
// string) pairs that share logits rows (w2v2_ctc_score_grad).  With c = -1 and one pair per utterance this is
// the gradient of the CTC loss in fp64 log space; with c_j = P_j (W_j - L) it is the gradient of an expected risk over an
// n-best list (minimum word error rate training).
//
// Definition (tests/score_grad_reference.py implements exactly this in fp64 numpy).  lp, ext, S = 2U + 1, the skip rule, alpha and
// logp are exactly those of score.hip.  The backward variable EXCLUDES the frame's own emission, so no lp is ever subtracted and
// no inf - inf can form:
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
// Structure.  score_grad_lse_kernel: score.hip's.  score_grad_alpha_kernel<P>: score_alpha_kernel<P> with every step's states
// stored to the pair's plane (fire-and-forget double2 stores behind lds_barrier, which does not wait for them).  It is a COPY,
// not a template flag on score.hip's kernel: the scorer keeps its instructions, bits and time by construction,
// and the copy is the same sequence of fp64 operations per state, so logp carries w2v2_ctc_score's bits.
// score_grad_beta_kernel<P>: the same thread layout run from the last frame to the first on b_t(s) = beta_t(s) + lp_t(ext[s]);
// what crosses threads is the FIRST pair of the next thread (two values); alpha_t is loaded one step ahead (P = 8: under the
// pair's own chains) and the plane entry is overwritten with gamma_t(s).  score_grad_reduce_kernel: one block per (utterance, frame, 256 vocabulary columns); per pair,
// in the caller's order, gamma is gathered into columns as 2^-61 fixed point with integer adds in LDS (sum_s gamma_t(s) = 1, so
// 64 bits cannot overflow, and integer adds are exact whatever their order), then G += c_j Gamma_j in fp64, and
// (sum c) y_t(v) is subtracted at the end.  No float atomics anywhere; bits do not depend on the other utterances of the call,
// their pairs or the position in the buffer, nor on the grouping below.
//
// Workspace: tables | lse (fp64 per frame) | per pair T (2U + 2) fp64.  A call that needs more than max_workspace_bytes runs the
// utterances in consecutive groups that fit, stream-ordered in the same scratch buffer.
#include "ctc_lattice.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace w2v2 {
namespace {

struct GradUtt {
    int64_t row0;      // first logits / gradient row
    int64_t lse0;      // first entry of the utterance's lse
    int32_t T;
    int32_t q0, q1;    // its pairs: by_utt[q0 .. q1), in the caller's order
    int32_t pad;
};

struct GradPair {
    int64_t row0;      // first logits row of the pair's utterance
    int64_t lse0;      // first entry of its lse
    int64_t label0;    // first label
    int64_t plane0;    // first fp64 of its plane, T rows of 2 (U + 1) (none when T < U: such a pair has no path)
    int32_t T, U;
    int32_t out, pad;  // index of the pair in the caller's order
};

struct GradArgs {
    const float* logits;
    const int32_t* labels;
    const GradUtt* utts;
    const GradPair* pairs;      // sorted by (P, utterance, caller's index)
    const int32_t* by_utt;      // indices into pairs, sorted by (utterance, caller's index)
    double* lse;
    double* plane;
    const double* coef;
    double* logp;
    float* grad;
    int V, blank;
};

__global__ __launch_bounds__(256) void score_grad_lse_kernel(GradArgs a) {
    const GradUtt u = a.utts[blockIdx.y];
    frame_lse(a.logits, a.V, u.row0, u.T, a.lse + u.lse0);
}

// score_alpha_kernel<P> of score.hip, state for state, with alpha_t stored to the plane
template <int P>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_grad_alpha_kernel(GradArgs a, int pair0) {
    constexpr int PF = P == 8 ? 1 : P == 4 ? 4 : 8;
    constexpr double NEG = -__builtin_inf();
    __shared__ double xv[2][LATTICE_MAX_THREADS + 1];
    __shared__ int red[LATTICE_MAX_THREADS / 64];
    __shared__ double fin[2];

    const GradPair sg = a.pairs[pair0 + blockIdx.x];
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const double* __restrict__ ls = a.lse + sg.lse0;
    const int k0 = tid * P;

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
            lj[j] = bad ? blank : l;
        }
    }
    bool nonfinite = false;
    for (int t = tid; t < T; t += NT) {
        const double v = ls[t];
        nonfinite |= !(v - v == 0.0);
    }
    const int nbad = block_count(bad || nonfinite, red);
    int R = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) R += block_count(k0 + j >= 1 && k0 + j < U && !(skipm >> j & 1u), red);
    if (nbad || T < U + R) {
        if (tid == 0) a.logp[sg.out] = nbad ? __builtin_nan("") : NEG;
        return;                                          // (block-uniform; T >= U from here on, so the pair has a plane)
    }
    double2* __restrict__ plane = reinterpret_cast<double2*>(a.plane + sg.plane0) + k0;
    const int64_t W = U + 1;                             // double2 per plane row

    double ev[P], od[P];
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
#pragma unroll
    for (int j = 0; j < P; ++j)
        if (k0 + j <= U) plane[j] = make_double2(ev[j], od[j]);
    for (int i = tid; i < 2 * (LATTICE_MAX_THREADS + 1); i += NT) (&xv[0][0])[i] = NEG;
    __syncthreads();
    xv[0][tid + 1] = od[P - 1];
    float qb[PF], ql[PF][P];
    double qs[PF];
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
        const double nb = xv[(t - 1) & 1][tid];
        const double lb = (double)yb - lt;
        double2* __restrict__ prow = plane + (int64_t)t * W;
#pragma unroll
        for (int j = P - 1; j >= 0; --j) {
            const double po = j ? od[j - 1] : nb;
            const double ne = lse2(ev[j], po);
            const double no = lse3(od[j], ev[j], (skipm >> j & 1u) ? po : NEG);
            const int k = k0 + j;
            od[j] = k < U ? no + ((double)yl[j] - lt) : NEG;
            ev[j] = k <= U ? ne + lb : NEG;
            if (k <= U) prow[j] = make_double2(ev[j], od[j]);
            if (P == 8) __builtin_amdgcn_sched_barrier(0);
        }
        xv[t & 1][tid + 1] = od[P - 1];
    };
    int t0 = 1;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            step(t0 + i, qb[i], ql[i], qs[i]);
            const int tt = min(t0 + i + PF, T - 1);
            const float* __restrict__ row = lg + (int64_t)tt * V;
            qb[i] = row[blank];
            qs[i] = ls[tt];
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (t0 + i < T) step(t0 + i, qb[i], ql[i], qs[i]);
    }
    if (tid == 0) fin[1] = NEG;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (k0 + j == U) fin[0] = ev[j];
        if (k0 + j + 1 == U) fin[1] = od[j];
    }
    __syncthreads();
    if (tid == 0) a.logp[sg.out] = U >= 1 ? lse2(fin[0], fin[1]) : fin[0];
}

// The beta sweep: frames T - 1 down to 0 on b_t(s) = beta_t(s) + lp_t(ext[s]); the plane's alpha_t(s) becomes gamma_t(s).
template <int P>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_grad_beta_kernel(GradArgs a, int pair0) {
    constexpr int PF = P == 8 ? 1 : P == 4 ? 4 : 8;
    constexpr double NEG = -__builtin_inf();
    __shared__ double xe[2][LATTICE_MAX_THREADS + 1];    // entry i = thread i's first even state; entry NT = "state S"
    __shared__ double xo[2][LATTICE_MAX_THREADS + 1];    // its first odd state

    const GradPair sg = a.pairs[pair0 + blockIdx.x];
    const double logp = a.logp[sg.out];                  // (the alpha sweep's, earlier on the stream)
    if (!(logp - logp == 0.0)) return;                   // -inf or NaN: no contribution, and no plane to touch (block-uniform)
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const double* __restrict__ ls = a.lse + sg.lse0;
    const int k0 = tid * P;
    double2* __restrict__ plane = reinterpret_cast<double2*>(a.plane + sg.plane0) + k0;
    const int64_t W = U + 1;

    // labels of the thread's pairs (all valid: logp is finite) and whether state 2k + 1 may skip to 2k + 3
    int lj[P];
    unsigned skipn = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = k0 + j;
        lj[j] = k < U ? lab[k] : blank;
        if (k + 1 < U && lab[k + 1] != lj[j]) skipn |= 1u << j;
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
            bo[j] = o_end ? (double)row[lj[j]] - lt : NEG;
            av[j] = make_double2(NEG, NEG);
            if (P != 8 && T >= 2 && k <= U) av[j] = (prow - W)[j];
        }
    }
    __syncthreads();
    xe[(T - 1) & 1][tid] = be[0];
    xo[(T - 1) & 1][tid] = bo[0];
    float qb[PF], ql[PF][P];                             // x_t(blank), x_t(l_k) of the next PF steps (frames T - 2, T - 3, ...)
    double qs[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int tt = max(T - 2 - i, 0);
        const float* __restrict__ row = lg + (int64_t)tt * V;
        qb[i] = row[blank];
        qs[i] = ls[tt];
#pragma unroll
        for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
    }
    auto step = [&](int t, float yb, const float* yl, double lt) {
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
            bo[j] = k < U ? bod + ((double)yl[j] - lt) : NEG;
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
            step(T - 2 - (i0 + i), qb[i], ql[i], qs[i]);
            const int tt = max(T - 2 - (i0 + i + PF), 0);
            const float* __restrict__ row = lg + (int64_t)tt * V;
            qb[i] = row[blank];
            qs[i] = ls[tt];
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (i0 + i < steps) step(T - 2 - (i0 + i), qb[i], ql[i], qs[i]);       // (block-uniform)
    }
}

constexpr int REDUCE_COLS = 256;
constexpr double FIX_SCALE = 2305843009213693952.0;      // 2^61

// one block per (frame, utterance, 256 vocabulary columns)
__global__ __launch_bounds__(REDUCE_COLS) void score_grad_reduce_kernel(GradArgs a) {
    __shared__ unsigned long long acc[REDUCE_COLS];
    __shared__ unsigned long long accb;
    const GradUtt u = a.utts[blockIdx.y];
    const int t = blockIdx.x;
    if (t >= u.T) return;
    const int tid = threadIdx.x, V = a.V, blank = a.blank;
    const int v0 = blockIdx.z * REDUCE_COLS, v = v0 + tid;
    double G = 0.0, csum = 0.0;
    bool any = false;
    for (int q = u.q0; q < u.q1; ++q) {
        const GradPair pr = a.pairs[a.by_utt[q]];
        const double lp = a.logp[pr.out];
        if (!(lp - lp == 0.0)) continue;                 // (block-uniform)
        const double c = a.coef[pr.out];
        acc[tid] = 0ull;
        if (tid == 0) accb = 0ull;
        __syncthreads();
        const double* __restrict__ row = a.plane + pr.plane0 + (int64_t)t * (2 * ((int64_t)pr.U + 1));
        const int32_t* __restrict__ lab = a.labels + pr.label0;
        const int S = 2 * pr.U + 1;
        unsigned long long bsum = 0ull;                  // even states: the blank's column, summed in registers
        for (int s = tid; s < S; s += REDUCE_COLS) {     // (the stride is even: a thread sees states of one parity)
            const unsigned long long fx = (unsigned long long)(row[s] * FIX_SCALE);
            if (s & 1) {
                const int l = lab[s >> 1] - v0;
                if (l >= 0 && l < REDUCE_COLS && fx) atomicAdd(&acc[l], fx);
            } else {
                bsum += fx;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bsum += __shfl_xor(bsum, off, 64);
        if ((tid & 63) == 0 && bsum) atomicAdd(&accb, bsum);
        __syncthreads();
        const double Gam = (double)(v == blank ? accb : acc[tid]) * (1.0 / FIX_SCALE);
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

inline int grad_pairs_per_thread(int U) { return pairs_per_thread(U + 1); }
inline int64_t plane_doubles(int T, int U) { return T >= U ? (int64_t)T * 2 * ((int64_t)U + 1) : 0; }

// the bytes of one pass over ng utterances with mg pairs, frames frames in all and planes fp64 of planes
inline int64_t group_bytes(int64_t ng, int64_t mg, int64_t frames, int64_t planes) {
    return (int64_t)(up256((size_t)ng * sizeof(GradUtt)) + up256((size_t)mg * sizeof(GradPair)) + up256((size_t)mg * sizeof(int32_t)) +
                     up256((size_t)frames * sizeof(double))) + planes * (int64_t)sizeof(double);
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

constexpr int64_t DEFAULT_CAP = (int64_t)8 << 30;
constexpr int MAX_GROUP_UTTS = 65535;                    // grid.y of the lse and reduce kernels

}  // namespace

int64_t ctc_score_grad_workspace(int n, const int32_t* frames, int m, const int32_t* utt_of, const int32_t* nlabels, int V) {
    if (int e = check_shapes("ctc_score_grad_workspace", V, n, frames, m, utt_of, nlabels)) return e;
    int64_t fr = 0, planes = 0;
    for (int i = 0; i < n; ++i) fr += frames[i];
    for (int j = 0; j < m; ++j) planes += plane_doubles(frames[utt_of[j]], nlabels[j]);
    return group_bytes(n, m, fr, planes);
}

int launch_ctc_score_grad(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                          const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, const double* coef,
                          double* logp, float* grad, int64_t max_workspace_bytes, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && utt_of && labels && label0 && nlabels && coef && logp && grad, "ctc_score_grad: null argument");
    if (int e = check_shapes("ctc_score_grad", V, n, frames, m, utt_of, nlabels)) return e;
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_score_grad: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(max_workspace_bytes >= 0, "ctc_score_grad: max_workspace_bytes %lld is negative (0: the default of 8 GiB)",
                 (long long)max_workspace_bytes);
    for (int i = 0; i < n; ++i) W2V2_REQUIRE(row0[i] >= 0, "ctc_score_grad: utterance %d has a negative offset", i);
    for (int j = 0; j < m; ++j) W2V2_REQUIRE(label0[j] >= 0, "ctc_score_grad: pair %d has a negative offset", j);
    const int64_t cap = max_workspace_bytes ? max_workspace_bytes : DEFAULT_CAP;

    // the pairs of each utterance, in the caller's order
    std::vector<int> first((size_t)n + 1, 0), of_utt((size_t)m);
    for (int j = 0; j < m; ++j) ++first[utt_of[j] + 1];
    for (int i = 0; i < n; ++i) first[i + 1] += first[i];
    {
        std::vector<int> fill(first.begin(), first.end() - 1);
        for (int j = 0; j < m; ++j) of_utt[fill[utt_of[j]]++] = j;
    }
    // consecutive utterances in groups that fit; a single utterance that does not fit fails the call before anything is allocated
    struct Group { int u0, u1; int64_t bytes; };
    std::vector<Group> groups;
    {
        int u0 = 0;
        int64_t fr = 0, planes = 0, mg = 0;
        for (int i = 0; i < n; ++i) {
            int64_t pl = 0;
            for (int q = first[i]; q < first[i + 1]; ++q) pl += plane_doubles(frames[i], nlabels[of_utt[q]]);
            const int64_t mi = first[i + 1] - first[i];
            const int64_t alone = group_bytes(1, mi, frames[i], pl);
            W2V2_REQUIRE(alone <= cap, "ctc_score_grad: utterance %d (%d frames, %lld pairs) needs %lld bytes of workspace; max_workspace_bytes is %lld",
                         i, frames[i], (long long)mi, (long long)alone, (long long)cap);
            if (i > u0 && (group_bytes(i - u0 + 1, mg + mi, fr + frames[i], planes + pl) > cap || i - u0 >= MAX_GROUP_UTTS)) {
                groups.push_back(Group{u0, i, group_bytes(i - u0, mg, fr, planes)});
                u0 = i;
                fr = planes = mg = 0;
            }
            fr += frames[i];
            planes += pl;
            mg += mi;
        }
        groups.push_back(Group{u0, n, group_bytes(n - u0, mg, fr, planes)});
    }
    int64_t need = 0;
    for (const Group& g : groups) need = std::max(need, g.bytes);
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_SCORE_GRAD, s, (size_t)need, &raw)) return e;

    ProfScope ps(nullptr, FAM_CTC, 0.0, 0.0, s);
    std::vector<GradUtt> utts;
    std::vector<GradPair> pairs;
    std::vector<int32_t> by_utt;
    std::vector<int> order, where;
    for (const Group& g : groups) {
        const int ng = g.u1 - g.u0, mg = first[g.u1] - first[g.u0];
        utts.assign((size_t)ng, GradUtt{});
        int64_t fr = 0;
        int Tmax = 0;
        for (int i = g.u0; i < g.u1; ++i) {
            utts[i - g.u0] = GradUtt{row0[i], fr, frames[i], first[i] - first[g.u0], first[i + 1] - first[g.u0], 0};
            fr += frames[i];
            Tmax = std::max(Tmax, (int)frames[i]);
        }
        if (mg == 0) {                                   // utterances without pairs: zero rows, from the reduce kernel alone
            by_utt.assign(1, 0);
            pairs.assign(1, GradPair{});
        } else {
            // q = position in (utterance, caller's index) order; sorted by (P, utterance, caller's index) for the sweeps
            order.resize((size_t)mg);
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
                return grad_pairs_per_thread(nlabels[of_utt[first[g.u0] + x]]) < grad_pairs_per_thread(nlabels[of_utt[first[g.u0] + y]]);
            });
            std::vector<int64_t> plane0((size_t)mg);
            int64_t pl = 0;
            for (int q = 0; q < mg; ++q) {
                const int j = of_utt[first[g.u0] + q];
                plane0[q] = pl;
                pl += plane_doubles(frames[utt_of[j]], nlabels[j]);
            }
            pairs.resize((size_t)mg);
            by_utt.resize((size_t)mg);
            for (int i = 0; i < mg; ++i) {
                const int q = order[i], j = of_utt[first[g.u0] + q];
                const GradUtt& u = utts[utt_of[j] - g.u0];
                pairs[i] = GradPair{u.row0, u.lse0, label0[j], plane0[q], u.T, nlabels[j], j, 0};
                by_utt[q] = i;
            }
        }
        const size_t utt_bytes = up256((size_t)ng * sizeof(GradUtt)), pair_bytes = up256((size_t)mg * sizeof(GradPair)),
                     idx_bytes = up256((size_t)mg * sizeof(int32_t)), lse_bytes = up256((size_t)fr * sizeof(double));
        char* base = static_cast<char*>(raw);
        GradArgs a;
        a.logits = logits;
        a.labels = labels;
        a.utts = reinterpret_cast<const GradUtt*>(base);
        a.pairs = reinterpret_cast<const GradPair*>(base + utt_bytes);
        a.by_utt = reinterpret_cast<const int32_t*>(base + utt_bytes + pair_bytes);
        a.lse = reinterpret_cast<double*>(base + utt_bytes + pair_bytes + idx_bytes);
        a.plane = reinterpret_cast<double*>(base + utt_bytes + pair_bytes + idx_bytes + lse_bytes);
        a.coef = coef;
        a.logp = logp;
        a.grad = grad;
        a.V = V;
        a.blank = blank;
        if (int e = staged_upload(SCRATCH_SCORE_GRAD, s, raw,
                                  {{utts.data(), (size_t)ng * sizeof(GradUtt), 0},
                                   {pairs.data(), (size_t)mg * sizeof(GradPair), utt_bytes},
                                   {by_utt.data(), (size_t)mg * sizeof(int32_t), utt_bytes + pair_bytes}},
                                  (size_t)64 << 10))
            return e;
        W2V2_LAUNCH(score_grad_lse_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)ng), dim3(256), 0, s, a);
        for (int i = 0; i < mg;) {
            const int P = grad_pairs_per_thread(pairs[i].U);
            int e = i, Umax = 0;
            for (; e < mg && grad_pairs_per_thread(pairs[e].U) == P; ++e) Umax = std::max(Umax, (int)pairs[e].U);
            const int nt = (((Umax + 1 + P - 1) / P + 63) / 64) * 64;
            dispatch_pairs(P, [&](auto p) {
                W2V2_LAUNCH(score_grad_alpha_kernel<decltype(p)::value>, dim3((unsigned)(e - i)), dim3((unsigned)nt), 0, s, a, i);
            });
            dispatch_pairs(P, [&](auto p) {
                W2V2_LAUNCH(score_grad_beta_kernel<decltype(p)::value>, dim3((unsigned)(e - i)), dim3((unsigned)nt), 0, s, a, i);
            });
            i = e;
        }
        W2V2_LAUNCH(score_grad_reduce_kernel, dim3((unsigned)Tmax, (unsigned)ng, (unsigned)((V + REDUCE_COLS - 1) / REDUCE_COLS)),
                    dim3(REDUCE_COLS), 0, s, a);
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
