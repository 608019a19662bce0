// Exact CTC scoring and its gradient with a star, the wildcard label of the aligners (w2v2_ctc_score_star,
// w2v2_ctc_score_grad_star): the score of a partial transcript summed over ALL frame paths, and the gradient of a
// weighted sum of such scores.  score.hip and score_grad.hip are not touched; the kernels here are copies with the star added.
//
// Definition (tests/score_star_reference.py implements exactly this in fp64 numpy).  Everything is score.hip's (alpha, logp) and
// score_grad.hip's (beta, gamma, Gamma, G) except the following.
//   The star label.  Label id V is the star, "as if the logits had one more column": the aligner's definition (align.hip).
//   Its emission.  lp_t(V) = ((double)m_t + (double)star_score) - lse_t.  m_t is the fp32 frame maximum of frame_lse_max
//   (ctc_lattice.h), blank included, NaN ignored; star_score <= 0 is an fp32 argument in nats per frame; lse_t is over the V real
//   columns only.
//   The recursion.  ext[2k + 1] = V is a state like any other.  The skip rule and R treat V like any id, so a star takes at least
//   one frame, and T < U + R gives -inf.  A label < 0, > V or equal to the blank gives NaN.  An utterance with a non-finite lse_t
//   gives NaN.
//   The value.  With a star, logp is a score of a set of paths, not a log-probability: the star's column is not part of the
//   softmax.  It may exceed 0.  It is never below the aligner's path score for the same input (a sum of non-negative terms that
//   holds the aligner's maximum).
//   The gradient.  a_t is the lowest column index with x_t(a_t) == m_t.  Then d lp_t(V) / d x_t(v) = [v = a_t] - y_t(v): the star
//   state emits the frame's top token.  Gamma_j(t, v) sums gamma over the states with ext[s] = v; for v = a_t it also sums the star
//   states.  G = sum_j c_j Gamma_j - (sum_j c_j) y is unchanged, and sum_s gamma_t(s) = 1 still holds, so the 2^-61 fixed-point
//   reduce keeps its overflow argument.
// What a loss built on this does on star frames: in proportion to the star's occupancy it sharpens the model's own top token; it
// does not supervise which token.
//
// Structure.  score_star_lse_kernel: one wave per frame; lse_t (frame_lse's bits), xs_t = m_t + star_score (fp64) and a_t (int32)
// of every utterance into the workspace (frame_lse_max_arg, ctc_lattice.h).  score_star_alpha_kernel<P, PLANE>: score_alpha_kernel<P>
// (PLANE = false) and score_grad_alpha_kernel<P> (PLANE = true: every step's states stored to the pair's plane) with align.hip's
// star scheme: a per-thread bit mask of the pairs that hold the star; xs_t loaded PF steps ahead like the blank's emission (one
// block-uniform fp64 per step); an odd state adds xs_t - lse_t where the mask is set and x_t(l_k) - lse_t otherwise; a star pair's
// per-lane logits load reads the blank's column and is discarded, so no address leaves the row.  score_star_beta_kernel<P>:
// score_grad_beta_kernel<P> with the same mask.  score_star_reduce_kernel: score_grad_reduce_kernel; a star state's gamma is summed
// in registers like the blank's, lands with one integer add per wave, and is added -- as an integer, before the one conversion to
// fp64 -- to column a_t.  No float atomics anywhere.  A state's value is the same sequence of fp64 operations as in score.hip and
// score_grad.hip, so a pair without a star carries the bits of w2v2_ctc_score / w2v2_ctc_score_grad, in a call of its own or mixed
// with star pairs (the tests pin that), and grouping under max_workspace_bytes changes no bit.
//
// Workspace of the gradient: tables | lse (fp64 per frame) | xs (fp64 per frame) | a (int32 per frame) | per pair T (2U + 2) fp64.
#include "ctc_lattice.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace w2v2 {
namespace {

struct StarUtt {
    int64_t row0;      // first logits / gradient row
    int64_t lse0;      // first entry of the utterance's lse, xs and a
    int32_t T;
    int32_t q0, q1;    // its pairs: by_utt[q0 .. q1), in the caller's order (gradient only)
    int32_t pad;
};

struct StarPair {
    int64_t row0;      // first logits row of the pair's utterance
    int64_t lse0;      // first entry of its lse, xs and a
    int64_t label0;    // first label
    int64_t plane0;    // first fp64 of its plane, T rows of 2 (U + 1) (gradient only; none when T < U)
    int32_t T, U;
    int32_t out, pad;  // index of the pair in the caller's order
};

struct StarArgs {
    const float* logits;
    const int32_t* labels;
    const StarUtt* utts;
    const StarPair* pairs;      // sorted by (P, utterance, caller's index)
    const int32_t* by_utt;      // indices into pairs, sorted by (utterance, caller's index) (gradient only)
    double* lse;
    double* xs;                 // the star's raw emission m_t + star_score, indexed like lse
    int32_t* amax;              // a_t, indexed like lse (gradient only: null for the scorer)
    double* plane;
    const double* coef;
    double* logp;
    float* grad;
    int V, blank;
    float star_score;
};

// lse_t, xs_t and (gradient) a_t of frame t of utterance blockIdx.y
__global__ __launch_bounds__(256) void score_star_lse_kernel(StarArgs a) {
    const StarUtt u = a.utts[blockIdx.y];
    float m;
    int am;
    const int t = frame_lse_max_arg(a.logits, a.V, u.row0, u.T, a.lse + u.lse0, m, am);
    if (t >= 0 && (threadIdx.x & 63) == 0) {
        a.xs[u.lse0 + t] = (double)m + (double)a.star_score;
        if (a.amax) a.amax[u.lse0 + t] = min(am, a.V - 1);          // (V: a frame of NaN only, whose utterance contributes nothing)
    }
}

// score_alpha_kernel<P> (PLANE = false) / score_grad_alpha_kernel<P> (PLANE = true), state for state, with the star
template <int P, bool PLANE>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_star_alpha_kernel(StarArgs a, int pair0) {
    constexpr int PF = P == 8 ? 1 : P == 4 ? 4 : 8;      // steps the emissions are loaded ahead (registers)
    constexpr double NEG = -__builtin_inf();
    __shared__ double xv[2][LATTICE_MAX_THREADS + 1];    // exchange: entry i + 1 = thread i's last odd state; entry 0 = "state -1"
    __shared__ int red[LATTICE_MAX_THREADS / 64];
    __shared__ double fin[2];

    const StarPair sg = a.pairs[pair0 + blockIdx.x];
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const double* __restrict__ ls = a.lse + sg.lse0;
    const double* __restrict__ xsr = a.xs + sg.lse0;
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
            bad |= l < 0 || l > V || l == blank;
            if (k >= 1 && l != lab[k - 1]) skipm |= 1u << j;
            if (l == V) starm |= 1u << j;
            lj[j] = (bad || l == V) ? blank : l;         // (never an address outside the row: a star pair loads the blank's column)
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
        qx[i] = xsr[tt];
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
            od[j] = k < U ? no + (((starm >> j & 1u) ? ys : (double)yl[j]) - lt) : NEG;
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
            qx[i] = xsr[tt];
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

// score_grad_beta_kernel<P> with the star: frames T - 1 down to 0 on b_t(s) = beta_t(s) + lp_t(ext[s]); the plane's alpha_t(s)
// becomes gamma_t(s)
template <int P>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void score_star_beta_kernel(StarArgs a, int pair0) {
    constexpr int PF = P == 8 ? 1 : P == 4 ? 4 : 8;
    constexpr double NEG = -__builtin_inf();
    __shared__ double xe[2][LATTICE_MAX_THREADS + 1];    // entry i = thread i's first even state; entry NT = "state S"
    __shared__ double xo[2][LATTICE_MAX_THREADS + 1];    // its first odd state

    const StarPair sg = a.pairs[pair0 + blockIdx.x];
    const double logp = a.logp[sg.out];                  // (the alpha sweep's, earlier on the stream)
    if (!(logp - logp == 0.0)) return;                   // -inf or NaN: no contribution, and no plane to touch (block-uniform)
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const double* __restrict__ ls = a.lse + sg.lse0;
    const double* __restrict__ xsr = a.xs + sg.lse0;
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
        if (l == V) starm |= 1u << j;
        lj[j] = l == V ? blank : l;                      // (a star pair loads the blank's column and discards it)
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
        const double ys = xsr[T - 1];
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
        qx[i] = xsr[tt];
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
            bo[j] = k < U ? bod + (((starm >> j & 1u) ? ys : (double)yl[j]) - lt) : NEG;
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
            qx[i] = xsr[tt];
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
__global__ __launch_bounds__(REDUCE_COLS) void score_star_reduce_kernel(StarArgs a) {
    __shared__ unsigned long long acc[REDUCE_COLS];
    __shared__ unsigned long long accb, accs;
    const StarUtt u = a.utts[blockIdx.y];
    const int t = blockIdx.x;
    if (t >= u.T) return;
    const int tid = threadIdx.x, V = a.V, blank = a.blank;
    const int v0 = blockIdx.z * REDUCE_COLS, v = v0 + tid;
    const int am = a.amax[u.lse0 + t];                   // a_t: the column the star states' gamma goes to (block-uniform)
    double G = 0.0, csum = 0.0;
    bool any = false;
    for (int q = u.q0; q < u.q1; ++q) {
        const StarPair pr = a.pairs[a.by_utt[q]];
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
                if (lv == V) ssum += fx;
                else if (l >= 0 && l < REDUCE_COLS && fx) atomicAdd(&acc[l], fx);
            } else {
                bsum += fx;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bsum += __shfl_xor(bsum, off, 64);
            ssum += __shfl_xor(ssum, off, 64);
        }
        if ((tid & 63) == 0 && bsum) atomicAdd(&accb, bsum);
        if ((tid & 63) == 0 && ssum) atomicAdd(&accs, ssum);
        __syncthreads();
        // (integer sum before the one conversion: without a star accs is 0 and the bits are score_grad_reduce_kernel's)
        const unsigned long long fx = (v == blank ? accb : acc[tid]) + (v == am ? accs : 0ull);
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

inline int star_pairs_per_thread(int U) { return pairs_per_thread(U + 1); }
inline int64_t plane_doubles(int T, int U) { return T >= U ? (int64_t)T * 2 * ((int64_t)U + 1) : 0; }

// the bytes of one gradient pass over ng utterances with mg pairs, frames frames in all and planes fp64 of planes
inline int64_t group_bytes(int64_t ng, int64_t mg, int64_t frames, int64_t planes) {
    return (int64_t)(up256((size_t)ng * sizeof(StarUtt)) + up256((size_t)mg * sizeof(StarPair)) + up256((size_t)mg * sizeof(int32_t)) +
                     2 * up256((size_t)frames * sizeof(double)) + up256((size_t)frames * sizeof(int32_t))) +
           planes * (int64_t)sizeof(double);
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

int launch_ctc_score_star(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                          const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, float star_score,
                          double* logp, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && utt_of && labels && label0 && nlabels && logp, "ctc_score_star: null argument");
    if (int e = check_shapes("ctc_score_star", V, n, frames, m, utt_of, nlabels)) return e;
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_score_star: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(star_score <= 0.f, "ctc_score_star: star_score %g (a log-domain penalty per frame: <= 0, not NaN)", (double)star_score);
    for (int i = 0; i < n; ++i) W2V2_REQUIRE(row0[i] >= 0, "ctc_score_star: utterance %d has a negative offset", i);
    for (int j = 0; j < m; ++j) W2V2_REQUIRE(label0[j] >= 0, "ctc_score_star: pair %d has a negative offset", j);
    int Tmax = 0;
    std::vector<StarUtt> utts((size_t)n);
    int64_t out = 0;
    for (int i = 0; i < n; ++i) {
        utts[i] = StarUtt{row0[i], out, frames[i], 0, 0, 0};
        out += frames[i];
        Tmax = std::max(Tmax, (int)frames[i]);
    }
    double work = 0.0;
    for (int j = 0; j < m; ++j) work += (double)frames[utt_of[j]] * (2.0 * nlabels[j] + 1.0);
    // the pairs by (pairs per thread, utterance, caller's index): one grid per P, an utterance's hypotheses adjacent
    std::vector<int> order((size_t)m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const int px = star_pairs_per_thread(nlabels[x]), py = star_pairs_per_thread(nlabels[y]);
        return px != py ? px < py : utt_of[x] < utt_of[y];
    });
    std::vector<StarPair> pairs((size_t)m);
    for (int i = 0; i < m; ++i) {
        const int j = order[i];
        const StarUtt& u = utts[utt_of[j]];
        pairs[i] = StarPair{u.row0, u.lse0, label0[j], 0, u.T, nlabels[j], j, 0};
    }
    // workspace: the utterance table | the pair table | lse (fp64, sum T_i) | xs (the same)
    const size_t utt_bytes = up256((size_t)n * sizeof(StarUtt)), pair_bytes = up256((size_t)m * sizeof(StarPair)),
                 lse_bytes = up256((size_t)out * sizeof(double));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_SCORE_STAR, s, utt_bytes + pair_bytes + 2 * lse_bytes, &raw)) return e;
    char* base = static_cast<char*>(raw);
    StarArgs a{};
    a.logits = logits;
    a.labels = labels;
    a.utts = reinterpret_cast<const StarUtt*>(base);
    a.pairs = reinterpret_cast<const StarPair*>(base + utt_bytes);
    a.lse = reinterpret_cast<double*>(base + utt_bytes + pair_bytes);
    a.xs = reinterpret_cast<double*>(base + utt_bytes + pair_bytes + lse_bytes);
    a.logp = logp;
    a.V = V;
    a.blank = blank;
    a.star_score = star_score;
    if (int e = staged_upload(SCRATCH_SCORE_STAR, s, raw,
                              {{utts.data(), (size_t)n * sizeof(StarUtt), 0}, {pairs.data(), (size_t)m * sizeof(StarPair), utt_bytes}},
                              (size_t)64 << 10))
        return e;
    ProfScope ps(nullptr, FAM_CTC, 100.0 * work, 4.0 * (double)out * V, s);
    W2V2_LAUNCH(score_star_lse_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
    for (int i = 0; i < m;) {
        const int P = star_pairs_per_thread(pairs[i].U);
        int e = i, Umax = 0;
        for (; e < m && star_pairs_per_thread(pairs[e].U) == P; ++e) Umax = std::max(Umax, (int)pairs[e].U);
        const int nt = (((Umax + 1 + P - 1) / P + 63) / 64) * 64;
        dispatch_pairs(P, [&](auto p) {
            W2V2_LAUNCH((score_star_alpha_kernel<decltype(p)::value, false>), dim3((unsigned)(e - i)), dim3((unsigned)nt), 0, s, a, i);
        });
        i = e;
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

int64_t ctc_score_grad_star_workspace(int n, const int32_t* frames, int m, const int32_t* utt_of, const int32_t* nlabels, int V) {
    if (int e = check_shapes("ctc_score_grad_star_workspace", V, n, frames, m, utt_of, nlabels)) return e;
    int64_t fr = 0, planes = 0;
    for (int i = 0; i < n; ++i) fr += frames[i];
    for (int j = 0; j < m; ++j) planes += plane_doubles(frames[utt_of[j]], nlabels[j]);
    return group_bytes(n, m, fr, planes);
}

int launch_ctc_score_grad_star(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m,
                               const int32_t* utt_of, const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank,
                               float star_score, const double* coef, double* logp, float* grad, int64_t max_workspace_bytes,
                               hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && utt_of && labels && label0 && nlabels && coef && logp && grad,
                 "ctc_score_grad_star: null argument");
    if (int e = check_shapes("ctc_score_grad_star", V, n, frames, m, utt_of, nlabels)) return e;
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_score_grad_star: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(star_score <= 0.f, "ctc_score_grad_star: star_score %g (a log-domain penalty per frame: <= 0, not NaN)",
                 (double)star_score);
    W2V2_REQUIRE(max_workspace_bytes >= 0, "ctc_score_grad_star: max_workspace_bytes %lld is negative (0: the default of 8 GiB)",
                 (long long)max_workspace_bytes);
    for (int i = 0; i < n; ++i) W2V2_REQUIRE(row0[i] >= 0, "ctc_score_grad_star: utterance %d has a negative offset", i);
    for (int j = 0; j < m; ++j) W2V2_REQUIRE(label0[j] >= 0, "ctc_score_grad_star: pair %d has a negative offset", j);
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
            W2V2_REQUIRE(alone <= cap, "ctc_score_grad_star: utterance %d (%d frames, %lld pairs) needs %lld bytes of workspace; max_workspace_bytes is %lld",
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
    if (int e = stream_scratch(SCRATCH_SCORE_GRAD_STAR, s, (size_t)need, &raw)) return e;

    ProfScope ps(nullptr, FAM_CTC, 0.0, 0.0, s);
    std::vector<StarUtt> utts;
    std::vector<StarPair> pairs;
    std::vector<int32_t> by_utt;
    std::vector<int> order;
    for (const Group& g : groups) {
        const int ng = g.u1 - g.u0, mg = first[g.u1] - first[g.u0];
        utts.assign((size_t)ng, StarUtt{});
        int64_t fr = 0;
        int Tmax = 0;
        for (int i = g.u0; i < g.u1; ++i) {
            utts[i - g.u0] = StarUtt{row0[i], fr, frames[i], first[i] - first[g.u0], first[i + 1] - first[g.u0], 0};
            fr += frames[i];
            Tmax = std::max(Tmax, (int)frames[i]);
        }
        if (mg == 0) {                                   // utterances without pairs: zero rows, from the reduce kernel alone
            by_utt.assign(1, 0);
            pairs.assign(1, StarPair{});
        } else {
            // q = position in (utterance, caller's index) order; sorted by (P, utterance, caller's index) for the sweeps
            order.resize((size_t)mg);
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
                return star_pairs_per_thread(nlabels[of_utt[first[g.u0] + x]]) < star_pairs_per_thread(nlabels[of_utt[first[g.u0] + y]]);
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
                const StarUtt& u = utts[utt_of[j] - g.u0];
                pairs[i] = StarPair{u.row0, u.lse0, label0[j], plane0[q], u.T, nlabels[j], j, 0};
                by_utt[q] = i;
            }
        }
        const size_t utt_bytes = up256((size_t)ng * sizeof(StarUtt)), pair_bytes = up256((size_t)mg * sizeof(StarPair)),
                     idx_bytes = up256((size_t)mg * sizeof(int32_t)), lse_bytes = up256((size_t)fr * sizeof(double)),
                     arg_bytes = up256((size_t)fr * sizeof(int32_t));
        char* base = static_cast<char*>(raw);
        StarArgs a{};
        a.logits = logits;
        a.labels = labels;
        a.utts = reinterpret_cast<const StarUtt*>(base);
        a.pairs = reinterpret_cast<const StarPair*>(base + utt_bytes);
        a.by_utt = reinterpret_cast<const int32_t*>(base + utt_bytes + pair_bytes);
        a.lse = reinterpret_cast<double*>(base + utt_bytes + pair_bytes + idx_bytes);
        a.xs = reinterpret_cast<double*>(base + utt_bytes + pair_bytes + idx_bytes + lse_bytes);
        a.amax = reinterpret_cast<int32_t*>(base + utt_bytes + pair_bytes + idx_bytes + 2 * lse_bytes);
        a.plane = reinterpret_cast<double*>(base + utt_bytes + pair_bytes + idx_bytes + 2 * lse_bytes + arg_bytes);
        a.coef = coef;
        a.logp = logp;
        a.grad = grad;
        a.V = V;
        a.blank = blank;
        a.star_score = star_score;
        if (int e = staged_upload(SCRATCH_SCORE_GRAD_STAR, s, raw,
                                  {{utts.data(), (size_t)ng * sizeof(StarUtt), 0},
                                   {pairs.data(), (size_t)mg * sizeof(StarPair), utt_bytes},
                                   {by_utt.data(), (size_t)mg * sizeof(int32_t), utt_bytes + pair_bytes}},
                                  (size_t)64 << 10))
            return e;
        W2V2_LAUNCH(score_star_lse_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)ng), dim3(256), 0, s, a);
        for (int i = 0; i < mg;) {
            const int P = star_pairs_per_thread(pairs[i].U);
            int e = i, Umax = 0;
            for (; e < mg && star_pairs_per_thread(pairs[e].U) == P; ++e) Umax = std::max(Umax, (int)pairs[e].U);
            const int nt = (((Umax + 1 + P - 1) / P + 63) / 64) * 64;
            dispatch_pairs(P, [&](auto p) {
                W2V2_LAUNCH((score_star_alpha_kernel<decltype(p)::value, true>), dim3((unsigned)(e - i)), dim3((unsigned)nt), 0, s, a, i);
            });
            dispatch_pairs(P, [&](auto p) {
                W2V2_LAUNCH(score_star_beta_kernel<decltype(p)::value>, dim3((unsigned)(e - i)), dim3((unsigned)nt), 0, s, a, i);
            });
            i = e;
        }
        W2V2_LAUNCH(score_star_reduce_kernel, dim3((unsigned)Tmax, (unsigned)ng, (unsigned)((V + REDUCE_COLS - 1) / REDUCE_COLS)),
                    dim3(REDUCE_COLS), 0, s, a);
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
