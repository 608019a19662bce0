// CTC phrase search: where in a recording a label string is spoken, for m (recording, phrase) pairs at once (w2v2_ctc_spot;
// DESIGN.md §19).  A Viterbi recursion with a free begin and a free end whose score is the ratio to the frame-wise best path.
//
// Definition (tests/spot_reference.py implements exactly this in fp64 numpy).  The phrase is l_0 .. l_{U-1}, 1 <= U <= 256, no
// label the blank.  S = 2U - 1 states, ext[2k] = l_k, ext[2k + 1] = blank: no leading and no trailing blank state, a hit begins
// on a frame of its first label and ends on a frame of its last.  m_t = max_v x_t(v) (fp32); e_t(v) = (double)x_t(v) -
// (double)m_t <= 0, exactly 0 for the argmax: a path's score is ln P(path) - ln P(greedy path) over the same frames, the
// log-sum-exp cancels, and there is no exp and no log.  Every state carries a score d (fp64) and the begin frame b (int32) of
// the path that produced it; before frame 0 d = -inf, b = -1.  At frame t the candidates of state s, in this order, each
// compared with a strict > (compare-and-select, never fmax) against the best so far:
//   1. stay (d_{t-1}(s), b_{t-1}(s))   2. s >= 1: from s - 1   3. s >= 2, s even, ext[s] != ext[s-2]: from s - 2
//   4. s == 0: the fresh start (0.0, t)
// then d_t(s) = chosen + e_t(ext[s]) and b_t(s) = the chosen candidate's begin: ties keep the earlier begin.  The phrase ends
// at t with z_t = d_t(S-1), c_t = b_t(S-1).
// Recording edges (delim >= 0 and U >= 3): l_0 == delim: state 2 also gets the fresh start (0.0, 0) at t = 0, compared last;
// l_{U-1} == delim: at t = T - 1 d_t(S-2) and then d_t(S-3), with their begins, also compete for (z, c), each with strict >.
// Hits, one pass over t with thr = min_score: frame t is a candidate (z_t, c_t, t) when z_t >= thr and z_t > -inf; one current
// hit is kept; a candidate with c_t <= cur.end overlaps it and replaces it only if z_t > cur.score; one that does not overlap
// flushes the current hit to the output and becomes it; the current hit is flushed behind the last frame.
// Per pair, neighbours unaffected: a recording with a NaN logit, a +inf logit or a frame of -inf only, or a device label
// outside [0, V) or equal to the blank, gives count -1, empty hit slots and an empty trace (NaN / -1).  -inf logits are
// otherwise legal; T < U yields no hit.
//
// Arithmetic: per state and step one to three fp64 compare-selects and ONE fp64 add, in the order above; no multiply, so
// nothing contracts, and the trace and the hits are bit-identical to the numpy loop.
//
// Structure.  spot_max_kernel: one wave per frame, m_t of every RECORDING (not pair) into the workspace, NaN for a frame that
// makes its recording bad.  spot_kernel<P>: one WAVE per pair; it shares nothing, so there is no LDS, no barrier and no atomic.
// A lane owns P consecutive (label, blank) state pairs in registers (P = 1 up to 64 labels, 2 up to 128, 4 up to 256).  State
// 2k of a lane's first pair needs the previous lane's last two states: they arrive by the wave-wide DPP shift edit.hip uses
// (v_mov_b32 wave_shr:1, three dwords per value), and lane 0's feed IS the fresh start (0.0, t) in the place of "from s - 1":
// stay, then the fresh start, is state 0's candidate order.  A candidate that a state does not have is -inf, which a strict >
// never selects, so every state runs the same instruction sequence whatever P and whatever its neighbours.  The P + 2 fp32
// values of a step (the labels' logits, the blank's, m_t) are loaded PF steps ahead into a register ring, as align.hip does,
// all of them as vector loads (see vz below).
// The lane that owns state S - 1 runs the hit pass and writes hits and trace with plain vector stores.  The host orders the
// pairs by P and then longest recording first, so that a long one does not trail its launch.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <type_traits>
#include <vector>

namespace w2v2 {
namespace {

struct SpotUtt {
    int64_t row0;      // first logits row
    int64_t m0;        // first entry of the recording's frame maxima
    int32_t T, pad;
};

struct SpotPair {
    int64_t row0;      // first logits row of the pair's recording
    int64_t m0;        // first entry of its frame maxima
    int64_t label0;    // first label
    int64_t trace0;    // first entry of the pair's trace, -1: none
    double thr;        // min_score
    int32_t T, U;
    int32_t out, pad;  // index of the pair in the caller's order
};

struct SpotArgs {
    const float* logits;
    const int32_t* labels;
    const SpotUtt* utts;
    const SpotPair* pairs;      // sorted by (P, frames descending, caller's index)
    float* fmax;                // (sum T_i over the recordings): m_t, NaN for a bad frame
    double* hit_score;          // (m, max_hits)
    int32_t* hit_begin;
    int32_t* hit_end;
    int32_t* count;             // (m)
    double* trace_score;        // optional
    int32_t* trace_begin;
    int V, blank, delim, max_hits;
};

// m_t of frame t of recording blockIdx.y: one wave per frame, grid.x covers the longest recording
__global__ __launch_bounds__(256) void spot_max_kernel(SpotArgs a) {
    const SpotUtt u = a.utts[blockIdx.y];
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= u.T) return;
    const int lane = threadIdx.x & 63;
    const float* __restrict__ r = a.logits + (u.row0 + t) * a.V;
    float m = -INFINITY;
    bool bad = false;
    for (int v = lane; v < a.V; v += 64) {
        const float x = r[v];
        bad |= !(x < INFINITY);                          // NaN or +inf
        m = fmaxf(m, x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    bad = __any(bad) || !(m > -INFINITY);                // ... or a frame of -inf only
    if (lane == 0) a.fmax[u.m0 + t] = bad ? __builtin_nanf("") : m;
}

// lane l <- v of lane l - 1; lane 0 <- feed
__device__ __forceinline__ uint32_t lane_shr1(uint32_t feed, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)feed, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ double lane_shr1(double feed, double v) {
    const uint64_t f = (uint64_t)__double_as_longlong(feed), x = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = lane_shr1((uint32_t)f, (uint32_t)x), hi = lane_shr1((uint32_t)(f >> 32), (uint32_t)(x >> 32));
    return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
}

template <int P>
__global__ __launch_bounds__(64) void spot_kernel(SpotArgs a, int pair0) {
    constexpr int PF = P == 4 ? 4 : 8;                   // steps the logits are loaded ahead (registers)
    constexpr double NEG = -__builtin_inf();
    const SpotPair sp = a.pairs[pair0 + blockIdx.x];
    const int lane = threadIdx.x, T = sp.T, U = sp.U, V = a.V, blank = a.blank, H = a.max_hits;
    const float* __restrict__ lg = a.logits + sp.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sp.label0;
    const float* __restrict__ fm = a.fmax + sp.m0;
    double* __restrict__ hs = a.hit_score + (int64_t)sp.out * H;
    int32_t* __restrict__ hb = a.hit_begin + (int64_t)sp.out * H;
    int32_t* __restrict__ he = a.hit_end + (int64_t)sp.out * H;
    const bool tracing = sp.trace0 >= 0;
    double* __restrict__ tz = a.trace_score + (tracing ? sp.trace0 : 0);     // (never dereferenced without a trace)
    int32_t* __restrict__ tc = a.trace_begin + (tracing ? sp.trace0 : 0);
    const int k0 = lane * P;                             // this lane's label indices: k0 .. k0 + P - 1
    // a zero the compiler takes for a per-lane value: the blank's logit and m_t are the same address in every lane, and as
    // scalar loads they return out of order, so that waiting for the one a step needs waits for the one just issued for PF
    // steps ahead -- the whole memory latency in every step.  As vector loads they are counted in order, like the labels'.
    int vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));

    // the lane's labels (the blank's column past U: any column inside the row), the skip flags, the per-pair checks
    int lj[P];
    unsigned skipm = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = k0 + j;
        lj[j] = blank;
        if (k < U) {
            const int l = lab[k];
            const bool b = l < 0 || l >= V || l == blank;
            bad |= b;
            if (k >= 1 && l != lab[k - 1]) skipm |= 1u << j;
            lj[j] = b ? blank : l;                       // (never an address outside the row)
        }
    }
    for (int t = lane; t < T; t += 64) {
        const float v = fm[t];
        bad |= v != v;                                   // a bad frame of the recording
    }
    const int l_first = lab[0], l_last = lab[U - 1];     // (wave-uniform)
    if (__any(bad)) {
        for (int i = lane; i < H; i += 64) {
            hs[i] = __builtin_nan("");
            hb[i] = -1;
            he[i] = -1;
        }
        if (tracing) {
            for (int t = lane; t < T; t += 64) {
                tz[t] = __builtin_nan("");
                tc[t] = -1;
            }
        }
        if (lane == 0) a.count[sp.out] = -1;
        return;                                          // (wave-uniform)
    }
    const bool edges = a.delim >= 0 && U >= 3;
    const bool edge_first = edges && l_first == a.delim, edge_last = edges && l_last == a.delim;
    const int owner = (U - 1) / P;                       // the lane of state S - 1
    const bool mine = lane == owner;

    // frame 0 in closed form: every earlier value is -inf, so state 0 takes its fresh start (and state 2 the edge's) and every
    // other state stays at -inf
    double ev[P], od[P];                                 // d(2k), d(2k + 1) of the lane's pairs
    int bev[P], bod[P];                                  // their begins
    double zs = NEG, z2 = NEG, z3 = NEG;                 // d(S - 1) where the lane holds it; at the last frame d(S - 2), d(S - 3)
    int cs = -1, c2 = -1, c3 = -1;
    {
        const double m0 = (double)fm[0];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int k = k0 + j;
            const bool start = k == 0 || (k == 1 && edge_first);
            ev[j] = (start ? 0.0 : NEG) + ((double)lg[lj[j]] - m0);
            bev[j] = start ? 0 : -1;
            od[j] = NEG;
            bod[j] = -1;
            if (k == U - 1) {
                zs = ev[j];
                cs = bev[j];
            }
            if (k == U - 2) {
                z3 = ev[j];
                c3 = bev[j];
            }
        }
    }
    // the hit pass, in the lane that owns state S - 1 alone
    double cur_z = NEG;
    int cur_b = -1, cur_e = -1, nhit = 0;
    bool have = false;
    const double thr = sp.thr;
    auto flush = [&]() {
        if (mine && nhit < H) {
            hs[nhit] = cur_z;
            hb[nhit] = cur_b;
            he[nhit] = cur_e;
        }
        ++nhit;
    };
    auto emit = [&](int t, double z, int c) {
        if (tracing && mine) {
            tz[t] = z;
            tc[t] = c;
        }
        if (mine && z >= thr && z > NEG) {
            if (have && c <= cur_e) {
                if (z > cur_z) {
                    cur_z = z;
                    cur_b = c;
                    cur_e = t;
                }
            } else {
                if (have) flush();
                have = true;
                cur_z = z;
                cur_b = c;
                cur_e = t;
            }
        }
    };
    // one frame: yl the logits of the lane's labels, yb the blank's, ym the frame's maximum; fin: the last frame, which also
    // keeps the two states below the last.  (The values are picked as they are formed: a pick out of the arrays behind the
    // step would index them by a run-time number and move them out of the registers.)
    auto step = [&](int t, const float* yl, float yb, float ym, auto fin) {
        const double mt = (double)ym;
        // the previous lane's last pair, before anything of this step is written; lane 0: the fresh start in the place of
        // "from s - 1", and no "from s - 2"
        const double po0 = lane_shr1(0.0, od[P - 1]);
        const double pe0 = lane_shr1(NEG, ev[P - 1]);
        const int pbo0 = (int)lane_shr1((uint32_t)t, (uint32_t)bod[P - 1]);
        const int pbe0 = (int)lane_shr1((uint32_t)-1, (uint32_t)bev[P - 1]);
        const double eb = (double)yb - mt;
#pragma unroll
        for (int j = P - 1; j >= 0; --j) {               // downwards: pair j - 1 still holds the previous frame's values
            const double po = j ? od[j - 1] : po0, pe = j ? ev[j - 1] : pe0;
            const int pbo = j ? bod[j - 1] : pbo0, pbe = j ? bev[j - 1] : pbe0;
            // state 2k + 1 (blank): stay, then from 2k
            double d1 = od[j];
            int b1 = bod[j];
            if (ev[j] > d1) {
                d1 = ev[j];
                b1 = bev[j];
            }
            // state 2k (label): stay, from 2k - 1, from 2k - 2 where the labels differ
            double d0 = ev[j];
            int b0 = bev[j];
            if (po > d0) {
                d0 = po;
                b0 = pbo;
            }
            const double sk = (skipm >> j & 1u) ? pe : NEG;
            if (sk > d0) {
                d0 = sk;
                b0 = pbe;
            }
            d1 += eb;
            d0 += (double)yl[j] - mt;
            od[j] = d1;
            bod[j] = b1;
            ev[j] = d0;
            bev[j] = b0;
            if (P == 1 || k0 + j == U - 1) {             // (P == 1: every lane keeps its own; the owner's is the phrase's)
                zs = d0;
                cs = b0;
            }
            if (decltype(fin)::value && k0 + j == U - 2) {
                z2 = d1;
                c2 = b1;
                z3 = d0;
                c3 = b0;
            }
        }
    };
    const std::false_type inner;

    if (T > 1) {
        emit(0, zs, cs);
        const int last = T - 1;                          // the last frame is stepped behind the loop: the edge rule
        float ql[PF][P], qb[PF], qm[PF];                 // x_t(l_k), x_t(blank), m_t of the next PF frames
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int tt = min(1 + i, last);
            const float* __restrict__ row = lg + (int64_t)tt * V;
            qb[i] = row[blank + vz];
            qm[i] = fm[tt + vz];
#pragma unroll
            for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
        }
        int t0 = 1;
        for (; t0 + PF <= last; t0 += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                step(t0 + i, ql[i], qb[i], qm[i], inner);
                emit(t0 + i, zs, cs);
                const int tt = min(t0 + i + PF, last);   // (wave-uniform row, per-lane column)
                const float* __restrict__ row = lg + (int64_t)tt * V;
                qb[i] = row[blank + vz];
                qm[i] = fm[tt + vz];
#pragma unroll
                for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
            }
        }
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            if (t0 + i < last) {                         // (wave-uniform)
                step(t0 + i, ql[i], qb[i], qm[i], inner);
                emit(t0 + i, zs, cs);
            }
        }
        {
            const float* __restrict__ row = lg + (int64_t)last * V;
            float yl[P];
#pragma unroll
            for (int j = 0; j < P; ++j) yl[j] = row[lj[j]];
            step(last, yl, row[blank + vz], fm[last + vz], std::true_type());
        }
    }
    // the last frame: the phrase may end a state or two early where its last label is the recording's edge
    double z = zs;
    int c = cs;
    if (edge_last) {                                     // (wave-uniform; U >= 3)
        const int src = (U - 2) / P;
        z2 = __shfl(z2, src, 64);
        z3 = __shfl(z3, src, 64);
        c2 = __shfl(c2, src, 64);
        c3 = __shfl(c3, src, 64);
        if (z2 > z) {
            z = z2;
            c = c2;
        }
        if (z3 > z) {
            z = z3;
            c = c3;
        }
    }
    emit(T - 1, z, c);
    if (have) flush();
    // behind the stored hits, and the count (the owner's)
    const int n = __shfl(nhit, owner, 64);
    for (int i = min(n, H) + lane; i < H; i += 64) {
        hs[i] = __builtin_nan("");
        hb[i] = -1;
        he[i] = -1;
    }
    if (mine) a.count[sp.out] = n;
}

inline int spot_pairs_per_lane(int U) { return U <= 64 ? 1 : U <= 128 ? 2 : 4; }

}  // namespace

int launch_ctc_spot(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int m, const int32_t* utt_of,
                    const int32_t* labels, const int64_t* label0, const int32_t* nlabels, int blank, int delim,
                    const double* min_score, int max_hits, double* hit_score, int32_t* hit_begin, int32_t* hit_end, int32_t* count,
                    double* trace_score, int32_t* trace_begin, const int64_t* trace0, hipStream_t s) {
    W2V2_REQUIRE(logits && row0 && frames && utt_of && labels && label0 && nlabels && min_score && hit_score && hit_begin && hit_end &&
                     count,
                 "ctc_spot: null argument");
    W2V2_REQUIRE((trace_score != nullptr) == (trace_begin != nullptr), "ctc_spot: one trace pointer without the other");
    W2V2_REQUIRE(!trace_score || trace0, "ctc_spot: null argument (trace pointers without trace offsets)");
    W2V2_REQUIRE(n >= 1, "ctc_spot: %d recordings (need at least one)", n);
    W2V2_REQUIRE(m >= 1, "ctc_spot: %d pairs (need at least one)", m);
    W2V2_REQUIRE(max_hits >= 1, "ctc_spot: max_hits %d (need at least one slot)", max_hits);
    W2V2_REQUIRE(V >= 2, "ctc_spot: vocabulary of %d entries (need the blank and a label)", V);
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_spot: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(delim == -1 || (delim >= 0 && delim < V && delim != blank),
                 "ctc_spot: delimiter %d is neither -1 nor a label of vocabulary %d other than the blank", delim, V);
    int Tmax = 0;
    std::vector<SpotUtt> utts((size_t)n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(frames[i] >= 1, "ctc_spot: recording %d has %d frames (need at least one)", i, frames[i]);
        W2V2_REQUIRE(row0[i] >= 0, "ctc_spot: recording %d has a negative offset", i);
        utts[i] = SpotUtt{row0[i], total, frames[i], 0};
        total += frames[i];
        Tmax = std::max(Tmax, (int)frames[i]);
    }
    double work = 0.0;
    for (int j = 0; j < m; ++j) {
        W2V2_REQUIRE(utt_of[j] >= 0 && utt_of[j] < n, "ctc_spot: pair %d searches recording %d of %d", j, utt_of[j], n);
        W2V2_REQUIRE(label0[j] >= 0, "ctc_spot: pair %d has a negative offset", j);
        W2V2_REQUIRE(nlabels[j] >= 1 && nlabels[j] <= W2V2_SPOT_MAX_LABELS, "ctc_spot: pair %d has %d labels; 1 to %d per pair", j,
                     nlabels[j], W2V2_SPOT_MAX_LABELS);
        W2V2_REQUIRE(!std::isnan(min_score[j]), "ctc_spot: pair %d has a NaN min_score", j);
        W2V2_REQUIRE(!trace_score || trace0[j] >= -1, "ctc_spot: pair %d has a negative trace offset (-1 means none)", j);
        work += (double)frames[utt_of[j]] * (2.0 * nlabels[j] - 1.0);
    }
    // the pairs by (pairs per lane, frames descending, caller's index): one grid per P, the long recordings first
    std::vector<int> order((size_t)m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const int px = spot_pairs_per_lane(nlabels[x]), py = spot_pairs_per_lane(nlabels[y]);
        return px != py ? px < py : frames[utt_of[x]] > frames[utt_of[y]];
    });
    std::vector<SpotPair> pairs((size_t)m);
    for (int i = 0; i < m; ++i) {
        const int j = order[i];
        const SpotUtt& u = utts[utt_of[j]];
        pairs[i] = SpotPair{u.row0, u.m0, label0[j], trace_score ? trace0[j] : -1, min_score[j], u.T, nlabels[j], j, 0};
    }
    // workspace: the recording table | the pair table | m_t (fp32, sum T_i)
    const size_t utt_bytes = up256((size_t)n * sizeof(SpotUtt)), pair_bytes = up256((size_t)m * sizeof(SpotPair));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_SPOT, s, utt_bytes + pair_bytes + (size_t)total * sizeof(float), &raw)) return e;
    SpotArgs a;
    a.logits = logits;
    a.labels = labels;
    a.utts = static_cast<const SpotUtt*>(raw);
    a.pairs = reinterpret_cast<const SpotPair*>(static_cast<char*>(raw) + utt_bytes);
    a.fmax = reinterpret_cast<float*>(static_cast<char*>(raw) + utt_bytes + pair_bytes);
    a.hit_score = hit_score;
    a.hit_begin = hit_begin;
    a.hit_end = hit_end;
    a.count = count;
    a.trace_score = trace_score;
    a.trace_begin = trace_begin;
    a.V = V;
    a.blank = blank;
    a.delim = delim;
    a.max_hits = max_hits;
    if (int e = staged_upload(SCRATCH_SPOT, s, raw,
                              {{utts.data(), (size_t)n * sizeof(SpotUtt), 0}, {pairs.data(), (size_t)m * sizeof(SpotPair), utt_bytes}},
                              (size_t)64 << 10))
        return e;
    // (work for the profile: three compare-selects and an add per state and step; the logits read once by the max pass)
    ProfScope ps(nullptr, FAM_CTC, 4.0 * work, 4.0 * (double)total * V, s);
    W2V2_LAUNCH(spot_max_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
    for (int i = 0; i < m;) {
        const int P = spot_pairs_per_lane(pairs[i].U);
        int e = i;
        for (; e < m && spot_pairs_per_lane(pairs[e].U) == P; ++e) {}
        if (P == 1) W2V2_LAUNCH(spot_kernel<1>, dim3((unsigned)(e - i)), dim3(64), 0, s, a, i);
        else if (P == 2) W2V2_LAUNCH(spot_kernel<2>, dim3((unsigned)(e - i)), dim3(64), 0, s, a, i);
        else W2V2_LAUNCH(spot_kernel<4>, dim3((unsigned)(e - i)), dim3(64), 0, s, a, i);
        i = e;
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
