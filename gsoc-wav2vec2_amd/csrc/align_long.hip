// CTC forced alignment of whole recordings: the Viterbi path of align.hip with the (frame, state) plane cut into tiles, so that the
// label count is bounded by memory and not by one block's registers (w2v2_ctc_align_long).
//
// Definition: exactly the one in the header of align.hip (tests/align_reference.py restates it) -- the fp64 compare-select in the
// order stay / advance / skip, the end-state rule, frame_logp, score = delta_end - sum_t lse_t with the sum lane-strided by 64 and
// then the butterfly, the -inf utterance (T < U + R) and the NaN utterance (a bad label) with their -1 rows.  Tiling changes no
// operation and no order, so every output, the score's bits included, equals w2v2_ctc_align's wherever that one accepts the input.
//
// Tiling.  States come in pairs (blank 2k, label 2k + 1); a recording has U + 1 pairs.  A STRIP is `sp` consecutive pairs: one
// block's share, sp / P threads with P pairs each (P = pairs_per_thread(sp); the block is rounded up to whole
// waves, the spare threads hold no state and store nothing).  A PANEL is `pf` consecutive steps (step t reads frame t - 1 and writes
// frame t; panel p holds steps 1 + p pf ...).  Tile (p, q) runs align.hip's per-step recursion over panel p for strip q.  It needs
// from outside only
//   - its own states at the frame before the panel: the CARRY ROW, one fp64 per state, which the tile reads at its start and whose
//     own part it rewrites at its end;
//   - per step ONE value from the strip below, that strip's last odd state at the previous frame: the BOUNDARY COLUMN of strip
//     q - 1, one fp64 per frame, kept full length (T x strips) so nothing is overwritten while it can still be read.  A tile's last
//     thread stores its last odd state to its own column every step (a plain fire-and-forget vector store, like the backpointer
//     words); the block loads the column it reads into LDS ahead of use, 512 steps at a time.  The column of "strip -1" is -inf;
//   - lab[k0 - 1] for the skip flag of its first pair, read from the labels.
// Tile (p, q) depends on (p - 1, q) and (p, q - 1): ONE LAUNCH PER ANTI-DIAGONAL d = p + q, its blocks the tiles of that diagonal
// of all recordings of the call.  Stream order is the only synchronisation: no block waits for, polls or signals another, there is
// no grid barrier, no flag and no atomic.  The host builds the tile table sorted by diagonal and uploads it once; a launch gets an
// offset and a count.  Every tile runs, also those outside the reachable band (their values are -inf by the recursion itself).
//
// Pre-pass: align_long_lse_kernel (lse_t, one wave per frame) and align_long_init_kernel (one block per recording:
// any label outside [0, V) or equal to the blank, R = labels equal to their predecessor -> a flag per recording; the carry row at
// frame 0).  Tiles of a flagged recording return at once.  Finish: one block per recording takes the end state from the carry row,
// sums the score, and runs align.hip's windowed backtrace (128 frames x 128 pairs of backpointer words in LDS, one lane walking, the
// block writing the outputs); flagged recordings get their -1 / NaN rows here.  Backpointers: 2 bits per state in align.hip's word
// layout, word (g, q (sp / P) + tid) = step group g of thread tid of strip q, i.e. column pair / P of a row of strips x (sp / P)
// words; pf is a multiple of 8, so a step group never straddles a panel.  All backpointer, carry and column indices are 64-bit.
//
// The star (w2v2_ctc_align_long_star): align.hip's, operation for operation.  The pre-pass writes xs_t beside lse_t
// (align_long_lse_star_kernel), the init kernel admits the label V, and the tile and finish kernels carry align.hip's compile-time
// STAR flag: the mask of star pairs, xs_t loaded PD steps ahead, V and xs_t - lse_t on star frames.  STAR = false is the star-free code.
#include "ctc_lattice.h"

#include <algorithm>
#include <vector>

namespace w2v2 {
namespace {

constexpr int LONG_COL_CHUNK = 512;          // steps whose boundary-column values a tile holds in LDS at a time (a multiple of 8)
constexpr int LONG_DEFAULT_STRIP = 1024;     // pairs per strip and frames per panel when the caller passes 0: the fastest of the
constexpr int LONG_DEFAULT_PANEL = 512;      // measured grid (profiles/align_long.md)
constexpr int64_t LONG_DEFAULT_CAP = (int64_t)32 << 30;

struct LongSeg {
    int64_t row0;      // first logits row
    int64_t label0;    // first label
    int64_t out0;      // first output frame (also the first lse entry)
    int64_t bp0;       // first backpointer word
    int64_t carry0;    // first entry of the carry row (S entries)
    int64_t col0;      // first entry of the boundary columns (strips columns of T entries)
    int32_t T, U, strips, panels;
};

struct LongTile {
    int32_t rec, p, q, pad;
};

struct LongArgs {
    const float* logits;
    const int32_t* labels;
    const LongSeg* segs;
    const LongTile* tiles;
    double* lse;            // (sum T_i), indexed like the outputs
    int32_t* flag;          // per recording: 0 = aligned, 1 = infeasible (T < U + R), 2 = a bad label
    double* carry;
    double* col;
    uint32_t* bp;
    int32_t* token;
    int32_t* label_index;
    float* frame_logp;
    double* score;
    int V, blank;
    int sp, pf, wps;        // pairs per strip, steps per panel, backpointer words per strip and step group (= sp / P: the threads that hold states)
};

// lse_t of frame t of recording blockIdx.y: one wave per frame, grid.x covers the longest recording
__global__ __launch_bounds__(256) void align_long_lse_kernel(LongArgs a) {
    const LongSeg sg = a.segs[blockIdx.y];
    frame_lse(a.logits, a.V, sg.row0, sg.T, a.lse + sg.out0);
}

// ... and xs_t = m_t + star_score into xs, indexed like lse
__global__ __launch_bounds__(256) void align_long_lse_star_kernel(LongArgs a, double* xs, float star_score) {
    const LongSeg sg = a.segs[blockIdx.y];
    float m;
    const int t = frame_lse_max(a.logits, a.V, sg.row0, sg.T, a.lse + sg.out0, m);
    if (t >= 0 && (threadIdx.x & 63) == 0) xs[sg.out0 + t] = (double)m + (double)star_score;
}

// one block per recording: the two checks that span strips (integer counts: any order gives the same flag), then the carry row at
// frame 0: delta_0(0) = x_0(blank), delta_0(1) = x_0(l_0) (xs_0 for the star), every other state -inf
template <bool STAR>
__global__ __launch_bounds__(256) void align_long_init_kernel(LongArgs a, const double* xs) {
    constexpr double NEG = -__builtin_inf();
    __shared__ long long red[2][4];
    const LongSeg sg = a.segs[blockIdx.x];
    const int tid = threadIdx.x, U = sg.U, V = a.V, blank = a.blank;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    long long nbad = 0, rep = 0;
    for (int64_t k = tid; k < U; k += 256) {
        const int l = lab[k];
        if constexpr (STAR) nbad += l < 0 || l > V || l == blank;
        else nbad += l < 0 || l >= V || l == blank;
        rep += k >= 1 && l == lab[k - 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nbad += __shfl_xor(nbad, off, 64);
        rep += __shfl_xor(rep, off, 64);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = nbad;
        red[1][tid >> 6] = rep;
    }
    __syncthreads();
    nbad = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    rep = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const int flag = nbad ? 2 : ((long long)sg.T < (long long)U + rep ? 1 : 0);
    if (tid == 0) a.flag[blockIdx.x] = flag;
    if (flag) return;                                    // (block-uniform; the labels index the logits only behind this point)
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    double* __restrict__ cr = a.carry + sg.carry0;
    const int64_t S = 2 * (int64_t)U + 1;
    if constexpr (STAR) {
        for (int64_t s = tid; s < S; s += 256)
            cr[s] = s == 0 ? (double)lg[blank] : s == 1 ? (lab[0] == V ? xs[sg.out0] : (double)lg[lab[0]]) : NEG;
    } else {
        for (int64_t s = tid; s < S; s += 256) cr[s] = s == 0 ? (double)lg[blank] : s == 1 ? (double)lg[lab[0]] : NEG;
    }
}

// tile tile0 + blockIdx.x of the table: align.hip's sweep over one panel for one strip
template <int P, bool STAR>
__global__ __launch_bounds__(P == 8 ? LATTICE_MAX_THREADS : 256) void align_long_tile_kernel(LongArgs a, int64_t tile0, const double* xs) {
    // (xs: the star's emission per frame, indexed like a.lse; read only with STAR)
    constexpr int G = 8 / P;                 // steps per backpointer word
    constexpr int PD = P == 8 ? 2 : 8;       // steps the emissions and the column are loaded ahead (a multiple of G)
    constexpr double NEG = -__builtin_inf();
    __shared__ double xv[2][LATTICE_MAX_THREADS + 1];    // exchange: entry i + 1 = thread i's last odd state (entry 0 is not used: thread 0 reads cl)
    __shared__ double cl[LONG_COL_CHUNK];                // the column of the strip below, frames cb - 1 .. of the current chunk of steps

    const LongTile tl = a.tiles[tile0 + blockIdx.x];
    if (a.flag[tl.rec]) return;                          // (block-uniform)
    const LongSeg sg = a.segs[tl.rec];
    const int tid = threadIdx.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const bool act = tid < a.wps;                        // the threads past sp / P hold no state
    const int64_t k0 = (int64_t)tl.q * a.sp + (int64_t)tid * P;      // this thread's pairs: k0 .. k0 + P - 1

    // labels of the thread's pairs (the blank past U), the skip flags, and the states from the carry row.  Of the thread's pairs the
    // first nod have a label state (k < U) and the first nod + 1 a blank state (k <= U); nod = -1: none
    const int nod = act ? (int)max((int64_t)-1, min((int64_t)P, (int64_t)U - k0)) : -1;
    double* __restrict__ cr = a.carry + sg.carry0;
    int lj[P];
    unsigned skipm = 0, starm = 0;                       // starm (STAR): the pairs whose label is the star
    double ev[P], od[P];                                 // delta(2k), delta(2k + 1) of the thread's pairs
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t k = k0 + j;
        lj[j] = blank;
        ev[j] = NEG;
        od[j] = NEG;
        if (j <= nod) ev[j] = cr[2 * k];
        if (j < nod) {
            const int l = lab[k];
            if (k >= 1 && l != lab[k - 1]) skipm |= 1u << j;     // (the first pair of a strip: the label of the strip below)
            lj[j] = l;
            if constexpr (STAR) {
                if (l == V) {
                    starm |= 1u << j;
                    lj[j] = blank;                       // (the column this pair loads and discards)
                }
            }
            od[j] = cr[2 * k + 1];
        }
    }

    // ---- sweep: steps [tb, te) ----
    const int tb = 1 + tl.p * a.pf, te = (int)min((int64_t)tb + a.pf, (int64_t)T);
    const int64_t W = (int64_t)sg.strips * a.wps;        // backpointer words per step group
    uint32_t* __restrict__ bpw = a.bp + sg.bp0 + (int64_t)tl.q * a.wps + tid;
    const double* __restrict__ colr = tl.q > 0 ? a.col + sg.col0 + (int64_t)(tl.q - 1) * T : nullptr;       // column q: T entries
    double* __restrict__ colw = a.col + sg.col0 + (int64_t)tl.q * T;
    const bool wcol = tl.q + 1 < sg.strips && tid == a.wps - 1;      // the strip's last thread, when a strip above reads the column
    xv[0][tid + 1] = od[P - 1];                          // (tb - 1 is even)
    float qb[PD], ql[PD][P];                             // x_t(blank), x_t(l_k) of the next PD steps
    const double* __restrict__ xsr = STAR ? xs + sg.out0 : nullptr;
    double qs[STAR ? PD : 1];                            // xs_t of the next PD steps (STAR)
    qs[0] = 0.0;
#pragma unroll
    for (int i = 0; i < PD; ++i) {
        const float* __restrict__ row = lg + (int64_t)min(tb + i, T - 1) * V;
        qb[i] = row[blank];
        if constexpr (STAR) qs[i] = xsr[min(tb + i, T - 1)];
#pragma unroll
        for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
    }
    uint32_t word = 0;
    int cb = tb;                                         // first step of the current chunk
    auto step = [&](int t, float yb, const float* yl, double ys, int slot) {
        lds_barrier();
        const double nb = *(tid ? &xv[(t - 1) & 1][tid] : &cl[t - cb]);      // delta_{t-1}(2 k0 - 1)
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
            if constexpr (STAR) od[j] = j < nod ? mo + ((starm >> j & 1u) ? ys : (double)yl[j]) : NEG;
            else od[j] = j < nod ? mo + (double)yl[j] : NEG;
            ev[j] = j <= nod ? me + xb : NEG;
            bits |= (be | bo << 2) << (4 * j);
        }
        xv[t & 1][tid + 1] = od[P - 1];
        if (wcol) colw[t] = od[P - 1];
        word |= bits << (slot * 4 * P);
    };
    // Per chunk of LONG_COL_CHUNK steps the block first brings the column values of those steps into LDS (frames cb - 1 ..; never
    // past the panel's last step: the entries behind it are being written by this diagonal's tile of the strip below).  Inside a
    // chunk: whole groups of PD steps without a branch between them (the compiler's wait counts then stay exact); then the tail
    int t0 = tb;
    for (; cb < te; cb += LONG_COL_CHUNK) {
        const int ce = min(cb + LONG_COL_CHUNK, te);
        __syncthreads();                                 // (the previous chunk's values have been read)
        for (int i = tid; i < ce - cb; i += blockDim.x) cl[i] = (colr && cb - 1 + i > 0) ? colr[cb - 1 + i] : NEG;      // (frame 0: no column is written; a strip's last odd state, 2 sp - 1 or higher, is -inf there)
        __syncthreads();
        for (; t0 + PD <= ce; t0 += PD) {
#pragma unroll
            for (int i = 0; i < PD; ++i) {
                step(t0 + i, qb[i], ql[i], qs[STAR ? i : 0], i % G);
                if (i % G == G - 1) {
                    if (act) bpw[(int64_t)((t0 + i - 1) / G) * W] = word;
                    word = 0;
                }
                const float* __restrict__ row = lg + (int64_t)min(t0 + i + PD, T - 1) * V;      // (block-uniform row, per-lane column)
                qb[i] = row[blank];
                if constexpr (STAR) qs[i] = xsr[min(t0 + i + PD, T - 1)];
#pragma unroll
                for (int j = 0; j < P; ++j) ql[i][j] = row[lj[j]];
            }
        }
    }
    cb -= LONG_COL_CHUNK;                                // (the last chunk's base: the tail below lies in it)
#pragma unroll
    for (int i = 0; i < PD; ++i) {
        if (t0 + i < te) {                               // (block-uniform)
            step(t0 + i, qb[i], ql[i], qs[STAR ? i : 0], i % G);
            if (i % G == G - 1 || t0 + i == te - 1) {
                if (act) bpw[(int64_t)((t0 + i - 1) / G) * W] = word;
                word = 0;
            }
        }
    }
    // the carry row: this tile's own part
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t k = k0 + j;
        if (j <= nod) cr[2 * k] = ev[j];
        if (j < nod) cr[2 * k + 1] = od[j];
    }
}

// one block per recording: end state, score, backtrace (align.hip's, on rows of strips x wps words), or the -1 / NaN rows
template <int P, bool STAR>
__global__ __launch_bounds__(256) void align_long_finish_kernel(LongArgs a, const double* xs) {
    constexpr int G = 8 / P;
    constexpr double NEG = -__builtin_inf();
    __shared__ uint32_t win[LATTICE_WIN_WORDS];          // backtrace window of backpointer words
    __shared__ long long path[LATTICE_CHUNK + 1];
    __shared__ long long s_cur;

    const LongSeg sg = a.segs[blockIdx.x];
    const int tid = threadIdx.x, NT = blockDim.x, T = sg.T, U = sg.U, V = a.V, blank = a.blank;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const int32_t* __restrict__ lab = a.labels + sg.label0;
    const int flag = a.flag[blockIdx.x];
    if (flag) {
        const double sc = flag == 2 ? __builtin_nan("") : NEG;
        for (int t = tid; t < T; t += NT) {
            a.token[sg.out0 + t] = -1;
            a.label_index[sg.out0 + t] = -1;
            a.frame_logp[sg.out0 + t] = __builtin_nanf("");
        }
        if (tid == 0) a.score[blockIdx.x] = sc;
        return;                                          // (block-uniform)
    }
    // end state
    const double* __restrict__ cr = a.carry + sg.carry0;
    const double fin0 = cr[2 * (int64_t)U];              // delta(S - 1)
    const double fin1 = U >= 1 ? cr[2 * (int64_t)U - 1] : NEG;       // delta(S - 2)
    const bool last_odd = U >= 1 && !(fin0 > fin1);
    const double dend = last_odd ? fin1 : fin0;
    if (tid == 0) s_cur = last_odd ? 2 * (long long)U - 1 : 2 * (long long)U;

    // score: sum_t lse_t by wave 0 in align.hip's order (lane l: frames l, l + 64, ...; then a butterfly)
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
    const int64_t W = (int64_t)sg.strips * a.wps;
    int t_hi = T - 1;
    __syncthreads();
    while (true) {
        const int t_lo = max(0, t_hi - LATTICE_CHUNK);
        const long long s_hi = s_cur;
        // frames (t_lo, t_hi] read the words of step groups (t - 1) / G and of pairs (s_hi >> 1) - C + 1 .. s_hi >> 1
        const int ph = (int)(s_hi >> 1), pl = max(0, ph - LATTICE_CHUNK + 1);
        const int w_lo = pl / P, ncol = ph / P - w_lo + 1;
        const int g_lo = t_lo / G, nrow = t_hi > t_lo ? (t_hi - 1) / G - g_lo + 1 : 0;
        for (int i = tid; i < nrow * ncol; i += NT) {
            const int r = i / ncol, c = i - r * ncol;
            win[i] = bpg[(int64_t)(g_lo + r) * W + w_lo + c];
        }
        __syncthreads();
        if (tid == 0) {
            long long s = s_hi;
            for (int t = t_hi; t > t_lo; --t) {
                path[t - t_lo] = s;
                const int p = (int)(s >> 1), g = (t - 1) / G;
                const uint32_t w = win[(g - g_lo) * ncol + p / P - w_lo];
                s -= (long long)(w >> (((t - 1) % G) * 4 * P + 4 * (p % P) + 2 * (int)(s & 1)) & 3u);
            }
            path[0] = s;
            s_cur = s;
        }
        __syncthreads();
        for (int t = t_lo + (t_lo > 0) + tid; t <= t_hi; t += NT) {
            const long long s = path[t - t_lo];
            const int tok = (s & 1) ? lab[s >> 1] : blank;
            const int64_t o = sg.out0 + t;
            a.token[o] = tok;
            a.label_index[o] = (s & 1) ? (int)(s >> 1) : -1;
            if constexpr (STAR) a.frame_logp[o] = (float)((tok == V ? xs[o] : (double)lg[(int64_t)t * V + tok]) - a.lse[o]);
            else a.frame_logp[o] = (float)((double)lg[(int64_t)t * V + tok] - a.lse[o]);
        }
        if (t_lo == 0) break;
        t_hi = t_lo;
    }
}

// the geometry of a call and the bytes of its workspace, from the shapes alone
struct LongPlan {
    int sp, pf, P, G, nt, wps, Tmax, Umax;
    int64_t frames, tiles, diagonals;
    size_t tile_bytes, seg_bytes, lse_bytes, xs_bytes, flag_bytes, carry_bytes, col_bytes, bp_bytes;
    int64_t total;          // INT64_MAX when it does not fit
};

int long_plan(int n, const int32_t* frames, const int32_t* nlabels, int strip_pairs, int panel_frames, bool star, LongPlan& pl) {
    W2V2_REQUIRE(frames && nlabels, "ctc_align_long: null argument");
    W2V2_REQUIRE(n >= 1, "ctc_align_long: %d recordings (need at least one)", n);
    W2V2_REQUIRE(strip_pairs == 0 || (strip_pairs >= 64 && strip_pairs <= 8192 && strip_pairs % 64 == 0),
                 "ctc_align_long: strip_pairs %d (0, or a multiple of 64 in [64, 8192])", strip_pairs);
    W2V2_REQUIRE(panel_frames == 0 || (panel_frames >= 8 && panel_frames % 8 == 0),
                 "ctc_align_long: panel_frames %d (0, or a multiple of 8 that is at least 8)", panel_frames);
    pl.Tmax = pl.Umax = 0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(frames[i] >= 1, "ctc_align_long: recording %d has %d frames (need at least one)", i, frames[i]);
        W2V2_REQUIRE(nlabels[i] >= 0, "ctc_align_long: recording %d has %d labels", i, nlabels[i]);
        pl.Tmax = std::max(pl.Tmax, (int)frames[i]);
        pl.Umax = std::max(pl.Umax, (int)nlabels[i]);
    }
    // a strip no wider than the longest recording needs (whole waves of pairs); pairs per thread from the strip
    const int64_t need_pairs = (((int64_t)pl.Umax + 1 + 63) / 64) * 64;
    pl.sp = (int)std::min<int64_t>(strip_pairs ? strip_pairs : LONG_DEFAULT_STRIP, need_pairs);
    pl.pf = panel_frames ? panel_frames : LONG_DEFAULT_PANEL;
    pl.P = pairs_per_thread(pl.sp);
    pl.G = 8 / pl.P;
    pl.wps = pl.sp / pl.P;
    pl.nt = ((pl.wps + 63) / 64) * 64;
    unsigned __int128 tiles = 0, carry = 0, col = 0, words = 0, out = 0;
    int64_t diag = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t strips = ((int64_t)nlabels[i] + 1 + pl.sp - 1) / pl.sp, panels = ((int64_t)frames[i] - 1 + pl.pf - 1) / pl.pf;
        tiles += (unsigned __int128)strips * panels;
        carry += 2 * (unsigned __int128)nlabels[i] + 1;
        col += (unsigned __int128)frames[i] * strips;
        words += (unsigned __int128)(((int64_t)frames[i] - 1 + pl.G - 1) / pl.G) * strips * pl.wps;
        out += frames[i];
        if (panels) diag = std::max(diag, strips + panels - 1);
    }
    const unsigned __int128 lim = (unsigned __int128)1 << 62;
    pl.total = INT64_MAX;
    if (tiles > lim / 16 || carry > lim / 8 || col > lim / 8 || words > lim / 4 || out > lim / 8) return W2V2_OK;
    pl.frames = (int64_t)out;
    pl.tiles = (int64_t)tiles;
    pl.diagonals = diag;
    pl.tile_bytes = up256(std::max<unsigned __int128>(tiles, 1) * sizeof(LongTile));
    pl.seg_bytes = up256((unsigned __int128)n * sizeof(LongSeg));
    pl.lse_bytes = up256(out * sizeof(double));
    pl.xs_bytes = star ? pl.lse_bytes : 0;
    pl.flag_bytes = up256((unsigned __int128)n * sizeof(int32_t));
    pl.carry_bytes = up256(carry * sizeof(double));
    pl.col_bytes = up256(col * sizeof(double));
    pl.bp_bytes = up256(std::max<unsigned __int128>(words, 1) * sizeof(uint32_t));
    const unsigned __int128 total = (unsigned __int128)pl.tile_bytes + pl.seg_bytes + pl.lse_bytes + pl.xs_bytes + pl.flag_bytes + pl.carry_bytes +
                                    pl.col_bytes + pl.bp_bytes;
    if (total < lim) pl.total = (int64_t)total;
    return W2V2_OK;
}

}  // namespace

int64_t ctc_align_long_workspace(int n, const int32_t* frames, const int32_t* nlabels, int strip_pairs, int panel_frames, bool star) {
    LongPlan pl;
    if (int e = long_plan(n, frames, nlabels, strip_pairs, panel_frames, star, pl)) return e;
    return pl.total;
}

int launch_ctc_align_long(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int32_t* labels,
                          const int64_t* label0, const int32_t* nlabels, int blank, int32_t* token, int32_t* label_index,
                          float* frame_logp, double* score, int strip_pairs, int panel_frames, int64_t max_workspace_bytes,
                          hipStream_t s, bool star, float star_score) {
    W2V2_REQUIRE(logits && row0 && frames && labels && label0 && nlabels && token && label_index && frame_logp && score,
                 "ctc_align_long: null argument");
    W2V2_REQUIRE(V >= 1, "ctc_align_long: vocabulary of %d entries", V);
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_align_long: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(max_workspace_bytes >= 0, "ctc_align_long: max_workspace_bytes %lld is negative", (long long)max_workspace_bytes);
    W2V2_REQUIRE(!star || star_score <= 0.f, "ctc_align_long: star_score %g (a log-domain penalty per frame: <= 0, not NaN)", (double)star_score);
    LongPlan pl;
    if (int e = long_plan(n, frames, nlabels, strip_pairs, panel_frames, star, pl)) return e;
    for (int i = 0; i < n; ++i)
        W2V2_REQUIRE(row0[i] >= 0 && label0[i] >= 0, "ctc_align_long: recording %d has a negative offset", i);
    const int64_t cap = max_workspace_bytes ? max_workspace_bytes : LONG_DEFAULT_CAP;
    W2V2_REQUIRE(pl.total <= cap,
                 "ctc_align_long: the call needs %lld bytes of workspace (about frames x labels / 2 per recording); max_workspace_bytes "
                 "is %lld",
                 (long long)pl.total, (long long)cap);

    // the two tables: the recordings, and the tiles sorted by anti-diagonal (within one, in recording order)
    std::vector<LongSeg> segs((size_t)n);
    std::vector<int64_t> first((size_t)pl.diagonals + 1, 0);
    {
        int64_t out = 0, words = 0, carry = 0, col = 0;
        for (int i = 0; i < n; ++i) {
            const int strips = (int)(((int64_t)nlabels[i] + 1 + pl.sp - 1) / pl.sp), panels = (int)(((int64_t)frames[i] - 1 + pl.pf - 1) / pl.pf);
            segs[i] = LongSeg{row0[i], label0[i], out, words, carry, col, frames[i], nlabels[i], strips, panels};
            out += frames[i];
            words += (int64_t)((frames[i] - 1 + pl.G - 1) / pl.G) * strips * pl.wps;
            carry += 2 * (int64_t)nlabels[i] + 1;
            col += (int64_t)frames[i] * strips;
            for (int d = 0; panels && d < strips + panels - 1; ++d)      // tiles of diagonal d: p from max(0, d - strips + 1) to min(d, panels - 1)
                first[(size_t)d + 1] += std::min(d, panels - 1) - std::max(0, d - strips + 1) + 1;
        }
    }
    for (int64_t d = 0; d < pl.diagonals; ++d) first[(size_t)d + 1] += first[(size_t)d];
    std::vector<LongTile> tiles((size_t)pl.tiles);
    {
        std::vector<int64_t> next(first.begin(), first.end() - 1);
        for (int i = 0; i < n; ++i)
            for (int p = 0; p < segs[i].panels; ++p)
                for (int q = 0; q < segs[i].strips; ++q) tiles[(size_t)next[(size_t)(p + q)]++] = LongTile{i, p, q, 0};
    }

    // workspace: the tiles | the recordings | lse | xs (star calls only) | flags | carry rows | boundary columns | backpointer words
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_ALIGN_LONG, s, (size_t)pl.total, &raw)) return e;
    char* base = static_cast<char*>(raw);
    LongArgs a;
    a.logits = logits;
    a.labels = labels;
    a.tiles = reinterpret_cast<const LongTile*>(base);
    base += pl.tile_bytes;
    a.segs = reinterpret_cast<const LongSeg*>(base);
    base += pl.seg_bytes;
    a.lse = reinterpret_cast<double*>(base);
    base += pl.lse_bytes;
    double* xsw = star ? reinterpret_cast<double*>(base) : nullptr;
    const double* xs = xsw;
    base += pl.xs_bytes;
    a.flag = reinterpret_cast<int32_t*>(base);
    base += pl.flag_bytes;
    a.carry = reinterpret_cast<double*>(base);
    base += pl.carry_bytes;
    a.col = reinterpret_cast<double*>(base);
    base += pl.col_bytes;
    a.bp = reinterpret_cast<uint32_t*>(base);
    a.token = token;
    a.label_index = label_index;
    a.frame_logp = frame_logp;
    a.score = score;
    a.V = V;
    a.blank = blank;
    a.sp = pl.sp;
    a.pf = pl.pf;
    a.wps = pl.wps;
    // (one upload: the recordings' table lies right behind the tiles)
    if (int e = staged_upload(SCRATCH_ALIGN_LONG, s, raw,
                              {{tiles.data(), (size_t)pl.tiles * sizeof(LongTile), 0}, {segs.data(), (size_t)n * sizeof(LongSeg), pl.tile_bytes}},
                              (size_t)64 << 10))
        return e;
    // (work for the profile: the sweep's ~12 fp64 operations per state and step; the logits read once by the lse pass)
    double work = 0.0;
    for (int i = 0; i < n; ++i) work += 12.0 * (double)frames[i] * (2.0 * nlabels[i] + 1.0);
    ProfScope ps(nullptr, FAM_CTC, work, 4.0 * (double)pl.frames * V, s);
    auto run = [&](auto st) {
        constexpr bool STAR = decltype(st)::value;
        if constexpr (STAR) W2V2_LAUNCH(align_long_lse_star_kernel, dim3((unsigned)((pl.Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a, xsw, star_score);
        else W2V2_LAUNCH(align_long_lse_kernel, dim3((unsigned)((pl.Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
        W2V2_LAUNCH(align_long_init_kernel<STAR>, dim3((unsigned)n), dim3(256), 0, s, a, xs);
        for (int64_t d = 0; d < pl.diagonals; ++d) {
            const int64_t off = first[(size_t)d], count = first[(size_t)d + 1] - off;
            if (!count) continue;
            dispatch_pairs(pl.P, [&](auto p) {
                W2V2_LAUNCH((align_long_tile_kernel<decltype(p)::value, STAR>), dim3((unsigned)count), dim3((unsigned)pl.nt), 0, s, a, off, xs);
            });
        }
        dispatch_pairs(pl.P, [&](auto p) {
            W2V2_LAUNCH((align_long_finish_kernel<decltype(p)::value, STAR>), dim3((unsigned)n), dim3(256), 0, s, a, xs);
        });
    };
    if (star) run(std::true_type());
    else run(std::false_type());
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
