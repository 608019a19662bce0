// Edit distance with its substitution / deletion / insertion breakdown, for many pairs of int32 token sequences at once
// (w2v2_edit_distance).  Model-free, like align.hip and beam.hip: host tables say which ranges of one token buffer
// form a pair, and every pair is computed as if it were alone.
//
// Definition (tests/edit_reference.py implements exactly this).  Hypothesis a (length m), reference b (length n).  v[i][j] is the
// lexicographically smallest (cost, substitutions) over the alignments of a[0, i) with b[0, j):
//   v[i][0] = (i, 0), v[0][j] = (j, 0),
//   v[i][j] = min(v[i-1][j-1] + (a_i == b_j ? (0, 0) : (1, 1)), v[i-1][j] + (1, 0), v[i][j-1] + (1, 0)).
// With (C, S) = v[m][n]: distance = C, substitutions = S, deletions D = (C - S - (m - n)) / 2, insertions I = D + m - n.  The
// result is a property of the pair (no tie-break rule enters it), so any evaluation order gives the same integers.
//
// A cell is ONE unsigned 32-bit word, C << 16 | S: C <= max(i, j) <= 65535 and S <= C, the lexicographic order is the unsigned
// order, and the recurrence is three adds and two unsigned mins.  The adds SATURATE: a candidate built on a cost of 65535 would
// carry into bit 32; it is never the minimum (the cell's own cost is at most 65535, and another candidate reaches it), so clamping
// it to 0xffffffff, the largest word, leaves the minimum what it is.
//
// Structure.  A wave owns a pair.  It walks the hypothesis in stripes of 64 rows, lane l holding row 64 r + l + 1 of stripe r, and
// sweeps a stripe along its anti-diagonals: at step t lane l computes column t - l + 1 (columns <= 0 are virtual, see edit_pair).
// Of a cell's three neighbours the left one is the lane's own previous word and the diagonal one its previous upper neighbour;
// the upper one is the word lane l - 1 produced a step earlier and arrives by a wave-wide DPP shift by one lane (v_mov_b32
// wave_shr:1), as does the reference token, which enters at lane 0 and moves down a lane per step.  Lane 0's upper neighbour is
// the boundary row, the last row of the stripe above (row 0: j << 16): the wave reads it 64 columns at a time, one group ahead,
// and picks a step's entry with v_readlane; the words lane 63 produces are collected the same way and written back 64 at a time
// IN PLACE (a column is written at least 63 steps after the wave read it, so one row per pair suffices).  The boundary row lives
// in the wave's slice of LDS for references of up to EDIT_LDS_REF tokens, and in a workspace row of the launch's longest reference
// per resident wave beyond that: memory is O(n) per resident pair and never O(m n).  No barrier: a wave shares nothing.
// The host sorts the pairs by cell count, longest first, so that the long ones do not trail the launch, and makes at most two
// launches per call: the LDS pairs, one per wave and four waves to a block, and the workspace pairs on a persistent grid whose
// wave w takes pairs w, w + W, ... into its own row.  No atomics; a pair's words never depend on the launch around it.
#include "common.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace w2v2 {
namespace {

constexpr int EDIT_WAVES = 4;                // waves (pairs in flight) per block
constexpr int EDIT_LDS_REF = 2048;           // longest reference whose boundary row stays in LDS (8 KB per wave)
constexpr int EDIT_WS_WAVES = 512;           // resident waves of the workspace launch (128 blocks): 512 rows of the longest reference

struct EditPair {
    int64_t hyp0, ref0;
    int32_t m, n, out, pad;
};

// lane l <- v of lane l - 1; lane 0 <- feed
__device__ __forceinline__ uint32_t lane_shr1(uint32_t feed, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)feed, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t add_sat(uint32_t a, uint32_t b) { return __builtin_elementwise_add_sat(a, b); }
// orders the wave's boundary-row stores before its later loads of the same words, for the compiler; the hardware keeps one
// wave's accesses to an address in order
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// one pair by one wave; bnd: the wave's boundary row (n words; LDS or global)
template <typename Bnd>
__device__ __forceinline__ void edit_pair(const int32_t* __restrict__ tok, const EditPair pr, Bnd bnd, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int m = pr.m, n = pr.n;
    uint32_t fin;
    if (m == 0 || n == 0) {                                  // (wave-uniform)
        fin = (uint32_t)(m + n) << 16;
    } else {
        const int32_t* __restrict__ a = tok + pr.hyp0;
        const int32_t* __restrict__ b = tok + pr.ref0;
        const int stripes = (m + 63) >> 6;
        uint32_t cur = 0;
        for (int r = 0; r < stripes; ++r) {
            const int i = (r << 6) + lane + 1;               // this lane's row
            const int rows = min(64, m - (r << 6));
            const int steps = n + rows - 1;                  // the stripe's last row finishes column n at the last step
            const bool last = r == stripes - 1;
            const int32_t ai = i <= m ? a[i - 1] : 0;
            // before its column 1 (steps 0 .. lane - 1) a lane runs the same recurrence over virtual columns j <= 0 that hold
            // v[i][j] = (i - j, 0): there the upper neighbour + 1 reproduces the pattern, so v[i][0] = (i, 0) comes out of the
            // recurrence itself and no step needs a guard.  Costs clamp at 65535: a clamped virtual word is still no smaller
            // than any candidate that matters, and row i's upper neighbour at column 0 is exact.
            cur = (uint32_t)min(i + lane, 65535) << 16;              // v[i][-lane], this lane's left neighbour at step 0
            uint32_t diag = (uint32_t)min(i - 1 + lane, 65535) << 16;      // v[i-1][-lane]
            uint32_t tk = 0, outw = 0;
            // group g of 64 steps reads reference tokens b[64 g + lane] and boundary columns 64 g + lane + 1, loaded a group ahead
            auto load_b = [&](int c) { return c < n ? (uint32_t)b[c] : 0u; };
            auto load_bnd = [&](int c) { return r == 0 ? (uint32_t)(c + 1) << 16 : (c < n ? bnd[c] : 0u); };
            uint32_t bn = load_b(lane), un = load_bnd(lane);
            for (int t0 = 0; t0 < steps; t0 += 64) {
                const uint32_t bc = bn, uc = un;
                bn = load_b(t0 + 64 + lane);
                un = load_bnd(t0 + 64 + lane);
                const int ks = min(64, steps - t0);
                auto step = [&](int k, bool collect) {
                    const uint32_t up = lane_shr1((uint32_t)__builtin_amdgcn_readlane((int)uc, k), cur);
                    tk = lane_shr1((uint32_t)__builtin_amdgcn_readlane((int)bc, k), tk);
                    const uint32_t c0 = add_sat(diag, (uint32_t)ai == tk ? 0u : 0x10001u);
                    const uint32_t c1 = add_sat(min(up, cur), 0x10000u);
                    cur = min(c0, c1);                       // (past column n: never read)
                    diag = up;
                    // lane 63's word of this step is column t - 62: slot k of the group
                    if (collect) outw = lane == k ? (uint32_t)__builtin_amdgcn_readlane((int)cur, 63) : outw;
                };
                if (last) {
                    for (int k = 0; k < ks; ++k) step(k, false);
                } else {
                    for (int k = 0; k < ks; ++k) step(k, true);
                    const int c = t0 + lane - 63;            // column - 1 of this lane's slot
                    if (lane < ks && c >= 0 && c < n) bnd[c] = outw;
                }
            }
            wave_fence();
        }
        fin = (uint32_t)__builtin_amdgcn_readlane((int)cur, (m - 1) & 63);
    }
    if (lane == 0) {
        const int C = (int)(fin >> 16), S = (int)(fin & 0xffffu);
        const int D = (C - S - (m - n)) / 2;
        int32_t* __restrict__ o = out + (int64_t)pr.out * 4;
        o[0] = C;
        o[1] = S;
        o[2] = D;
        o[3] = D + m - n;
    }
}

// pairs [first, first + count) of the table, one per wave; lds_ref: words of a wave's boundary row
__global__ __launch_bounds__(EDIT_WAVES * 64) void edit_lds_kernel(const int32_t* __restrict__ tok, const EditPair* __restrict__ pairs,
                                                                  int first, int count, int lds_ref, int32_t* __restrict__ out) {
    extern __shared__ uint32_t edit_rows[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = blockIdx.x * EDIT_WAVES + wave;
    if (p >= count) return;                                  // (wave-uniform; no barrier follows)
    edit_pair(tok, pairs[first + p], edit_rows + wave * lds_ref, out);
}

// pairs [0, count) of the table on a persistent grid: wave w takes w, w + W, ... with row w of the workspace
__global__ __launch_bounds__(EDIT_WAVES * 64) void edit_ws_kernel(const int32_t* __restrict__ tok, const EditPair* __restrict__ pairs,
                                                                 int count, uint32_t* __restrict__ ws, int64_t ws_row,
                                                                 int32_t* __restrict__ out) {
    const int w = blockIdx.x * EDIT_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = gridDim.x * EDIT_WAVES;
    uint32_t* __restrict__ row = ws + (int64_t)w * ws_row;
    for (int p = w; p < count; p += W) edit_pair(tok, pairs[p], row, out);
}

}  // namespace

int launch_edit_distance(const int32_t* tokens, int64_t n_tokens, int n_pairs, const int64_t* hyp0, const int32_t* hyp_len,
                         const int64_t* ref0, const int32_t* ref_len, int32_t* out, hipStream_t s) {
    W2V2_REQUIRE(tokens && hyp0 && hyp_len && ref0 && ref_len && out, "edit_distance: null argument");
    W2V2_REQUIRE(n_pairs >= 1, "edit_distance: %d pairs (need at least one)", n_pairs);
    W2V2_REQUIRE(n_tokens >= 0, "edit_distance: negative token count");
    for (int p = 0; p < n_pairs; ++p) {
        W2V2_REQUIRE(hyp0[p] >= 0 && ref0[p] >= 0, "edit_distance: pair %d has a negative offset", p);
        W2V2_REQUIRE(hyp_len[p] >= 0 && ref_len[p] >= 0, "edit_distance: pair %d has a negative length", p);
        W2V2_REQUIRE(hyp_len[p] <= W2V2_EDIT_MAX_LEN && ref_len[p] <= W2V2_EDIT_MAX_LEN,
                     "edit_distance: pair %d has lengths %d and %d; at most %d tokens per sequence", p, hyp_len[p], ref_len[p],
                     W2V2_EDIT_MAX_LEN);
        W2V2_REQUIRE(hyp0[p] <= n_tokens - hyp_len[p] && ref0[p] <= n_tokens - ref_len[p],
                     "edit_distance: pair %d reaches past the %lld tokens", p, (long long)n_tokens);
    }
    // the workspace pairs first, then the LDS pairs; inside each, most cells first (ties by index: the order is a function of the lengths)
    std::vector<int> order((size_t)n_pairs);
    std::iota(order.begin(), order.end(), 0);
    auto cells = [&](int p) { return (int64_t)(hyp_len[p] + 63) / 64 * (ref_len[p] + 63); };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const bool wx = ref_len[x] > EDIT_LDS_REF, wy = ref_len[y] > EDIT_LDS_REF;
        if (wx != wy) return wx;
        return cells(x) > cells(y);
    });
    int n_ws = 0, ws_ref = 0, lds_ref = 0;
    double work = 0.0;
    for (int p = 0; p < n_pairs; ++p) {
        if (ref_len[p] > EDIT_LDS_REF) {
            ++n_ws;
            ws_ref = std::max(ws_ref, (int)ref_len[p]);
        } else {
            lds_ref = std::max(lds_ref, (int)ref_len[p]);
        }
        work += (double)hyp_len[p] * ref_len[p];
    }
    lds_ref = std::max(64, (lds_ref + 63) & ~63);
    const int ws_blocks = std::min((n_ws + EDIT_WAVES - 1) / EDIT_WAVES, EDIT_WS_WAVES / EDIT_WAVES);
    const int64_t ws_row = (ws_ref + 63) & ~63;
    // workspace: the table | the boundary rows of the workspace launch
    const size_t tab_bytes = up256((size_t)n_pairs * sizeof(EditPair));
    const size_t ws_bytes = (size_t)ws_blocks * EDIT_WAVES * (size_t)ws_row * sizeof(uint32_t);
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_EDIT, s, tab_bytes + ws_bytes, &raw)) return e;
    const EditPair* pairs = static_cast<const EditPair*>(raw);
    uint32_t* ws = reinterpret_cast<uint32_t*>(static_cast<char*>(raw) + tab_bytes);
    auto fill = [&](void* stage) {                       // (the rows are written straight into the pinned stage)
        EditPair* t = static_cast<EditPair*>(stage);
        for (int k = 0; k < n_pairs; ++k) {
            const int p = order[k];
            t[k] = EditPair{hyp0[p], ref0[p], hyp_len[p], ref_len[p], p, 0};
        }
    };
    if (int e = staged_fill(SCRATCH_EDIT, s, raw, (size_t)n_pairs * sizeof(EditPair), (size_t)64 << 10, fill)) return e;
    // (work for the profile: ~10 integer operations per cell; the tokens are read once per stripe)
    ProfScope ps(nullptr, FAM_CTC, 10.0 * work, 0.0, s);
    if (n_ws > 0) W2V2_LAUNCH(edit_ws_kernel, dim3((unsigned)ws_blocks), dim3(EDIT_WAVES * 64), 0, s, tokens, pairs, n_ws, ws, ws_row, out);
    const int n_lds = n_pairs - n_ws;
    if (n_lds > 0)
        W2V2_LAUNCH(edit_lds_kernel, dim3((unsigned)((n_lds + EDIT_WAVES - 1) / EDIT_WAVES)), dim3(EDIT_WAVES * 64),
                    (size_t)EDIT_WAVES * lds_ref * sizeof(uint32_t), s, tokens, pairs, n_ws, n_lds, lds_ref, out);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
