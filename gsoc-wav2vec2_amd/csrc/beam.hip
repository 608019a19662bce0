// CTC prefix beam search: the n best transcripts of each of n utterances with their log-probabilities, optionally fused with a
// character n-gram language model held as a dense table on the device, or with a word n-gram model and a lexicon (second part of
// this header), and with a phrase bias on top of either (third part).  Model-free, like ctc.hip and align.hip.
//
// Definition (tests/beam_reference.py implements exactly this).  x_t(v) is the fp32 logit widened to fp64, lp_t(v) = x_t(v) - lse_t
// (lse_t: ctc_lattice.h, frame_lse), lse2(a, b) = max + log1p(exp(-|a - b|)) with -inf neutral.  A beam entry is a
// prefix p (labels, no blanks) with pb, pnb (log-probability of the frame paths so far that collapse to p and end in a blank / a
// non-blank) and lm(p).  Start: the empty prefix, pb = 0, pnb = -inf, lm = 0.  Per frame, from every entry, tot = lse2(pb, pnb):
//   stay    p     : pb'  = tot + lp(blank);  pnb' = pnb + lp(p[-1]) if p is not empty
//   extend  p + c : pnb' = (pb if c == p[-1] else tot) + lp(c);  lm(p + c) = (lm(p) + alpha table[ctx(p), c]) + beta   (c != blank)
// If p + c is itself in the beam (entry q), the extension is no candidate of its own: q gets pnb' = lse2(pnb', that term).  Candidate
// index j V + blank for the prefix already at rank j, j V + c for a new one made from rank j.  Key = lse2(pb', pnb') + lm; -inf keys
// drop; the W largest keys form the next beam in key order, equal keys by ascending index.  Result: the first nbest entries after
// the last frame: labels, length, score = lse2(pb, pnb) (the CTC log-probability over the frame paths the beam kept: a LOWER
// bound of the exact value, equal to it when nothing was pruned), total = score + lm.  ctx(p): the last order - 1 labels of p as
// digits base V, oldest first, blank-filled.  An utterance with a non-finite lse_t (a NaN or +inf logit, a frame of -inf only)
// has no hypothesis: every length -1, score = total = NaN.
//
// Structure.  beam_lse_kernel: one wave per frame.  beam_search_kernel: one block of 256 threads (one wave
// per SIMD) per utterance, every score fp64.  Why 256: the W V <= 4096 candidate keys of a step live in registers, 16 per thread at
// the limits (32 VGPRs for the keys); more waves would only add to every barrier of a step that is latency-, not throughput-bound.
//  * Prefixes are nodes (parent, label) of a per-utterance trie in the workspace, one 8-byte plain store per NEW survivor; node
//    1 + t W + rank, so T W + 1 nodes bound it and no counter is needed.  A prefix that was pruned and is made again gets a second
//    node, so node identity alone does not answer "is p + c in the beam".  Each entry carries a 64-bit hash of its prefix and of its
//    parent prefix and its length: an entry q is p + c iff len(q) = len(p) + 1, hash(parent of q) = hash(p) and the prefixes are
//    equal -- the last is known when q's parent node IS p's node, and otherwise (rare) decided exactly by walking both chains
//    (same_prefix), after which q is re-pointed at p's node.  Hashes only ever save that walk; they decide nothing.
//  * Per step: (1) the W x W match, 4 lanes per entry, gives each entry the rank of its parent (mi) and each entry the set of its
//    children's labels (a 64-bit mask: V <= 64); (2) every thread computes the keys of its candidates (index k 256 + tid) while wave
//    0 computes the <= W "stay" candidates, the only ones that need lse2 (two in a row: the step's serial floor); (3) an exact
//    radix select, 8 bits per pass, on the 80-bit composite (order-preserving image of the key, then 0xffff - index): a 256-bin
//    LDS histogram (integer ds_add: counts do not depend on arrival order -- the only atomics in the file), every wave scanning it
//    redundantly so that a pass costs ONE barrier; it stops as soon as the boundary bin holds exactly what is still needed (3-4
//    passes on distinct keys; the index passes run only on keys that are bit-equal at the boundary); (4) the survivors are compacted
//    by ballots (slots fixed by their indices alone), ranked by a W x W count of larger composites (4 lanes per survivor) and written to the other beam
//    buffer.  Barriers are LDS-only (s_waitcnt lgkmcnt(0); s_barrier) except the one that ends a step, which also drains the
//    node stores so that same_prefix may read them.
//  * LDS: beam state as structure-of-arrays of 64 (doubles and ints: consecutive lanes on consecutive banks; the match reads one
//    entry per 4 lanes, a broadcast); the log-probabilities of 8 frames ahead in a double-buffered ring, loaded one step and
//    written at its end; the language model row values are loaded at the top of a step, used after the match.
//  * After the sweep nbest lanes walk their node chains back to the root and write the labels with plain stores (the rest of each
//    row is -1).  Two identical calls give identical bits; neighbours, order and repetition have no influence.
//
// Word n-gram language model with a lexicon (w2v2_ctc_beam_search_words; tests/wordlm_reference.py implements exactly
// this from the prefix alone).  One label d is the word delimiter; a prefix is split into words at d, empty words do not exist.
//  * Compiled model (host, from an ARPA model): words 0 .. NW - 1 with `unk` and `eos` (or -1); one state per context of 0 to
//    order - 1 words, state 0 the empty context, the start state the context <s> if the model has it; per state a backoff weight
//    bo[s] and a backoff state bstate[s] (the context without its oldest word), and arcs (word, logp, next_state) sorted by word,
//    next_state = the longest suffix of h w that is a state.  fp32 values, widened to fp64.  State 0 holds every word, in order.
//    lookup(s, w): acc = 0; search w among the arcs of s; hit: (acc + logp, next_state); miss: acc = acc + bo[s], s = bstate[s], again.
//  * Lexicon: a trie over labels, child[node, c] dense (n_nodes, V), -1 no child; word_at[node] a word or -1; node 0 the root.
//  * Every entry carries (wnode, lmstate) beside lm, functions of the prefix alone; wnode -2 = left the lexicon.  Extension by c:
//      c != d          : wnode' = child[wnode, c] (-2 stays -2); no child: dropped (key -inf) when unk_penalty = -inf (CONSTRAINED
//                        mode), else wnode' = -2.  lm' = lm, lmstate' = lmstate.
//      c == d, wnode 0 : nothing changes (no word ended).
//      c == d, w = word_at[wnode] >= 0 : (lpw, s') = lookup(lmstate, w); lm' = (lm + alpha lpw) + beta; wnode' = 0, lmstate' = s'.
//      c == d otherwise: constrained: dropped; else (lpu, s') = lookup(lmstate, unk); lm' = (lm + alpha (lpu + unk_penalty)) + beta;
//                        wnode' = 0, lmstate' = s'.
//    pb, pnb, the key, the tie rule, the -inf drop and bad rows are the search's above.
//  * Finalisation, per entry in beam order: fin = lm if wnode = 0, else the lm' of the c == d rule (the entry is removed where that
//    rule drops it); with an eos word and score_eos: fin = fin + alpha lookup(state after that word, eos).logp (no beta);
//    total = score + fin; the entries in descending total, equal totals by beam rank; the first nbest are returned, labels as
//    searched (no delimiter appended).  Nothing left: no hypothesis (length -1, NaN).
//  * In the kernel (beam_search_kernel<true>): the child lookups of a step's candidates replace the table loads at the top of the
//    step; the c == d rule of an entry is evaluated ONCE, by the lane that writes the entry into the next beam, and kept with it
//    (dlm, dstate; dstate -1 = dropped), so a step's delimiter candidates and the finalisation only read it; an entry that stays
//    copies it.  lookup is a binary search per backoff level, state 0 indexed directly.  No barrier is added to a step.
//
// Phrase bias (contextual biasing, "hotwords"; w2v2_ctc_beam_search_biased; tests/bias_reference.py implements exactly
// this from the prefix alone, by brute force over the phrase list, with no automaton).  On top of either search above.
//  * A bias is a set of phrases.  Phrase h is a label string h_0 .. h_{m-1}, labels in [0, V), none the blank, with a boost b_h in
//    nats per COUNTED label (finite, >= 0) and the weight w_h = b_h counted(h).  With `whole_words` (host) every phrase is wrapped in
//    one leading and one trailing word delimiter; those two are not counted, every other label is, and the string in front of the
//    first label of a prefix is one delimiter.
//  * state(p): the longest suffix of the prefix p that is a prefix of some phrase, proper or whole; the empty string is the root.
//    C(p): the sum of w_h over all i <= len(p) and all phrases h that p[:i] ends with: EVERY occurrence counts, overlapping and nested
//    ones included (with the phrases NEW YORK and YORK the string NEW YORK earns both weights).
//    phi(s) = (partial counted(s)) max{b_h : s is a PROPER prefix of h}, 0 where no such h exists and at the root: credit in advance
//    for a phrase under way, which keeps it in the beam; partial in [0, 1], 1 by convention (not tuned), 0 = completed phrases only.
//    The bias of a prefix is B(p) = C(p) + phi(state(p)).
//  * Transition from state s by label c, s' = state(s + c):
//      delta(s, c) = ([the sum of w_h, in phrase order, over the phrases h that s + c ends with] + phi(s')) - phi(s)
//    formed in fp64 and rounded ONCE to fp32.  End of the utterance: final(s) = E(s) - phi(s), rounded once; E(s) = 0 without
//    whole_words, else the sum of w_h over the phrases that s + delimiter ends with (the end closes a word).  So an unfinished phrase
//    gives its credit back, at the label that leaves it or at the end, and the sum along a prefix plus final is C(p) (+ E).
//  * Compiled on the host (wav2vec2.decoding.ContextBias): an Aho-Corasick automaton with its failure links resolved into dense tables
//    next (n_states, V) int32, delta (n_states, V) fp32, final (n_states) fp32; state 0 the root; the blank's column next = s, delta = 0.
//  * In the search every entry carries its state bst, a function of the prefix alone like lm; the empty prefix starts at start_state
//    with lm = 0.  Every product or sum one fp64 operation, in this order:
//      character table or none: lm(p + c) = ((lm(p) + alpha table[ctx, c]) + beta) + (double)delta[bst(p), c]
//      word model             : the lm' of the rules above, for c == d and c != d alike, then + (double)delta[bst(p), c]; the cached dlm
//                               stays the value of the word rule alone: the candidate adds its delta
//      bst(p + c) = next[bst(p), c]
//    Keys, the -inf drop, ties, the merging of p + c into an entry already in the beam (which keeps its own lm and bst) and bad rows
//    are unchanged.  Finalisation, both forms: fin = lm (word model: after the open word and eos) + (double)final[bst]; total =
//    score + fin; the final beam in descending total, equal totals by beam rank; the first nbest are returned.
//  * In the kernel (beam_search_kernel<WORD, true>; the two <., false> instances are the searches above, instruction for
//    instruction): bst lives in LDS arrays of its own (two halves of 64 ints beside the two beam buffers, and s_bst for the
//    survivors' parents), so BeamBuf / BeamBufWord keep their layouts; the deltas of a thread's candidates are loaded at the top of
//    the step beside lmv / wch (one fp32 per candidate from delta[bst[j] V + c], at most 16 per thread) and used after the match; the
//    new state is read once, by the lane that writes the entry into the next beam, where word_end is evaluated; a stay copies it.  No
//    barrier and no atomic is added to a step; every store is a plain vector store.
//
// Resumable search (streaming; w2v2_ctc_beam_search_stream).  The definition above is a recursion over frames, so a
// search may stop after any frame and go on later: the four <., ., true> instances run the SAME step body (the four <., ., false>
// instances are the searches above, instruction for instruction) between a load and a store of the beam.
//  * State slab, per stream, in global memory: the live BeamBuf / BeamBufWord, its half of bst, nb, a sticky `dead` flag, stable_len
//    and stable_node.  A call with frames_done == 0 starts from the empty prefix as above; one with frames_done > 0 loads the slab
//    into half 0 (buf[0], bst[0]) before the barrier that precedes the first step.  Step parity and the ring of log-probabilities are
//    functions of the call-local t, so where a recording is cut changes which half an entry sits in and nothing else.  After the last
//    step the live half goes back to the slab with plain vector stores; finalisation only reads the beam, so a call that returns
//    hypotheses leaves the next call what a call without results would have left.
//  * Nodes are numbered 1 + (frames_done + t) W + rank in a trie buffer the caller keeps for the stream (not in the call's scratch):
//    same_prefix and the label walks cross into nodes of earlier calls, which stream order makes visible.
//  * A call whose new frames hold a non-finite lse, or whose slab is dead, sets `dead`, advances nothing and reports no hypothesis, as
//    does every later call of that stream.  A call of zero frames loads, stores and reports again.
//  * stable_len: the length of the longest common prefix of the label strings of the nb entries after the call.  Every later entry
//    extends a current one, so it never decreases and every hypothesis of a later call begins with those labels.  Wave 0 computes it
//    after the state store: the entries walk their chains to the shortest entry's depth, then down in lockstep to the previous call's
//    stable_len only, comparing LABELS across lanes (a prefix made twice has two nodes); once all chains stand on one node the rest
//    is common.  stable_node is lane 0's node at that depth.  No atomic, no LDS, no barrier beyond those of the search above.
//  * With a null labels array the call ends there: no -1 fill, no finalisation, no walk.
#include "ctc_lattice.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace w2v2 {
namespace {

constexpr int BEAM_NT = 256;
constexpr int BEAM_W = W2V2_BEAM_MAX_WIDTH;
constexpr int BEAM_V = W2V2_BEAM_MAX_VOCAB;
constexpr int BEAM_KMAX = BEAM_W * BEAM_V / BEAM_NT;        // candidate keys per thread at the limits
constexpr int BEAM_RING = 8;                                  // frames of log-probabilities per ring half
static_assert(BEAM_W == 64 && BEAM_V == 64, "beam.hip: one 64-bit child mask per entry, 4 lanes per entry in 256 threads");

typedef unsigned long long u64;

struct BeamSeg {
    int64_t row0;      // first logits row
    int64_t lse0;      // first lse entry
    int64_t node0;     // first trie node
    int32_t T;
    int32_t done;      // frames of this stream that earlier calls searched (0 outside the resumable entry)
};

struct BeamArgs {
    const float* logits;
    const BeamSeg* segs;
    double* lse;
    u64* nodes;             // (parent << 32) | label
    const float* lm;        // (ctxmod, V) or null
    int32_t* labels;
    int32_t* length;
    double* score;
    double* total;
    double alpha, beta;
    int V, blank, W, nbest, max_len, ctxmod;
};

// the device arrays of a compiled word model and lexicon (w2v2_word_lm) and the search's scalars
struct BeamWordArgs : BeamArgs {
    w2v2_word_lm w;
    double unk_penalty;
    int delim, constrained, score_eos;
};

// the device tables of a compiled phrase bias (w2v2_ctc_bias) behind the arguments of either form
template <class Base>
struct BeamBiasArgs : Base {
    const int32_t* bnext;   // (n_states, V)
    const float* bdelta;    // (n_states, V)
    const float* bfinal;    // (n_states)
    int bstart;
};

// the state slabs and the stable-prefix output of the resumable instances behind the arguments of any of the four forms
template <class Base>
struct BeamStreamArgs : Base {
    char* state;            // n slabs of BEAM_STATE_BYTES
    int32_t* stable_len;    // (n)
};

template <bool WORD, bool BIAS>
using BeamFormArgs = std::conditional_t<BIAS, BeamBiasArgs<std::conditional_t<WORD, BeamWordArgs, BeamArgs>>,
                                        std::conditional_t<WORD, BeamWordArgs, BeamArgs>>;
template <bool WORD, bool BIAS, bool STREAM = false>
using BeamKernelArgs = std::conditional_t<STREAM, BeamStreamArgs<BeamFormArgs<WORD, BIAS>>, BeamFormArgs<WORD, BIAS>>;

struct BeamBuf {
    double pb[BEAM_W], pnb[BEAM_W], tot[BEAM_W], lm[BEAM_W];
    u64 h[BEAM_W], hp[BEAM_W];                  // hash of the prefix, of its parent prefix
    int node[BEAM_W], pn[BEAM_W];               // trie node, parent's node
    int len[BEAM_W], last[BEAM_W], ctx[BEAM_W];
    int mi[BEAM_W];                             // rank of the entry that is this prefix without its last label, or -1
};

struct BeamBufWord : BeamBuf {
    double dlm[BEAM_W];                         // lm and lmstate of this prefix + d (the c == d rule); dstate -1: dropped
    int wnode[BEAM_W], lmstate[BEAM_W], dstate[BEAM_W];
};

// A stream's state slab (w2v2_ctc_beam_search_stream): what a call leaves for the next one.  One size for all four forms.
//   [0, 256)   int32 nb, dead, stable_len, stable_node
//   [256, 512) the bias states of the entries (64 int32)
//   [512, ..)  the live BeamBuf / BeamBufWord
constexpr int BEAM_STATE_BST = 256, BEAM_STATE_BUF = 512;
constexpr int BEAM_STATE_BYTES = BEAM_STATE_BUF + (int)sizeof(BeamBufWord);
static_assert(BEAM_STATE_BYTES % 256 == 0 && sizeof(BeamBuf) % 8 == 0 && sizeof(BeamBufWord) % 8 == 0, "beam.hip: state slab layout");
typedef u64 __attribute__((may_alias)) u64_alias;         // a beam buffer copied as 8-byte words

__global__ __launch_bounds__(256) void beam_lse_kernel(BeamArgs a) {
    const BeamSeg sg = a.segs[blockIdx.y];
    frame_lse(a.logits, a.V, sg.row0, sg.T, a.lse + sg.lse0);
}

// the search's own lse2 (header; tests/beam_reference.py): log1p and early returns, so other bits than ctc_lattice.h's lse2
__device__ __forceinline__ double beam_lse2(double a, double b) {
    constexpr double NEG = -__builtin_inf();
    if (a == NEG) return b;
    if (b == NEG) return a;
    return (a > b ? a : b) + log1p(exp(-fabs(a - b)));
}

// order-preserving image of a double that is neither NaN nor -0.0
__device__ __forceinline__ u64 key_image(double k) {
    const u64 b = (u64)__double_as_longlong(k);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ u64 hash_step(u64 h, int c) {
    h = (h ^ (u64)(c + 1)) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// a node as the whole block sees it (past this CU's vector cache: the walk may have cached a neighbour of a later node)
__device__ __forceinline__ u64 node_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// do nodes x and y, of equal depth, spell the same prefix?
__device__ __forceinline__ bool same_prefix(const u64* __restrict__ nodes, int x, int y) {
    while (x != y) {
        if (x <= 0 || y <= 0) return false;
        const u64 vx = node_load(nodes + x), vy = node_load(nodes + y);
        if ((uint32_t)vx != (uint32_t)vy) return false;
        x = (int)(vx >> 32);
        y = (int)(vy >> 32);
    }
    return true;
}

__device__ __forceinline__ int select_digit(u64 img, int idx, int pass) {
    if (pass < 8) return (int)(img >> (56 - 8 * pass)) & 255;
    const int inv = 0xffff - idx;
    return pass == 8 ? inv >> 8 : inv & 255;
}

// lookup(s, w) of the compiled word model: log P(w | context s) with the backoff weights added in order, and the next state
__device__ __forceinline__ double word_lookup(const w2v2_word_lm& L, int s, int w, int* next) {
    double acc = 0.0;
    for (int hop = 0; hop < W2V2_WORDLM_MAX_ORDER && s != 0; ++hop) {          // (a context has at most order - 1 words)
        int lo = L.arc0_dev[s], hi = L.arc0_dev[s + 1];
        while (lo < hi) {
            const int mid = (lo + hi) >> 1, aw = L.arc_word_dev[mid];
            if (aw == w) {
                *next = L.arc_next_dev[mid];
                return __dadd_rn(acc, (double)L.arc_logp_dev[mid]);
            }
            if (aw < w) lo = mid + 1;
            else hi = mid;
        }
        acc = __dadd_rn(acc, (double)L.bo_dev[s]);
        s = L.bstate_dev[s];
    }
    const int i = L.arc0_dev[0] + w;                                            // state 0 holds every word, in order
    *next = L.arc_next_dev[i];
    return __dadd_rn(acc, (double)L.arc_logp_dev[i]);
}

// the c == d rule for an entry (wnode, lmstate, lm): lm and lmstate of the prefix + d; state -1: dropped
__device__ __forceinline__ void word_end(const BeamWordArgs& a, int wn, int st, double lm, double* lmo, int* sto) {
    *lmo = lm;
    *sto = st;
    if (wn == 0) return;
    int w = wn > 0 ? a.w.word_at_dev[wn] : -1;
    const bool unk = w < 0;
    if (unk) {
        if (a.constrained) {
            *sto = -1;
            return;
        }
        w = a.w.unk;
    }
    double lp = word_lookup(a.w, st, w, sto);
    if (unk) lp = __dadd_rn(lp, a.unk_penalty);
    *lmo = __dadd_rn(__dadd_rn(lm, __dmul_rn(a.alpha, lp)), a.beta);
}

// WORD: the word n-gram model with a lexicon in place of the character table (the header's second part)
// BIAS: a phrase bias on top of either (the header's third part)
// STREAM: the resumable instance (the header's fourth part); what it does sits under `if constexpr (STREAM)`, and the few values it
// shares with the common code (done, results, fresh) are compile-time constants when STREAM is false
template <bool WORD, bool BIAS, bool STREAM>
__global__ __launch_bounds__(BEAM_NT) void beam_search_kernel(BeamKernelArgs<WORD, BIAS, STREAM> a) {
    constexpr double NEG = -__builtin_inf();
    using Buf = std::conditional_t<WORD, BeamBufWord, BeamBuf>;
    __shared__ Buf buf[2];
    __shared__ int s_wn[WORD ? BEAM_W : 1], s_st[WORD ? BEAM_W : 1];      // (WORD) wnode and lmstate of the survivors
    __shared__ int bst[2][BIAS ? BEAM_W : 1], s_bst[BIAS ? BEAM_W : 1];   // (BIAS) bias state of the entries (half t & 1) and of the survivors' parents
    __shared__ double lpr[2][BEAM_RING][BEAM_V];            // lp of frames 8 (t / 8) + r, half (t / 8) & 1
    __shared__ u64 childmask[BEAM_W];
    __shared__ double spb[BEAM_W], spnb[BEAM_W], stot[BEAM_W], skey[BEAM_W];      // the stay candidates of a step
    __shared__ u64 s_img[BEAM_W];                           // the survivors of a step, compacted (not yet in key order)
    __shared__ int s_idx[BEAM_W];
    __shared__ double s_pb[BEAM_W], s_pnb[BEAM_W], s_tot[BEAM_W], s_lm[BEAM_W];
    __shared__ __attribute__((aligned(16))) int hist[3][256];
    __shared__ int wtot[BEAM_NT / 64];

    const BeamSeg sg = a.segs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, W = a.W, blank = a.blank, T = sg.T, nbest = a.nbest;
    const float* __restrict__ lg = a.logits + sg.row0 * V;
    const double* __restrict__ ls = a.lse + sg.lse0;
    u64* __restrict__ nodes = a.nodes + sg.node0;
    const float* __restrict__ lmt = a.lm;
    const double alpha = a.alpha, beta = a.beta;
    int32_t* __restrict__ out_lab = a.labels + (int64_t)blockIdx.x * nbest * a.max_len;
    const int64_t out0 = (int64_t)blockIdx.x * nbest;

    // (STREAM) the slab, the frames behind this stream, the stable prefix the previous call left, and whether results are wanted
    char* slab = nullptr;
    int32_t* hdr = nullptr;
    int done = 0, st_len = 0, st_node = 0;
    bool results = true;
    bool bad = false;
    if constexpr (STREAM) {
        slab = a.state + (int64_t)blockIdx.x * BEAM_STATE_BYTES;
        hdr = reinterpret_cast<int32_t*>(slab);
        done = sg.done;
        results = a.labels != nullptr;
        if (done > 0) {
            bad = hdr[1] != 0;                              // the sticky dead flag
            st_len = hdr[2];
            st_node = hdr[3];
        }
    }
    for (int t = tid; t < T; t += BEAM_NT) bad |= !(fabs(ls[t]) <= 1.7976931348623157e308);
    const int anybad = __syncthreads_or(bad);
    if (results)
        for (int i = tid; i < nbest * a.max_len; i += BEAM_NT) out_lab[i] = -1;
    if (anybad) {                                           // (block-uniform)
        if constexpr (STREAM) {                             // dead from here on: nothing advances, the stable prefix stays
            if (tid == 0) {
                if (done == 0) hdr[0] = 0;
                hdr[1] = 1;
                hdr[2] = st_len;
                hdr[3] = st_node;
                a.stable_len[blockIdx.x] = st_len;
            }
        }
        if (results && tid < nbest) {
            a.length[out0 + tid] = -1;
            a.score[out0 + tid] = __builtin_nan("");
            a.total[out0 + tid] = __builtin_nan("");
        }
        return;
    }

    // this thread's candidates: index k 256 + tid = j V + c, packed j << 8 | c; its elements of a ring half: e = q 256 + tid = r V + c
    int jc[BEAM_KMAX];
#pragma unroll
    for (int k = 0; k < BEAM_KMAX; ++k) {
        const int idx = k * BEAM_NT + tid, j = idx / V;
        jc[k] = j << 8 | (idx - j * V);
    }
    int er[2], ec[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = q * BEAM_NT + tid;
        er[q] = e / V;
        ec[q] = e - er[q] * V;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (er[q] < BEAM_RING && er[q] < T) lpr[0][er[q]][ec[q]] = (double)lg[(int64_t)er[q] * V + ec[q]] - ls[er[q]];
    const bool fresh = !STREAM || done == 0;
    if (tid == 0 && fresh) {
        Buf& B = buf[0];
        B.pb[0] = 0.0;
        B.pnb[0] = NEG;
        B.tot[0] = 0.0;
        B.lm[0] = 0.0;
        B.h[0] = 0x243F6A8885A308D3ull;
        B.hp[0] = 0;
        B.node[0] = 0;
        B.pn[0] = -1;
        B.len[0] = 0;
        B.last[0] = -1;
        int ctx = 0;
        for (int m = 1; m < a.ctxmod; m *= V) ctx = ctx * V + blank;
        B.ctx[0] = ctx;
        B.mi[0] = -1;
        if constexpr (WORD) {
            B.wnode[0] = 0;
            B.lmstate[0] = a.w.start_state;
            B.dlm[0] = 0.0;
            B.dstate[0] = a.w.start_state;
        }
        if constexpr (BIAS) bst[0][0] = a.bstart;
    }
    int nb = 1;
    if constexpr (STREAM) {
        if (!fresh) {                                       // the beam as the previous call left it, into half 0
            const u64_alias* src = reinterpret_cast<const u64_alias*>(slab + BEAM_STATE_BUF);
            u64_alias* dst = reinterpret_cast<u64_alias*>(&buf[0]);
            for (int i = tid; i < (int)(sizeof(Buf) / 8); i += BEAM_NT) dst[i] = src[i];
            if constexpr (BIAS)
                if (tid < BEAM_W) bst[0][tid] = reinterpret_cast<const int*>(slab + BEAM_STATE_BST)[tid];
            nb = min(max(hdr[0], 0), BEAM_W);
        }
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        Buf& B = buf[t & 1];
        Buf& N = buf[(t & 1) ^ 1];
        const double* lp = lpr[(t >> 3) & 1][t & 7];
        const int nk = (nb * V + BEAM_NT - 1) / BEAM_NT;

        // the ring half of the next 8 frames: loaded now, written at the end of this step
        float pfx[2] = {0.f, 0.f};
        double pfl[2] = {0.0, 0.0};
        const bool fill = (t & 7) == 0;
        if (fill) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int tt = t + BEAM_RING + er[q];
                if (er[q] < BEAM_RING && tt < T) {
                    pfx[q] = lg[(int64_t)tt * V + ec[q]];
                    pfl[q] = ls[tt];
                }
            }
        }
        // the language model's values of this thread's candidates
        // (WORD: their lexicon nodes: the child of the entry's node, -2 outside the lexicon, -1 dropped)
        // (BIAS: their increments delta[bst, c], used after the match)
        float lmv[BEAM_KMAX];
        int wch[BEAM_KMAX];
        float bdl[BIAS ? BEAM_KMAX : 1];
#pragma unroll
        for (int k = 0; k < BEAM_KMAX; ++k) {
            lmv[k] = 0.f;
            wch[k] = -2;
            if constexpr (BIAS) {
                bdl[k] = 0.f;
                if (k < nk) {
                    const int j = jc[k] >> 8, c = jc[k] & 255;
                    if (j < nb && c != blank) bdl[k] = a.bdelta[bst[t & 1][j] * V + c];
                }
            }
            if constexpr (WORD) {
                if (k < nk) {
                    const int j = jc[k] >> 8, c = jc[k] & 255;
                    if (j < nb && c != blank && c != a.delim) {
                        const int wn = B.wnode[j];
                        if (wn >= 0) {
                            const int ch = a.w.child_dev[(int64_t)wn * V + c];
                            wch[k] = ch >= 0 ? ch : a.constrained ? -1 : -2;
                        }
                    }
                }
            } else if (lmt && k < nk) {
                const int j = jc[k] >> 8, c = jc[k] & 255;
                if (j < nb && c != blank) lmv[k] = lmt[(int64_t)B.ctx[j] * V + c];
            }
        }
        hist[0][tid] = 0;

        // (1) match: entry i against every entry j; j is a child of i iff its prefix is i's plus one label
        {
            const int i = tid >> 2, part = tid & 3;
            u64 mask = 0;
            if (i < nb) {
                const u64 hi = B.h[i];
                const int li = B.len[i] + 1, ni = B.node[i];
                for (int j = part; j < nb; j += 4) {
                    if (B.len[j] == li && B.hp[j] == hi) {
                        bool ok = B.pn[j] == ni;
                        if (!ok) {
                            ok = same_prefix(nodes, B.pn[j], ni);
                            if (ok) B.pn[j] = ni;
                        }
                        if (ok) {
                            B.mi[j] = i;
                            mask |= 1ull << B.last[j];
                        }
                    }
                }
            }
            mask |= __shfl_xor(mask, 1, 64);
            mask |= __shfl_xor(mask, 2, 64);
            if (part == 0) childmask[i] = mask;
        }
        lds_barrier();

        // (2) keys: the extensions by every thread, the stays by wave 0
        u64 img[BEAM_KMAX];
        unsigned valid = 0;
#pragma unroll
        for (int k = 0; k < BEAM_KMAX; ++k) {
            img[k] = 0;
            if (k < nk) {
                const int j = jc[k] >> 8, c = jc[k] & 255;
                if (j < nb && c != blank && !((childmask[j] >> c) & 1ull)) {
                    const double base = c == B.last[j] ? B.pb[j] : B.tot[j];
                    const double pnbn = base + lp[c];
                    double lmn;
                    bool keep = true;
                    if constexpr (WORD) {
                        if (c == a.delim) {
                            lmn = B.dlm[j];
                            keep = B.dstate[j] >= 0;
                        } else {
                            lmn = B.lm[j];
                            keep = wch[k] != -1;
                        }
                    } else {
                        lmn = __dadd_rn(__dadd_rn(B.lm[j], __dmul_rn(alpha, (double)lmv[k])), beta);
                    }
                    if constexpr (BIAS) lmn = __dadd_rn(lmn, (double)bdl[k]);
                    const double key = (pnbn + lmn) + 0.0;
                    if (key > NEG && keep) {
                        img[k] = key_image(key);
                        valid |= 1u << k;
                    }
                }
            }
        }
        if (tid < nb) {
            const int j = tid, last = B.last[j], i = B.mi[j];
            const double pbn = B.tot[j] + lp[blank];
            double pnbn = last >= 0 ? B.pnb[j] + lp[last] : NEG;
            if (i >= 0) pnbn = beam_lse2(pnbn, (last == B.last[i] ? B.pb[i] : B.tot[i]) + lp[last]);
            const double totn = beam_lse2(pbn, pnbn);
            spb[j] = pbn;
            spnb[j] = pnbn;
            stot[j] = totn;
            skey[j] = (totn + B.lm[j]) + 0.0;
        }
        lds_barrier();
#pragma unroll
        for (int k = 0; k < BEAM_KMAX; ++k) {
            if (k < nk) {
                const int j = jc[k] >> 8, c = jc[k] & 255;
                if (j < nb && c == blank) {
                    const double key = skey[j];
                    if (key > NEG) {
                        img[k] = key_image(key);
                        valid |= 1u << k;
                    }
                }
            }
        }

        // (3) exact radix select of the min(W, valid) largest composites (image, 0xffff - index)
        unsigned active = valid, acc = 0;
        int need = 0, nsel = 0;
        for (int pass = 0; pass < 10; ++pass) {
            int* H = hist[pass % 3];
            hist[(pass + 1) % 3][tid] = 0;
#pragma unroll
            for (int k = 0; k < BEAM_KMAX; ++k)
                if (active >> k & 1u) atomicAdd(&H[select_digit(img[k], k * BEAM_NT + tid, pass)], 1);
            lds_barrier();
            const int4 hv = reinterpret_cast<const int4*>(H)[lane];      // bins 4 lane .. 4 lane + 3
            const int s = hv.x + hv.y + hv.z + hv.w;
            int suf = s;                                                  // sum over the lanes >= this one
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_down(suf, off, 64);
                if (lane + off < 64) suf += v;
            }
            if (pass == 0) {
                need = min(W, __shfl(suf, 0, 64));
                nsel = need;
            }
            if (need == 0) break;                                         // (block-uniform)
            const int above = suf - s;
            const int L = __ffsll((long long)__ballot(above < need && need <= suf)) - 1;      // exactly one lane
            const int h3 = __shfl(hv.w, L, 64), h2 = __shfl(hv.z, L, 64), h1 = __shfl(hv.y, L, 64), h0 = __shfl(hv.x, L, 64);
            int cum = __shfl(above, L, 64), d, hd;
            if (cum + h3 >= need) { d = 4 * L + 3; hd = h3; }
            else if (cum + h3 + h2 >= need) { cum += h3; d = 4 * L + 2; hd = h2; }
            else if (cum + h3 + h2 + h1 >= need) { cum += h3 + h2; d = 4 * L + 1; hd = h1; }
            else { cum += h3 + h2 + h1; d = 4 * L; hd = h0; }
            need -= cum;
            const bool all = hd == need;                                  // the boundary bin is taken whole: done
#pragma unroll
            for (int k = 0; k < BEAM_KMAX; ++k) {
                if (active >> k & 1u) {
                    const int dg = select_digit(img[k], k * BEAM_NT + tid, pass);
                    if (dg > d || (dg == d && all)) acc |= 1u << k;
                    if (dg != d || all) active &= ~(1u << k);
                }
            }
            if (all) break;                                               // (block-uniform)
        }

        // (4) the survivors compacted, then their ranks, then the next beam
        {
            int mine = 0;
#pragma unroll
            for (int k = 0; k < BEAM_KMAX; ++k) mine += __popcll(__ballot(acc >> k & 1u));
            if (lane == 0) wtot[wave] = mine;
        }
        lds_barrier();
        {
            // distinct slots 0 .. nsel - 1, fixed by the indices alone; the ranks below put them in key order
            int before_k = 0;
#pragma unroll
            for (int k = 0; k < BEAM_KMAX; ++k) {
                if (k < nk) {                                             // (block-uniform)
                    const bool f = acc >> k & 1u;
                    const u64 bl = __ballot(f);
                    if (f) {                                              // (wave w fills the slots behind the earlier waves')
                        int slot = before_k + __popcll(bl & ((1ull << lane) - 1ull));
                        for (int w = 0; w < wave; ++w) slot += wtot[w];
                        slot = min(slot, BEAM_W - 1);
                        const int j = jc[k] >> 8, c = jc[k] & 255;
                        s_img[slot] = img[k];
                        s_idx[slot] = k * BEAM_NT + tid;
                        if (c == blank) {
                            s_pb[slot] = spb[j];
                            s_pnb[slot] = spnb[j];
                            s_tot[slot] = stot[j];
                            s_lm[slot] = B.lm[j];
                        } else {
                            const double pnbn = (c == B.last[j] ? B.pb[j] : B.tot[j]) + lp[c];
                            s_pb[slot] = NEG;
                            s_pnb[slot] = pnbn;
                            s_tot[slot] = pnbn;
                            if constexpr (WORD) {
                                const bool ends = c == a.delim;
                                s_lm[slot] = ends ? B.dlm[j] : B.lm[j];
                                s_wn[slot] = ends ? 0 : wch[k];
                                s_st[slot] = ends ? B.dstate[j] : B.lmstate[j];
                            } else {
                                s_lm[slot] = __dadd_rn(__dadd_rn(B.lm[j], __dmul_rn(alpha, (double)lmv[k])), beta);
                            }
                            if constexpr (BIAS) {
                                s_lm[slot] = __dadd_rn(s_lm[slot], (double)bdl[k]);
                                s_bst[slot] = bst[t & 1][j];
                            }
                        }
                    }
                    before_k += __popcll(bl);
                }
            }
        }
        lds_barrier();
        {
            const int r = tid >> 2, part = tid & 3;
            int cnt = 0;
            if (r < nsel) {
                const u64 my = s_img[r];
                const int myi = s_idx[r];
                for (int q = part; q < nsel; q += 4) {
                    const u64 o = s_img[q];
                    cnt += (o > my || (o == my && s_idx[q] < myi)) ? 1 : 0;
                }
            }
            cnt += __shfl_xor(cnt, 1, 64);
            cnt += __shfl_xor(cnt, 2, 64);
            if (part == 0 && r < nsel) {
                const int idx = s_idx[r], j = idx / V, c = idx - j * V;
                N.pb[cnt] = s_pb[r];
                N.pnb[cnt] = s_pnb[r];
                N.tot[cnt] = s_tot[r];
                N.lm[cnt] = s_lm[r];
                N.mi[cnt] = -1;
                if (c == blank) {
                    N.h[cnt] = B.h[j];
                    N.hp[cnt] = B.hp[j];
                    N.node[cnt] = B.node[j];
                    N.pn[cnt] = B.pn[j];
                    N.len[cnt] = B.len[j];
                    N.last[cnt] = B.last[j];
                    N.ctx[cnt] = B.ctx[j];
                    if constexpr (WORD) {
                        N.wnode[cnt] = B.wnode[j];
                        N.lmstate[cnt] = B.lmstate[j];
                        N.dlm[cnt] = B.dlm[j];
                        N.dstate[cnt] = B.dstate[j];
                    }
                    if constexpr (BIAS) bst[(t & 1) ^ 1][cnt] = bst[t & 1][j];
                } else {
                    int node = 1 + t * W + cnt;
                    if constexpr (STREAM) node = 1 + (done + t) * W + cnt;
                    nodes[node] = (u64)(uint32_t)B.node[j] << 32 | (u64)(uint32_t)c;
                    N.h[cnt] = hash_step(B.h[j], c);
                    N.hp[cnt] = B.h[j];
                    N.node[cnt] = node;
                    N.pn[cnt] = B.node[j];
                    N.len[cnt] = B.len[j] + 1;
                    N.last[cnt] = c;
                    N.ctx[cnt] = (B.ctx[j] * V + c) % a.ctxmod;
                    if constexpr (WORD) {                     // the word-end rule of the new prefix, once (see the header)
                        double dl;
                        int ds;
                        word_end(a, s_wn[r], s_st[r], s_lm[r], &dl, &ds);
                        N.wnode[cnt] = s_wn[r];
                        N.lmstate[cnt] = s_st[r];
                        N.dlm[cnt] = dl;
                        N.dstate[cnt] = ds;
                    }
                    if constexpr (BIAS) bst[(t & 1) ^ 1][cnt] = a.bnext[s_bst[r] * V + c];      // the new prefix' state, once
                }
            }
        }
        if (fill) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int tt = t + BEAM_RING + er[q];
                if (er[q] < BEAM_RING && tt < T) lpr[((t >> 3) + 1) & 1][er[q]][ec[q]] = (double)pfx[q] - pfl[q];
            }
        }
        nb = nsel;
        __syncthreads();                                    // (also drains this step's node stores)
    }

    if constexpr (STREAM) {
        // the state for the next call (plain vector stores), then the stable prefix; the finalisation below only reads the beam
        {
            const u64_alias* src = reinterpret_cast<const u64_alias*>(&buf[T & 1]);
            u64_alias* dst = reinterpret_cast<u64_alias*>(slab + BEAM_STATE_BUF);
            for (int i = tid; i < (int)(sizeof(Buf) / 8); i += BEAM_NT) dst[i] = src[i];
            if constexpr (BIAS)
                if (tid < BEAM_W) reinterpret_cast<int*>(slab + BEAM_STATE_BST)[tid] = bst[T & 1][tid];
        }
        if (wave == 0) {
            // the longest common prefix of the entries' label strings: every entry begins with the previous call's stable prefix
            // (st_len labels), so the chains are compared from the shortest entry's depth back to depth st_len only.  Labels are
            // compared, not nodes (a prefix made twice has two nodes); once all chains stand on ONE node the rest is common.
            const Buf& B = buf[T & 1];
            const bool on = lane < nb;
            int n = on ? B.node[lane] : 0, d = on ? B.len[lane] : 0x7fffffff;
            int minlen = d;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) minlen = min(minlen, __shfl_xor(minlen, off, 64));
            int cand = st_len, sn = st_node;
            if (nb > 0) {                                   // (wave-uniform)
                while (d > minlen && n > 0) {
                    n = (int)(node_load(nodes + n) >> 32);
                    --d;
                }
                cand = minlen;
                sn = __shfl(n, 0, 64);
                for (int dd = minlen; dd > st_len; --dd) {
                    const int n0 = __shfl(n, 0, 64);
                    if (__ballot(on && n != n0) == 0) break;
                    const u64 v = on && n > 0 ? node_load(nodes + n) : 0;
                    const int lab = (int)(uint32_t)v, par = (int)(v >> 32);
                    const int lab0 = __shfl(lab, 0, 64), par0 = __shfl(par, 0, 64);
                    if (__ballot(on && lab != lab0) != 0) {
                        cand = dd - 1;
                        sn = par0;
                    }
                    n = par;
                }
            }
            if (lane == 0) {
                hdr[0] = nb;
                hdr[1] = 0;
                hdr[2] = cand;
                hdr[3] = sn;
                a.stable_len[blockIdx.x] = cand;
            }
        }
        if (!results) return;
    }
    if constexpr (WORD || BIAS) {
        // finalisation (wave 0: W <= 64): the open word ended, eos, the bias' end-of-utterance term, then the entries in descending
        // total, equal totals by beam rank
        if (wave != 0) return;
        const Buf& B = buf[T & 1];
        bool ok = lane < nb;
        if constexpr (WORD) ok = ok && B.dstate[lane] >= 0;
        double tot = 0.0;
        if (ok) {
            double fin;
            if constexpr (WORD) {
                fin = B.dlm[lane];
                if (a.score_eos && a.w.eos >= 0) {
                    int nx;
                    fin = __dadd_rn(fin, __dmul_rn(alpha, word_lookup(a.w, B.dstate[lane], a.w.eos, &nx)));
                }
            } else {
                fin = B.lm[lane];
            }
            if constexpr (BIAS) fin = __dadd_rn(fin, (double)a.bfinal[bst[T & 1][lane]]);
            tot = B.tot[lane] + fin;
        }
        int rank = 0;
        for (int q = 0; q < nb; ++q) {
            const double tq = __shfl(tot, q, 64);
            const int okq = __shfl((int)ok, q, 64);
            rank += (okq && (tq > tot || (tq == tot && q < lane))) ? 1 : 0;
        }
        const int nfin = __popcll(__ballot(ok));
        if (ok && rank < nbest) {
            const int len = B.len[lane];
            a.length[out0 + rank] = len;
            a.score[out0 + rank] = B.tot[lane];
            a.total[out0 + rank] = tot;
            int n = B.node[lane];
            for (int k = len - 1; k >= 0 && n > 0; --k) {
                const u64 v = node_load(nodes + n);
                out_lab[(int64_t)rank * a.max_len + k] = (int32_t)(uint32_t)v;
                n = (int)(v >> 32);
            }
        }
        if (lane >= nfin && lane < nbest) {
            a.length[out0 + lane] = -1;
            a.score[out0 + lane] = __builtin_nan("");
            a.total[out0 + lane] = __builtin_nan("");
        }
        return;
    }
    // results: the first nbest entries, their labels walked back to the root
    if (tid < nbest) {
        const Buf& B = buf[T & 1];
        if (tid < nb) {
            const int len = B.len[tid];
            a.length[out0 + tid] = len;
            a.score[out0 + tid] = B.tot[tid];
            a.total[out0 + tid] = B.tot[tid] + B.lm[tid];
            int n = B.node[tid];
            for (int k = len - 1; k >= 0 && n > 0; --k) {
                const u64 v = node_load(nodes + n);
                out_lab[(int64_t)tid * a.max_len + k] = (int32_t)(uint32_t)v;
                n = (int)(v >> 32);
            }
        } else {
            a.length[out0 + tid] = -1;
            a.score[out0 + tid] = __builtin_nan("");
            a.total[out0 + tid] = __builtin_nan("");
        }
    }
}

// what the resumable entry adds to a call: per stream the frames already searched, the state slab and the trie's place and room
struct BeamStreamCall {
    const int64_t* frames_done;
    void* state;
    u64* nodes;
    const int64_t* node0;
    const int64_t* node_cap;
    int32_t* stable_len;
};

template <bool WORD, bool BIAS, class Args>
void beam_launch_stream(const Args& form, const BeamStreamCall& sc, int n, hipStream_t s) {
    BeamStreamArgs<Args> b{};
    static_cast<Args&>(b) = form;
    b.state = static_cast<char*>(sc.state);
    b.stable_len = sc.stable_len;
    W2V2_LAUNCH((beam_search_kernel<WORD, BIAS, true>), dim3((unsigned)n), dim3(BEAM_NT), 0, s, b);
}

// the checks, the workspace and the launches the entries share; `a` arrives with its language model fields set; `bias` (checked by
// the caller) or null; `sc`: the resumable entry's arguments, null for the entries that search whole utterances
int beam_run(BeamWordArgs& a, bool word, const w2v2_ctc_bias* bias, const float* logits, int V, int n, const int64_t* row0,
             const int32_t* frames, int blank, int beam_width, int nbest, float lm_alpha, float lm_beta, int max_len,
             int32_t* labels_out, int32_t* length, double* score, double* total, hipStream_t s, const BeamStreamCall* sc = nullptr) {
    W2V2_REQUIRE(logits && row0 && frames && (labels_out || sc) && ((length && score && total) || (sc && !labels_out)),
                 "ctc_beam_search: null argument");
    W2V2_REQUIRE(!sc || (sc->frames_done && sc->state && sc->nodes && sc->node0 && sc->node_cap && sc->stable_len),
                 "ctc_beam_search_stream: null argument");
    W2V2_REQUIRE(n >= 1, "ctc_beam_search: %d utterances (need at least one)", n);
    W2V2_REQUIRE(V >= 1 && V <= W2V2_BEAM_MAX_VOCAB, "ctc_beam_search: vocabulary of %d entries; 1 to %d", V, W2V2_BEAM_MAX_VOCAB);
    W2V2_REQUIRE(blank >= 0 && blank < V, "ctc_beam_search: blank index %d outside vocabulary %d", blank, V);
    W2V2_REQUIRE(beam_width >= 1 && beam_width <= W2V2_BEAM_MAX_WIDTH, "ctc_beam_search: beam width %d; 1 to %d", beam_width,
                 W2V2_BEAM_MAX_WIDTH);
    W2V2_REQUIRE(nbest >= 1 && nbest <= beam_width, "ctc_beam_search: nbest %d outside [1, beam width %d]", nbest, beam_width);
    W2V2_REQUIRE(std::isfinite(lm_alpha) && std::isfinite(lm_beta), "ctc_beam_search: language model weights must be finite");
    int Tmax = 0;           // the longest utterance of the call
    int64_t Lmax = 0;       // the most frames a hypothesis can span: with `sc`, the earlier calls' frames included
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(row0[i] >= 0, "ctc_beam_search: utterance %d has a negative offset", i);
        if (sc) {
            const int64_t done = sc->frames_done[i];
            W2V2_REQUIRE(frames[i] >= 0, "ctc_beam_search_stream: stream %d is given %d frames", i, frames[i]);
            W2V2_REQUIRE(done >= 0, "ctc_beam_search_stream: stream %d has %lld frames done", i, (long long)done);
            W2V2_REQUIRE(done < ((int64_t)1 << 31) && (done + frames[i]) * beam_width < ((int64_t)1 << 31) - 1,
                         "ctc_beam_search_stream: stream %d has too many frames (%lld done and %d new)", i, (long long)done, frames[i]);
            W2V2_REQUIRE(sc->node0[i] >= 0, "ctc_beam_search_stream: stream %d has a negative node offset", i);
            W2V2_REQUIRE((done + frames[i]) * beam_width + 1 <= sc->node_cap[i],
                         "ctc_beam_search_stream: stream %d needs %lld trie nodes after this call, its buffer holds %lld", i,
                         (long long)((done + frames[i]) * beam_width + 1), (long long)sc->node_cap[i]);
            Lmax = std::max(Lmax, done + frames[i]);
        } else {
            W2V2_REQUIRE(frames[i] >= 1, "ctc_beam_search: utterance %d has %d frames (need at least one)", i, frames[i]);
            W2V2_REQUIRE((int64_t)frames[i] * beam_width < ((int64_t)1 << 31) - 1, "ctc_beam_search: utterance %d has too many frames (%d)",
                         i, frames[i]);
            Lmax = std::max(Lmax, (int64_t)frames[i]);
        }
        Tmax = std::max(Tmax, (int)frames[i]);
    }
    if (labels_out) {
        W2V2_REQUIRE(max_len >= Lmax, "ctc_beam_search: max_len %d below the longest utterance's %lld frames", max_len, (long long)Lmax);
        W2V2_REQUIRE((int64_t)nbest * max_len < ((int64_t)1 << 31), "ctc_beam_search: nbest * max_len = %d * %d does not fit 31 bits", nbest,
                     max_len);
    }
    std::vector<BeamSeg> segs((size_t)n);
    int64_t out = 0, nn = 0;
    for (int i = 0; i < n; ++i) {
        segs[i] = BeamSeg{row0[i], out, sc ? sc->node0[i] : nn, frames[i], sc ? (int32_t)sc->frames_done[i] : 0};
        out += frames[i];
        if (!sc) nn += (int64_t)frames[i] * beam_width + 1;
    }
    // workspace: the table | lse (fp64, sum T_i) | trie nodes (sum T_i W + 1; with `sc` the caller's buffers hold them)
    const size_t tab_bytes = up256((size_t)n * sizeof(BeamSeg)), lse_bytes = up256((size_t)out * sizeof(double));
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_BEAM, s, tab_bytes + lse_bytes + (size_t)nn * sizeof(u64), &raw)) return e;
    a.logits = logits;
    a.segs = static_cast<const BeamSeg*>(raw);
    a.lse = reinterpret_cast<double*>(static_cast<char*>(raw) + tab_bytes);
    a.nodes = sc ? sc->nodes : reinterpret_cast<u64*>(static_cast<char*>(raw) + tab_bytes + lse_bytes);
    a.labels = labels_out;
    a.length = length;
    a.score = score;
    a.total = total;
    a.alpha = (double)lm_alpha;
    a.beta = (double)lm_beta;
    a.V = V;
    a.blank = blank;
    a.W = beam_width;
    a.nbest = nbest;
    a.max_len = max_len;
    if (int e = staged_upload(SCRATCH_BEAM, s, raw, {{segs.data(), (size_t)n * sizeof(BeamSeg), 0}}, (size_t)16 << 10)) return e;
    // (work for the profile: about 4 fp64 operations per candidate and step; the logits read once by the lse pass)
    ProfScope ps(nullptr, FAM_CTC, 4.0 * (double)out * beam_width * V, 4.0 * (double)out * V, s);
    if (Tmax > 0) W2V2_LAUNCH(beam_lse_kernel, dim3((unsigned)((Tmax + 3) / 4), (unsigned)n), dim3(256), 0, s, a);     // (a stream call may bring no frame)
    if (bias && word) {
        BeamBiasArgs<BeamWordArgs> b{};
        static_cast<BeamWordArgs&>(b) = a;
        b.bnext = bias->next_dev, b.bdelta = bias->delta_dev, b.bfinal = bias->final_dev, b.bstart = bias->start_state;
        if (sc) beam_launch_stream<true, true>(b, *sc, n, s);
        else W2V2_LAUNCH((beam_search_kernel<true, true, false>), dim3((unsigned)n), dim3(BEAM_NT), 0, s, b);
    } else if (bias) {
        BeamBiasArgs<BeamArgs> b{};
        static_cast<BeamArgs&>(b) = a;
        b.bnext = bias->next_dev, b.bdelta = bias->delta_dev, b.bfinal = bias->final_dev, b.bstart = bias->start_state;
        if (sc) beam_launch_stream<false, true>(b, *sc, n, s);
        else W2V2_LAUNCH((beam_search_kernel<false, true, false>), dim3((unsigned)n), dim3(BEAM_NT), 0, s, b);
    } else if (word) {
        if (sc) beam_launch_stream<true, false>(a, *sc, n, s);
        else W2V2_LAUNCH((beam_search_kernel<true, false, false>), dim3((unsigned)n), dim3(BEAM_NT), 0, s, a);
    } else {
        if (sc) beam_launch_stream<false, false>(static_cast<const BeamArgs&>(a), *sc, n, s);
        else W2V2_LAUNCH((beam_search_kernel<false, false, false>), dim3((unsigned)n), dim3(BEAM_NT), 0, s, static_cast<const BeamArgs&>(a));
    }
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

// the character form's own check and its fields of `a`
int char_args(BeamWordArgs& a, int V, const float* lm_table, int lm_order) {
    W2V2_REQUIRE(lm_order >= 1 && lm_order <= 4, "ctc_beam_search: language model order %d; 1 to 4", lm_order);
    a.lm = lm_table;
    a.ctxmod = 1;
    if (lm_table && V >= 1 && V <= W2V2_BEAM_MAX_VOCAB)
        for (int k = 1; k < lm_order; ++k) a.ctxmod *= V;
    return W2V2_OK;
}

// the word form's own checks and its fields of `a`
int word_args(BeamWordArgs& a, int V, int blank, const w2v2_word_lm* lm, int delim, float unk_penalty, int score_eos) {
    W2V2_REQUIRE(lm, "ctc_beam_search_words: null language model");
    W2V2_REQUIRE(lm->child_dev && lm->word_at_dev && lm->arc0_dev && lm->arc_word_dev && lm->arc_logp_dev && lm->arc_next_dev &&
                     lm->bo_dev && lm->bstate_dev, "ctc_beam_search_words: null language model array");
    W2V2_REQUIRE(lm->n_nodes >= 1 && lm->n_states >= 1 && lm->n_arcs >= 1 && lm->n_words >= 1,
                 "ctc_beam_search_words: language model sizes must be positive (nodes %d, states %d, arcs %d, words %d)", lm->n_nodes,
                 lm->n_states, lm->n_arcs, lm->n_words);
    W2V2_REQUIRE(lm->order >= 1 && lm->order <= W2V2_WORDLM_MAX_ORDER, "ctc_beam_search_words: language model order %d; 1 to %d",
                 lm->order, W2V2_WORDLM_MAX_ORDER);
    W2V2_REQUIRE(V < 1 || (int64_t)lm->n_nodes * V < ((int64_t)1 << 31), "ctc_beam_search_words: lexicon of %d nodes times %d labels does not fit 31 bits",
                 lm->n_nodes, V);
    W2V2_REQUIRE(lm->start_state >= 0 && lm->start_state < lm->n_states, "ctc_beam_search_words: start state %d outside [0, %d)",
                 lm->start_state, lm->n_states);
    W2V2_REQUIRE(lm->unk >= 0 && lm->unk < lm->n_words, "ctc_beam_search_words: unk word %d outside [0, %d)", lm->unk, lm->n_words);
    W2V2_REQUIRE(lm->eos >= -1 && lm->eos < lm->n_words, "ctc_beam_search_words: eos word %d outside [-1, %d)", lm->eos, lm->n_words);
    W2V2_REQUIRE(lm->n_arcs >= lm->n_words, "ctc_beam_search_words: %d arcs cannot hold the %d words of state 0", lm->n_arcs, lm->n_words);
    W2V2_REQUIRE(delim >= 0 && delim < V && delim != blank, "ctc_beam_search_words: word delimiter %d outside vocabulary %d or the blank", delim, V);
    W2V2_REQUIRE(!(unk_penalty != unk_penalty) && unk_penalty <= 0.f, "ctc_beam_search_words: unk_penalty must be <= 0 or -inf, not NaN");
    a.lm = nullptr;
    a.ctxmod = 1;
    a.w = *lm;
    a.constrained = std::isinf(unk_penalty) ? 1 : 0;
    a.unk_penalty = a.constrained ? 0.0 : (double)unk_penalty;
    a.delim = delim;
    a.score_eos = score_eos ? 1 : 0;
    return W2V2_OK;
}

}  // namespace

int launch_ctc_beam_search(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank, int beam_width,
                           int nbest, const float* lm_table, int lm_order, float lm_alpha, float lm_beta, int max_len,
                           int32_t* labels_out, int32_t* length, double* score, double* total, hipStream_t s) {
    BeamWordArgs a{};
    if (int e = char_args(a, V, lm_table, lm_order)) return e;
    return beam_run(a, false, nullptr, logits, V, n, row0, frames, blank, beam_width, nbest, lm_alpha, lm_beta, max_len, labels_out,
                    length, score, total, s);
}

int launch_ctc_beam_search_words(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank,
                                 int beam_width, int nbest, const w2v2_word_lm* lm, int delim, float lm_alpha, float lm_beta,
                                 float unk_penalty, int score_eos, int max_len, int32_t* labels_out, int32_t* length, double* score,
                                 double* total, hipStream_t s) {
    BeamWordArgs a{};
    if (int e = word_args(a, V, blank, lm, delim, unk_penalty, score_eos)) return e;
    return beam_run(a, true, nullptr, logits, V, n, row0, frames, blank, beam_width, nbest, lm_alpha, lm_beta, max_len, labels_out,
                    length, score, total, s);
}

int launch_ctc_beam_search_biased(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, int blank,
                                  int beam_width, int nbest, const float* lm_table, int lm_order, const w2v2_word_lm* word_lm, int delim,
                                  float lm_alpha, float lm_beta, float unk_penalty, int score_eos, const w2v2_ctc_bias* bias, int max_len,
                                  int32_t* labels_out, int32_t* length, double* score, double* total, hipStream_t s) {
    W2V2_REQUIRE(bias, "ctc_beam_search_biased: null bias");
    W2V2_REQUIRE(bias->next_dev && bias->delta_dev && bias->final_dev, "ctc_beam_search_biased: null bias array");
    W2V2_REQUIRE(bias->n_states >= 1 && bias->n_states <= W2V2_BIAS_MAX_STATES, "ctc_beam_search_biased: %d bias states; 1 to %d",
                 bias->n_states, W2V2_BIAS_MAX_STATES);
    W2V2_REQUIRE(bias->start_state >= 0 && bias->start_state < bias->n_states, "ctc_beam_search_biased: bias start state %d outside [0, %d)",
                 bias->start_state, bias->n_states);
    W2V2_REQUIRE(V < 1 || (int64_t)bias->n_states * V < ((int64_t)1 << 31),
                 "ctc_beam_search_biased: bias of %d states times %d labels does not fit 31 bits", bias->n_states, V);
    W2V2_REQUIRE(!(word_lm && lm_table), "ctc_beam_search_biased: both a word model and a character table given");
    BeamWordArgs a{};
    if (int e = word_lm ? word_args(a, V, blank, word_lm, delim, unk_penalty, score_eos) : char_args(a, V, lm_table, lm_order)) return e;
    return beam_run(a, word_lm != nullptr, bias, logits, V, n, row0, frames, blank, beam_width, nbest, lm_alpha, lm_beta, max_len,
                    labels_out, length, score, total, s);
}

int64_t ctc_beam_stream_state_bytes() { return BEAM_STATE_BYTES; }

int launch_ctc_beam_search_stream(const float* logits, int V, int n, const int64_t* row0, const int32_t* frames, const int64_t* frames_done,
                                  int blank, int beam_width, int nbest, const float* lm_table, int lm_order, const w2v2_word_lm* word_lm,
                                  int delim, float lm_alpha, float lm_beta, float unk_penalty, int score_eos, const w2v2_ctc_bias* bias,
                                  void* state, uint64_t* nodes, const int64_t* node0, const int64_t* node_cap, int max_len,
                                  int32_t* labels_out, int32_t* length, double* score, double* total, int32_t* stable_len, hipStream_t s) {
    if (bias) {
        W2V2_REQUIRE(bias->next_dev && bias->delta_dev && bias->final_dev, "ctc_beam_search_stream: null bias array");
        W2V2_REQUIRE(bias->n_states >= 1 && bias->n_states <= W2V2_BIAS_MAX_STATES, "ctc_beam_search_stream: %d bias states; 1 to %d",
                     bias->n_states, W2V2_BIAS_MAX_STATES);
        W2V2_REQUIRE(bias->start_state >= 0 && bias->start_state < bias->n_states, "ctc_beam_search_stream: bias start state %d outside [0, %d)",
                     bias->start_state, bias->n_states);
        W2V2_REQUIRE(V < 1 || (int64_t)bias->n_states * V < ((int64_t)1 << 31),
                     "ctc_beam_search_stream: bias of %d states times %d labels does not fit 31 bits", bias->n_states, V);
    }
    W2V2_REQUIRE(!(word_lm && lm_table), "ctc_beam_search_stream: both a word model and a character table given");
    BeamWordArgs a{};
    if (int e = word_lm ? word_args(a, V, blank, word_lm, delim, unk_penalty, score_eos) : char_args(a, V, lm_table, lm_order)) return e;
    const BeamStreamCall sc{frames_done, state, reinterpret_cast<u64*>(nodes), node0, node_cap, stable_len};
    return beam_run(a, word_lm != nullptr, bias, logits, V, n, row0, frames, blank, beam_width, nbest, lm_alpha, lm_beta, max_len,
                    labels_out, length, score, total, s, &sc);
}

}  // namespace w2v2
