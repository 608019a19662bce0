"""fp64 numpy reference of the CTC prefix beam search of csrc/beam.hip (w2v2_ctc_beam_search): the same definition, prefixes held as
tuples of labels (so "is p + c in the beam" is a dictionary lookup, independent of the kernel's trie and hashes).

Per frame, from every beam entry (p, pb, pnb, lm), tot = lse2(pb, pnb):
  stay on a blank   p     : pb'  = tot + lp(blank)
  repeat last label p     : pnb' = lse2(pnb', pnb + lp(p[-1]))
  extend by c       p + c : pnb' = lse2(pnb', (pb if c == p[-1] else tot) + lp(c)),  lm(p + c) = lm(p) + alpha table[ctx(p), c] + beta
A prefix occurs once among the candidates; candidate index j V + blank for the prefix already at rank j, j V + c for a new one made
from rank j.  Key lse2(pb', pnb') + lm; -inf keys drop; the W largest keys survive, equal keys by ascending index.

``search`` also returns the utterance's smallest decision margin (key of the last kept minus key of the first dropped candidate at
every step, and the gaps between adjacent entries of the final list up to the first one not returned) and the largest |key| seen:
what the GPU tests need to tell a legitimate rounding flip from an error."""

import itertools
import math

import numpy as np

NEG = -math.inf


def lse2(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def log_probs(x):
    """(T, V) fp64 log-softmax of fp32 logits, and the per-frame lse"""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=1, keepdims=True)
        lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    return x - lse[:, None], lse


def lm_context(prefix, V, blank, order):
    """row of the dense table for a prefix: its last order - 1 labels as digits base V, oldest first, blank-filled"""
    ctx = 0
    if order > 1:
        h = ([blank] * (order - 1) + list(prefix))[-(order - 1):]
        for k in h:
            ctx = ctx * V + int(k)
    return ctx


class Result:
    """hyps: [(labels tuple, score, total)] best first; margin: smallest decision margin; kmax: largest |key| met; rejoined: how
    often an entry p + c met an entry p that had been pruned and made again since p + c was made (the kernel's trie then holds two
    nodes for p, and it has to compare label strings: the tests want inputs where that happens)"""

    def __init__(self, hyps, margin, kmax, bad=False, rejoined=0):
        self.hyps, self.margin, self.kmax, self.bad, self.rejoined = hyps, margin, kmax, bad, rejoined


def search(x, beam_width, nbest=1, blank=0, lm=None, order=1, alpha=0.0, beta=0.0):
    x = np.asarray(x, np.float32)
    T, V = x.shape
    lp, lse = log_probs(x)
    if not np.isfinite(lse).all():                           # a NaN or +inf logit (or a frame of -inf only): no hypothesis
        return Result([], math.inf, 0.0, bad=True)
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    table = None if lm is None else np.asarray(lm, np.float32).astype(np.float64).reshape(-1, V)
    W = int(beam_width)
    beam = [((), 0.0, NEG, 0.0)]                             # (prefix, pb, pnb, lm)
    margin, kmax = math.inf, 0.0
    born = {(): -1}                                          # prefix -> step it was last made at
    parent_born = {}                                         # prefix in the beam -> `born` of its parent when it was made / last met
    rejoined = 0
    cols = np.arange(V)
    for t in range(T):
        row = lp[t]
        nb = len(beam)
        rank = {e[0]: j for j, e in enumerate(beam)}
        tots = [lse2(e[1], e[2]) for e in beam]
        PB = np.full((nb, V), NEG)                           # candidate j V + c: pb', pnb', lm
        PNB = np.full((nb, V), NEG)
        LM = np.zeros((nb, V))
        with np.errstate(invalid="ignore"):
            for j, (p, pb, pnb, l) in enumerate(beam):
                last = p[-1] if p else -1
                PNB[j] = np.where(cols == last, pb, tots[j]) + row
                tv = 0.0 if table is None else table[lm_context(p, V, blank, order)]
                LM[j] = (l + alpha * tv) + beta
                PB[j, blank] = tots[j] + row[blank]
                PNB[j, blank] = pnb + row[last] if p else NEG
                LM[j, blank] = l
        for q, (p, pb, pnb, l) in enumerate(beam):           # p = p_i + c with p_i in the beam: one candidate, at q's index
            i = rank.get(p[:-1]) if p else None
            if i is not None:
                if parent_born[p] != born[p[:-1]]:
                    rejoined += 1
                    parent_born[p] = born[p[:-1]]
                PNB[q, blank] = lse2(PNB[q, blank], PNB[i, p[-1]])
                PNB[i, p[-1]] = NEG
        key = np.full(nb * V, NEG)
        for j in range(nb):
            key[j * V + blank] = lse2(PB[j, blank], PNB[j, blank]) + LM[j, blank]
        ext = np.ones((nb, V), bool)
        ext[:, blank] = False
        flat = ext.ravel()
        key[flat] = (PNB.ravel() + LM.ravel())[flat]         # pb' = -inf there: lse2(pb', pnb') = pnb'
        key = key + 0.0
        order_ = np.argsort(-key, kind="stable")             # equal keys: ascending candidate index
        nvalid = int((key > NEG).sum())
        keep = order_[:min(W, nvalid)]
        if nvalid > W:
            margin = min(margin, float(key[order_[W - 1]] - key[order_[W]]))
        if nvalid:
            kmax = max(kmax, abs(float(key[keep[0]])), abs(float(key[keep[-1]])))
        nxt = []
        for idx in keep:
            j, c = divmod(int(idx), V)
            p = beam[j][0] if c == blank else beam[j][0] + (c,)
            if c != blank:
                born[p] = t
                parent_born[p] = born[beam[j][0]]
            nxt.append((p, float(PB[j, c]), float(PNB[j, c]), float(LM[j, c])))
        beam = nxt
    fin = [(p, lse2(pb, pnb), lse2(pb, pnb) + l) for p, pb, pnb, l in beam]
    for a, b in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[2] - b[2])
    return Result(fin[:nbest], margin, kmax, rejoined=rejoined)


def tau(T, kmax):
    """bound on the accumulated fp64 rounding of T steps, with a factor 16 for the library functions"""
    return 16.0 * T * 2.0 ** -52 * max(1.0, kmax)


def brute_force(x, blank=0, lm=None, order=1, alpha=0.0, beta=0.0):
    """every one of the V^T frame paths collapsed by the CTC rule: [(labels, score, total)] by descending total (ties: unordered)"""
    lp, _ = log_probs(x)
    T, V = lp.shape
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    table = None if lm is None else np.asarray(lm, np.float32).astype(np.float64).reshape(-1, V)
    d = {}
    for path in itertools.product(range(V), repeat=T):
        s = 0.0
        for t, c in enumerate(path):
            s += lp[t, c]
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        k = tuple(out)
        d[k] = lse2(d.get(k, NEG), s)
    res = []
    for k, s in d.items():
        l = 0.0
        for n in range(len(k)):
            tv = 0.0 if table is None else float(table[lm_context(k[:n], V, blank, order), k[n]])
            l = l + alpha * tv + beta
        res.append((k, s, s + l))
    res.sort(key=lambda z: -z[2])
    return res
