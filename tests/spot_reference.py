"""fp64 numpy reference of the CTC phrase search (w2v2_ctc_spot, wav2vec2.spotting): the definition in
include/w2v2.h, step by step, vectorised over the states so that 20 000 frames stay well under a second.  Every operation is the
kernel's: one fp64 compare-select (strict >) or add in the same order, so the results are compared bitwise.

``trace``        z_t, c_t of every frame of one (recording, phrase) pair, or None for a bad pair
``hit_pass``     the hits of a trace
``spot``         the kernel's outputs of one pair: (count, score (max_hits), begin, end, z, c)
``chunk_plan`` / ``chunked``   the overlapping pieces of find_phrases(chunk_frames=, overlap_frames=) and their merged hits
``brute_force``  max over all begins and all frame strings, for tiny shapes
"""

import itertools

import numpy as np

NEG = -np.inf


def emissions(x):
    """e_t(v) = (double)x_t(v) - (double)m_t with m_t the fp32 max of the frame; None for a recording with a NaN logit, a +inf
    logit or a frame whose max is -inf"""
    x = np.asarray(x, np.float32)
    if np.isnan(x).any() or (x == np.inf).any():
        return None
    m = x.max(axis=1)
    if (m == -np.inf).any():
        return None
    return x.astype(np.float64) - m.astype(np.float64)[:, None]


def trace(x, labels, blank, delim=-1):
    """(z (T,) float64, c (T,) int32) of the phrase in the recording; None for a bad recording or a bad label"""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    U = lab.size
    assert U >= 1
    if (lab < 0).any() or (lab >= V).any() or (lab == blank).any():
        return None
    e = emissions(x)
    if e is None:
        return None
    S = 2 * U - 1
    ext = np.full(S, blank, np.int64)
    ext[0::2] = lab
    skip = np.zeros(S, bool)
    skip[2::2] = lab[1:] != lab[:-1]
    edges = delim >= 0 and U >= 3
    edge_first = edges and lab[0] == delim
    edge_last = edges and lab[-1] == delim
    d = np.full(S, NEG)
    b = np.full(S, -1, np.int32)
    z = np.empty(T, np.float64)
    c = np.empty(T, np.int32)
    em = e[:, ext]                                          # (T, S)
    for t in range(T):
        best, bb = d.copy(), b.copy()                       # 1. stay
        if S >= 2:                                          # 2. from s - 1
            m = d[:-1] > best[1:]
            best[1:][m] = d[:-1][m]
            bb[1:][m] = b[:-1][m]
        if S >= 3:                                          # 3. from s - 2 (even states whose labels differ)
            m = skip[2:] & (d[:-2] > best[2:])
            best[2:][m] = d[:-2][m]
            bb[2:][m] = b[:-2][m]
        if 0.0 > best[0]:                                   # 4. the fresh start
            best[0], bb[0] = 0.0, t
        if edge_first and t == 0 and 0.0 > best[2]:         # the recording's first edge
            best[2], bb[2] = 0.0, 0
        d = best + em[t]
        b = bb
        zt, ct = d[S - 1], b[S - 1]
        if edge_last and t == T - 1:                        # the recording's last edge
            if d[S - 2] > zt:
                zt, ct = d[S - 2], b[S - 2]
            if d[S - 3] > zt:
                zt, ct = d[S - 3], b[S - 3]
        z[t], c[t] = zt, ct
    return z, c


def overlap_pass(cands):
    """the hit rule over candidates (score, begin, end) in their order: a candidate whose begin is <= the current hit's end
    overlaps it and replaces it only with a strictly higher score; one that does not flushes it"""
    out, cur = [], None
    for s, bg, en in cands:
        if cur is not None and bg <= cur[2]:
            if s > cur[0]:
                cur = (s, bg, en)
        else:
            if cur is not None:
                out.append(cur)
            cur = (s, bg, en)
    if cur is not None:
        out.append(cur)
    return out


def hit_pass(z, c, thr):
    """the hits [(score, begin, end)] of a trace, in time order"""
    idx = np.flatnonzero((z >= thr) & (z > NEG))
    return overlap_pass((float(z[t]), int(c[t]), int(t)) for t in idx)


def spot(x, labels, blank, delim=-1, thr=NEG, max_hits=64):
    """what the kernel writes for one pair: (count, score (max_hits,) f64, begin, end (max_hits,) i32, z, c); a bad pair: count -1,
    empty slots, NaN / -1 trace"""
    T = np.asarray(x).shape[0]
    score = np.full(max_hits, np.nan)
    begin = np.full(max_hits, -1, np.int32)
    end = np.full(max_hits, -1, np.int32)
    tr = trace(x, labels, blank, delim)
    if tr is None:
        return -1, score, begin, end, np.full(T, np.nan), np.full(T, -1, np.int32)
    hits = hit_pass(tr[0], tr[1], thr)
    for i, (s, bg, en) in enumerate(hits[:max_hits]):
        score[i], begin[i], end[i] = s, bg, en
    return len(hits), score, begin, end, tr[0], tr[1]


def chunk_plan(T, chunk, overlap):
    """[(start, frames)] of the pieces of a recording of T frames: piece k starts at k (chunk - overlap) and the last one is the
    first that reaches the recording's end"""
    assert 0 < overlap < chunk
    out, start = [], 0
    while True:
        out.append((start, min(chunk, T - start)))
        if start + chunk >= T:
            return out
        start += chunk - overlap


def chunked(x, labels, blank, thr, chunk, overlap, max_hits=64):
    """the hits of find_phrases(chunk_frames=chunk, overlap_frames=overlap): every piece searched alone (no edge rule), a piece
    behind the first keeping the hits whose local end is >= overlap, all kept hits sorted by (end, begin) and passed through the
    overlap rule once more; None for a bad pair"""
    x = np.asarray(x, np.float32)
    kept = []
    for k, (start, frames) in enumerate(chunk_plan(x.shape[0], chunk, overlap)):
        n, s, bg, en, _, _ = spot(x[start:start + frames], labels, blank, -1, thr, max_hits)
        if n < 0:
            return None
        for i in range(min(n, max_hits)):
            if k == 0 or en[i] >= overlap:
                kept.append((float(s[i]), int(bg[i]) + start, int(en[i]) + start))
    kept.sort(key=lambda h: (h[2], h[1]))
    return overlap_pass(kept)


def collapse(path, blank):
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def brute_force(x, labels, blank):
    """per t: (the max over all begins b <= t and all frame strings on [b, t] that start with l_0, end with l_{U-1} and collapse
    to the phrase, of the sum of e; the set of begins that attain it); (-inf, empty) where there is none"""
    e = emissions(x)
    T, V = e.shape
    lab = list(labels)
    out = []
    for t in range(T):
        best, begins = NEG, set()
        for bg in range(t + 1):
            for path in itertools.product(range(V), repeat=t - bg + 1):
                if path[0] != lab[0] or path[-1] != lab[-1] or collapse(path, blank) != lab:
                    continue
                s = 0.0
                for k, v in enumerate(path):                # in frame order, as the recursion adds
                    s = s + e[bg + k, v]
                if s > best:
                    best, begins = s, {bg}
                elif s == best and s > NEG:
                    begins.add(bg)
        out.append((best, begins))
    return out


def path_score(x, labels, blank, begin, end):
    """the best score of a path of the phrase over exactly [begin, end] that starts on l_0 and ends on l_{U-1} (a plain Viterbi
    without the free begin), for checking that the reported begin attains z_t"""
    e = emissions(x)
    lab = np.asarray(labels, np.int64)
    U = lab.size
    S = 2 * U - 1
    ext = np.full(S, blank, np.int64)
    ext[0::2] = lab
    d = np.full(S, NEG)
    d[0] = e[begin, ext[0]]
    for t in range(begin + 1, end + 1):
        n = d.copy()
        n[1:] = np.maximum(n[1:], d[:-1])
        for s in range(2, S, 2):
            if ext[s] != ext[s - 2]:
                n[s] = max(n[s], d[s - 2])
        d = n + e[t, ext]
    return d[S - 1]


def planted(rng, T, V, blank, path_at, scale=8.0):
    """N(0, 1) logits with `scale` added on the given {frame: token}"""
    x = rng.standard_normal((T, V)).astype(np.float32)
    for t, v in path_at.items():
        x[t, v] += np.float32(scale)
    return x

