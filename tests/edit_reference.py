"""The edit distance's definition in plain Python (include/w2v2.h, w2v2_edit_distance): the DP over the
lexicographic cost (errors, substitutions), one row at a time, a brute-force enumeration of all alignments for tiny pairs, and the minimum-Bayes-risk formula written out."""

import math


def edit_counts(a, b):
    """(distance, substitutions, deletions, insertions) of the hypothesis a against the reference b.  A cell (errors,
    substitutions) is held as the integer errors * K + substitutions, whose order is the lexicographic one (Python integers do
    not overflow)."""
    a, b = list(a), list(b)
    m, n = len(a), len(b)
    K = 1 << 20
    row = [j * K for j in range(n + 1)]
    for i in range(1, m + 1):
        ai, left = a[i - 1], i * K
        new = [left]
        for j in range(1, n + 1):
            d = row[j - 1] if ai == b[j - 1] else row[j - 1] + K + 1
            left = min(d, row[j] + K, left + K)
            new.append(left)
        row = new
    C, S = divmod(row[n], K)
    D = (C - S - (m - n)) // 2
    return C, S, D, D + m - n


def all_alignments(a, b):
    """(hits, substitutions, deletions, insertions) of EVERY alignment of a against b (a monotone path of diagonal, down and
    right moves; a diagonal move is a hit or a substitution by the tokens): exponential, for lengths up to 6 or so."""
    a, b = list(a), list(b)
    out = []

    def walk(i, j, h, s, d, ins):
        if i == len(a) and j == len(b):
            out.append((h, s, d, ins))
            return
        if i < len(a) and j < len(b):
            eq = a[i] == b[j]
            walk(i + 1, j + 1, h + eq, s + (not eq), d, ins)
        if j < len(b):
            walk(i, j + 1, h, s, d + 1, ins)
        if i < len(a):
            walk(i + 1, j, h, s, d, ins + 1)

    walk(0, 0, 0, 0, 0, 0)
    return out


def mbr_reference(lists, tokens, scale):
    """(indices, risks) of wav2vec2.metrics.mbr_select: per utterance a list of (ids, total); p = softmax(scale * total),
    R_k = sum_j p_j distance(tokens(h_k), tokens(h_j)), the index of the smallest R (the first on ties)."""
    indices, risks = [], []
    for hyps in lists:
        z = [scale * t for _, t in hyps]
        e = [math.exp(x - max(z)) for x in z]
        p = [x / sum(e) for x in e]
        R = [sum(p[j] * edit_counts(tokens(hk), tokens(hj))[0] for j, (hj, _) in enumerate(hyps)) for hk, _ in hyps]
        indices.append(R.index(min(R)) if R else -1)
        risks.append(R)
    return indices, risks
