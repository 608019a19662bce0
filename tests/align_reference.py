"""fp64 numpy reference of the CTC forced alignment, step for step the definition in csrc/align.hip (test infrastructure only;
the package never imports it)."""

import numpy as np


def lse(logits):
    """fp64 log-sum-exp of each row of fp32 logits."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True)
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def repeats(labels):
    a = np.asarray(labels, np.int64).reshape(-1)
    return int((a[1:] == a[:-1]).sum()) if a.size > 1 else 0


def viterbi(logits, labels, blank, return_states=False):
    """(token, label_index, frame_logp, score) of the best path; -1 rows, NaN frame_logp and score -inf (infeasible) or NaN
    (a label outside the vocabulary or equal to the blank) when there is none."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    U = lab.size
    none = (np.full(T, -1, np.int32), np.full(T, -1, np.int32), np.full(T, np.nan, np.float32))
    if U and ((lab < 0) | (lab >= V) | (lab == blank)).any():
        return none + (float("nan"),)
    if T < U + repeats(lab):
        return none + (float("-inf"),)
    S = 2 * U + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(S, bool)
    if U > 1:
        skip[3::2] = lab[1:] != lab[:-1]
    delta = np.full(S, -np.inf)
    delta[0] = x[0, blank]
    if U:
        delta[1] = x[0, lab[0]]
    bp = np.zeros((T, S), np.uint8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            m = delta.copy()
            b = bp[t]
            take = delta[:-1] > m[1:]
            m[1:][take] = delta[:-1][take]
            b[1:][take] = 1
            take2 = skip[2:] & (delta[:-2] > m[2:])
            m[2:][take2] = delta[:-2][take2]
            b[2:][take2] = 2
            delta = m + x[t, ext]
        s = (S - 1 if delta[S - 1] > delta[S - 2] else S - 2) if U else 0
        end = delta[s]
        states = np.empty(T, np.int64)
        for t in range(T - 1, 0, -1):
            states[t] = s
            s -= int(bp[t, s])
        states[0] = s
        token = ext[states].astype(np.int32)
        label_index = np.where(states & 1, states >> 1, -1).astype(np.int32)
        ls = lse(x)
        frame_logp = (x[np.arange(T), token] - ls).astype(np.float32)
        score = float(end - ls.sum())
    if return_states:
        return token, label_index, frame_logp, score, states
    return token, label_index, frame_logp, score
