"""fp64 numpy reference of the exact CTC score, step for step the definition in csrc/score.hip (w2v2_ctc_score; test
infrastructure only; the package never imports it).

lp_t(v) = x_t(v) - lse_t on the fp32 logits widened to fp64; ext the labels with blanks interleaved, S = 2U + 1:
  alpha_0(0) = lp_0(blank), alpha_0(1) = lp_0(l_0);
  alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [ext[s] != blank and ext[s] != ext[s-2]] alpha_{t-1}(s-2)) + lp_t(ext[s]);
  logp = lse(alpha_{T-1}(S-1), alpha_{T-1}(S-2)), U = 0: alpha_{T-1}(0).
T < U + repeats: -inf.  A label outside [0, V) or the blank: NaN.  A frame whose lse is not finite (a NaN or +inf logit, or a frame
of -inf only): NaN.  -inf logits are legal."""

import itertools
import math

import numpy as np


def lse_rows(logits):
    """fp64 log-sum-exp of each row of fp32 logits (max-subtracted)."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=1, keepdims=True)
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def repeats(labels):
    a = np.asarray(labels, np.int64).reshape(-1)
    return int((a[1:] == a[:-1]).sum()) if a.size > 1 else 0


def tau(T, reference):
    """bound on the accumulated fp64 rounding of T steps, with a factor 16 for the library functions (tests/beam_reference.py::tau)"""
    return 16.0 * T * 2.0 ** -52 * max(1.0, abs(reference))


def _lse_stack(rows):
    """element-wise log-sum-exp of a list of equal-length fp64 arrays; -inf where all are -inf"""
    a = np.stack(rows)
    m = a.max(axis=0)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.exp(a - safe).sum(axis=0)), -np.inf)


def ctc_logp(logits, labels, blank=0):
    """the exact CTC log-probability of ``labels`` given (T, V) ``logits``"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    U = lab.size
    if U and ((lab < 0) | (lab >= V) | (lab == blank)).any():
        return float("nan")
    ls = lse_rows(x)
    if not np.isfinite(ls).all():
        return float("nan")
    if T < U + repeats(lab):
        return float("-inf")
    lp = x - ls[:, None]
    S = 2 * U + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(S, bool)
    if U > 1:
        skip[3::2] = lab[1:] != lab[:-1]
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, blank]
    if U:
        alpha[1] = lp[0, lab[0]]
    neg1 = np.array([-np.inf])
    neg2 = np.array([-np.inf, -np.inf])
    for t in range(1, T):
        one = np.concatenate((neg1, alpha[:-1]))
        two = np.where(skip, np.concatenate((neg2, alpha[:-2]))[:S], -np.inf)
        alpha = _lse_stack([alpha, one, two]) + lp[t, ext]
    if U == 0:
        return float(alpha[0])
    return float(_lse_stack([alpha[S - 1:S], alpha[S - 2:S - 1]])[0])


def brute_force(logits, labels, blank=0):
    """log of the summed probability of every one of the V^T frame paths that collapses to ``labels`` (tiny T and V only)"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    lp = x - lse_rows(x)[:, None]
    want = tuple(int(v) for v in labels)
    total = 0.0
    for path in itertools.product(range(V), repeat=T):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if tuple(out) == want:
            total += math.exp(sum(lp[t, c] for t, c in enumerate(path)))
    return math.log(total) if total > 0 else -math.inf
