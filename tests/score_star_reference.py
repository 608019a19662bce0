"""fp64 numpy reference of the exact CTC score with a star and of its gradient, step for step the definition in
csrc/score.hip (w2v2_ctc_score_star, w2v2_ctc_score_grad_star; test infrastructure only; the package never
imports it).

Everything is tests/score_reference.py (alpha, logp) and tests/score_grad_reference.py (beta, gamma, Gamma, G) except:
  the star label: id V is the star, "as if the logits had one more column" (tests/align_star_reference.py);
  its emission: lp_t(V) = ((double)m_t + (double)star_score) - lse_t, m_t the fp32 frame maximum (blank included, NaN ignored),
  star_score <= 0 an fp32 value, lse_t over the V real columns only;
  the recursion: ext[2k + 1] = V is a state like any other; the skip rule and R treat V like any id, so a star takes at least one
  frame and T < U + R gives -inf; a label < 0, > V or equal to the blank gives NaN; a non-finite lse_t gives NaN;
  the gradient: a_t the lowest column index with x_t(a_t) == m_t; d lp_t(V) / d x_t(v) = [v = a_t] - y_t(v), so Gamma(t, a_t) also
  sums the star states' gamma; G = sum_j c_j Gamma_j - (sum_j c_j) y is unchanged.
With a star logp is the score of a set of paths, not a log-probability: it may exceed 0."""

import itertools
import math

import numpy as np

from align_star_reference import frame_max, star_emission
from score_reference import _lse_stack, lse_rows, repeats, tau
from score_grad_reference import bar


def top_token(logits):
    """a_t: the lowest column index whose logit equals the frame's fp32 maximum m_t (0 for a frame of NaN only)"""
    x = np.asarray(logits, np.float32)
    m = frame_max(x)
    return np.argmax(x == m[:, None], axis=1)


def log_emissions(logits, star_score):
    """(T, V + 1) fp64: lp_t(v) = x_t(v) - lse_t for the V real columns, lp_t(V) = (m_t + star_score) - lse_t; and lse_t"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    ls = lse_rows(x)
    xs = star_emission(logits, star_score)
    with np.errstate(invalid="ignore"):
        return np.concatenate([x, xs[:, None]], axis=1) - ls[:, None], ls


def occupancy(logits, labels, blank=0, star_score=-0.5):
    """(logp, Gamma) of one pair: Gamma is (T, V) fp64 with the star states' gamma on column a_t; None when logp is -inf or NaN"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    U = lab.size
    if U and ((lab < 0) | (lab > V) | (lab == blank)).any():
        return float("nan"), None
    lp, ls = log_emissions(logits, star_score)
    if not np.isfinite(ls).all():
        return float("nan"), None
    if T < U + repeats(lab):
        return float("-inf"), None
    S = 2 * U + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(S, bool)                    # state s may be entered from s - 2
    if U > 1:
        skip[3::2] = lab[1:] != lab[:-1]
    neg1, neg2 = np.array([-np.inf]), np.array([-np.inf, -np.inf])
    alpha = np.full((T, S), -np.inf)
    alpha[0, 0] = lp[0, blank]
    if U:
        alpha[0, 1] = lp[0, lab[0]]
    for t in range(1, T):
        a = alpha[t - 1]
        one = np.concatenate((neg1, a[:-1]))
        two = np.where(skip, np.concatenate((neg2, a[:-2]))[:S], -np.inf)
        alpha[t] = _lse_stack([a, one, two]) + lp[t, ext]
    logp = float(alpha[T - 1, 0]) if U == 0 else float(_lse_stack([alpha[T - 1, S - 1:S], alpha[T - 1, S - 2:S - 1]])[0])
    if not np.isfinite(logp):
        return logp, None                       # (every path runs through a -inf logit)
    beta = np.full((T, S), -np.inf)
    beta[T - 1, S - 1] = 0.0
    if U:
        beta[T - 1, S - 2] = 0.0
    skip_from = np.concatenate((skip[2:], [False, False]))[:S]      # state s may leave to s + 2
    for t in range(T - 2, -1, -1):
        b = beta[t + 1] + lp[t + 1, ext]
        one = np.concatenate((b[1:], neg1))
        two = np.where(skip_from, np.concatenate((b[2:], neg2))[:S], -np.inf)
        beta[t] = _lse_stack([b, one, two])
    with np.errstate(invalid="ignore"):
        e = alpha + beta - logp
    gamma = np.where(np.isfinite(alpha) & np.isfinite(beta), np.exp(np.where(np.isfinite(e), e, -np.inf)), 0.0)
    at = top_token(logits)
    rows = np.arange(T)
    Gamma = np.zeros((T, V))
    for s in range(S):
        if ext[s] == V:
            Gamma[rows, at] += gamma[:, s]      # the star state emits the frame's top token
        else:
            Gamma[:, ext[s]] += gamma[:, s]
    return logp, Gamma


def ctc_logp(logits, labels, blank=0, star_score=-0.5):
    """the exact star score of ``labels`` given (T, V) ``logits``"""
    return occupancy(logits, labels, blank, star_score)[0]


def score_grad(logits, pairs, coef, blank=0, star_score=-0.5):
    """One utterance: ``logits`` (T, V), ``pairs`` a list of label sequences (V is the star), ``coef`` their coefficients.
    Returns (logp (m) fp64, G (T, V) fp64, slack: score_grad_reference.bar's second argument)."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    logp = np.empty(len(pairs))
    G = np.zeros((T, V))
    csum, slack = 0.0, 0.0
    for j, lab in enumerate(pairs):
        logp[j], Gam = occupancy(logits, lab, blank, star_score)
        if Gam is None:
            continue
        G += float(coef[j]) * Gam
        csum += float(coef[j])
        slack += abs(float(coef[j])) * 4.0 * 16.0 * T * 2.0 ** -52 * max(1.0, abs(logp[j]) + 40.0)
    if csum != 0.0 or slack != 0.0:
        ls = lse_rows(x)
        with np.errstate(over="ignore", invalid="ignore"):
            y = np.exp(x - ls[:, None])
        G = G - csum * np.where(np.isfinite(y), y, 0.0)
    return logp, G, slack


def brute_force(logits, labels, blank=0, star_score=-0.5):
    """log of the summed score of every one of the (V + 1)^T frame paths over the (V + 1)-column matrix of ``log_emissions`` that
    collapses to ``labels`` (tiny T and V only)"""
    lp, _ = log_emissions(logits, star_score)
    T, W = lp.shape
    want = tuple(int(v) for v in labels)
    total = 0.0
    for path in itertools.product(range(W), repeat=T):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if tuple(out) == want:
            total += math.exp(sum(lp[t, c] for t, c in enumerate(path)))
    return math.log(total) if total > 0 else -math.inf


__all__ = ["top_token", "log_emissions", "occupancy", "ctc_logp", "score_grad", "brute_force", "bar", "tau"]
