"""fp64 numpy reference of the gradient of a weighted sum of exact CTC log-probabilities, step for step the definition in
csrc/score.hip (w2v2_ctc_score_grad; test infrastructure only; the package never imports it).

lp, ext, S = 2U + 1, the skip rule, alpha and logp are those of tests/score_reference.py.  The backward variable excludes the
frame's own emission, so no lp is ever subtracted:
  beta_{T-1}(S-1) = 0; beta_{T-1}(S-2) = 0 if U >= 1; every other state -inf;
  beta_t(s) = lse(beta_{t+1}(s) + lp_{t+1}(ext[s]), beta_{t+1}(s+1) + lp_{t+1}(ext[s+1]),
                  [s+2 < S and ext[s+2] != blank and ext[s+2] != ext[s]] (beta_{t+1}(s+2) + lp_{t+1}(ext[s+2])));
  gamma_t(s) = exp(alpha_t(s) + beta_t(s) - logp), 0 where alpha_t(s) or beta_t(s) is -inf;
  Gamma(t, v) = sum over s with ext[s] = v of gamma_t(s); y_t(v) = exp(lp_t(v)); d logp / d x_t(v) = Gamma(t, v) - y_t(v).
Per utterance over its pairs: G(t, v) = sum_j c_j Gamma_j(t, v) - (sum_j c_j) y_t(v); a pair whose logp is -inf or NaN contributes
nothing to either sum."""

import numpy as np

from score_reference import _lse_stack, lse_rows, repeats, tau


def occupancy(logits, labels, blank=0):
    """(logp, Gamma) of one pair: Gamma is (T, V) fp64, None when logp is -inf or NaN"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    U = lab.size
    if U and ((lab < 0) | (lab >= V) | (lab == blank)).any():
        return float("nan"), None
    ls = lse_rows(x)
    if not np.isfinite(ls).all():
        return float("nan"), None
    if T < U + repeats(lab):
        return float("-inf"), None
    lp = x - ls[:, None]
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
    Gamma = np.zeros((T, V))
    for s in range(S):
        Gamma[:, ext[s]] += gamma[:, s]
    return logp, Gamma


def score_grad(logits, pairs, coef, blank=0):
    """One utterance: ``logits`` (T, V), ``pairs`` a list of label sequences, ``coef`` their coefficients.
    Returns (logp (m) fp64, G (T, V) fp64, bar (T, V): the tests' tolerance without its fp32 term)."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    logp = np.empty(len(pairs))
    G = np.zeros((T, V))
    csum, slack = 0.0, 0.0
    for j, lab in enumerate(pairs):
        logp[j], Gam = occupancy(x, lab, blank)
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


def bar(ref, slack):
    """|got - ref| <= 2^-23 |ref| + sum_j |c_j| 4 * 16 T 2^-52 max(1, |logp_j| + 40): fp32 rounding of the result, plus alpha, beta,
    logp and the frame lse each within score_reference.tau, passed one for one through an exponent whose result is at most 1 (a
    state with gamma < e^-40 contributes less than the bound whatever its error)"""
    return 2.0 ** -23 * np.abs(ref) + slack


__all__ = ["occupancy", "score_grad", "bar", "tau"]
