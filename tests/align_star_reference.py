"""fp64 numpy reference of the CTC forced alignment with a star (wildcard) label, step for step the definition in csrc/align.hip
(test infrastructure only; the package never imports it).  The star's id is V, the vocabulary size, as if the logits had one more
column whose raw-logit value at frame t is xs_t = (double)m_t + (double)star_score, m_t the fp32 maximum of the frame's V logits
with fmax semantics (a NaN is ignored).  Everything else is tests/align_reference.py's recursion, which stays as it is: without a
star in the labels ``viterbi`` here returns its bits."""

import numpy as np

import align_reference as AR


def frame_max(logits):
    """m_t: fp32 maximum of each row, NaN ignored (-inf for a row of NaN): the value of frame_lse_max in ctc_lattice.h."""
    x = np.asarray(logits, np.float32)
    with np.errstate(invalid="ignore"):
        return np.fmax(np.float32(-np.inf), np.fmax.reduce(x, axis=1))


def star_emission(logits, star_score):
    """xs_t = (double)m_t + (double)star_score, star_score an fp32 value."""
    return frame_max(logits).astype(np.float64) + np.float64(np.float32(star_score))


def lse_lane_order(logits):
    """lse_t in the order of operations of frame_lse (ctc_lattice.h): the fp32 maximum (fmax), fp64 sums of exp(x - max) per lane
    over the columns lane, lane + 64, ..., the butterfly over the 64 lanes (xor 32, 16, ..., 1), then max + log(sum).  What is
    left to differ from the device is the last bit of exp and log themselves."""
    x32 = np.asarray(logits, np.float32)
    T, V = x32.shape
    m = frame_max(x32).astype(np.float64)
    x = x32.astype(np.float64)
    acc = np.zeros((T, 64))
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for v0 in range(0, V, 64):
            w = min(64, V - v0)
            acc[:, :w] += np.exp(x[:, v0:v0 + w] - m[:, None])
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
        return m + np.log(acc[:, 0])


def viterbi(logits, labels, blank, star_score, device_order=False, return_states=False):
    """(token, label_index, frame_logp, score) of the best path of ``labels``, in which the id V is the star; -1 rows, NaN
    frame_logp and score -inf (infeasible: T < U + R, the star counting like any label) or NaN (a label < 0, > V or equal to the
    blank) when there is none.  lse_t and its sum over t are align_reference's (numpy's own order of additions), so that without a
    star every bit equals align_reference.viterbi; ``device_order=True`` takes both in the kernels' order of operations
    (``lse_lane_order``, ``score_sum``), which is what the definition fixes."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    T, V = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    U = lab.size
    none = (np.full(T, -1, np.int32), np.full(T, -1, np.int32), np.full(T, np.nan, np.float32))
    if U and ((lab < 0) | (lab > V) | (lab == blank)).any():
        return none + (float("nan"),)
    if T < U + AR.repeats(lab):
        return none + (float("-inf"),)
    xa = np.concatenate([x, star_emission(logits, star_score)[:, None]], axis=1)       # column V: the star
    S = 2 * U + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(S, bool)
    if U > 1:
        skip[3::2] = lab[1:] != lab[:-1]
    delta = np.full(S, -np.inf)
    delta[0] = xa[0, blank]
    if U:
        delta[1] = xa[0, lab[0]]
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
            delta = m + xa[t, ext]
        s = (S - 1 if delta[S - 1] > delta[S - 2] else S - 2) if U else 0
        end = delta[s]
        states = np.empty(T, np.int64)
        for t in range(T - 1, 0, -1):
            states[t] = s
            s -= int(bp[t, s])
        states[0] = s
        token = ext[states].astype(np.int32)
        label_index = np.where(states & 1, states >> 1, -1).astype(np.int32)
        ls = lse_lane_order(logits) if device_order else AR.lse(x)
        frame_logp = (xa[np.arange(T), token] - ls).astype(np.float32)
        score = float(end - (score_sum(ls) if device_order else ls.sum()))
    if return_states:
        return token, label_index, frame_logp, score, states
    return token, label_index, frame_logp, score


def score_sum(ls):
    """sum_t lse_t in the kernels' order: lane l adds frames l, l + 64, ... in turn, then the butterfly over the 64 lanes."""
    ls = np.asarray(ls, np.float64)
    acc = np.zeros(64)
    for t0 in range(0, ls.size, 64):
        w = min(64, ls.size - t0)
        acc[:w] += ls[t0:t0 + w]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
    return acc[0]
