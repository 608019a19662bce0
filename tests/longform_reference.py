"""numpy reference of the pause cuts (w2v2_ctc_pause_cuts; the definition in include/w2v2.h, frame by frame) and the greedy CTC
collapse.  The GPU kernel must reproduce `pause_cuts` exactly; tests/test_longform_cpu.py pins the reference itself on
hand-built cases."""

import numpy as np


def frame_codes(x, blank, margin):
    """(a_t, quiet_t) per row of x (T, V) fp32.  a_t: argmax, lowest index on ties, -1 for a row that holds a NaN.
    quiet_t: a_t == blank and x_t[blank] - max_{v != blank} x_t[v] >= margin, one fp32 subtraction; V == 1: quiet."""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    a = np.full(T, -1, np.int64)
    quiet = np.zeros(T, bool)
    margin = np.float32(margin)
    for t in range(T):
        row = x[t]
        if np.isnan(row).any():
            continue
        a[t] = int(np.argmax(row))          # (numpy returns the first of equal maxima)
        if a[t] != blank:
            continue
        if V == 1:
            quiet[t] = True
            continue
        other = np.max(np.delete(row, blank))
        with np.errstate(invalid="ignore"):
            quiet[t] = bool(np.float32(row[blank]) - np.float32(other) >= margin)
    return a, quiet


def pause_cuts(x, blank, delim, margin, min_pause):
    """(cuts, pauses) of one utterance: every maximal run [a, b) of quiet frames with b - a >= min_pause, a > 0 and b < T --
    with delim >= 0 only if the last frame before a with a_t != blank exists and has a_t == delim -- gives the cut
    a + (b - a) // 2 and the pause length b - a."""
    a_t, quiet = frame_codes(x, blank, margin)
    T = len(a_t)
    cuts, pauses = [], []
    t = 0
    while t < T:
        if not quiet[t]:
            t += 1
            continue
        a = t
        while t < T and quiet[t]:
            t += 1
        b = t
        if b - a < min_pause or a == 0 or b == T:
            continue
        if delim >= 0:
            before = [u for u in range(a - 1, -1, -1) if a_t[u] != blank][:1]
            if not before or a_t[before[0]] != delim:
                continue
        cuts.append(a + (b - a) // 2)
        pauses.append(b - a)
    return np.asarray(cuts, np.int32), np.asarray(pauses, np.int32)


def greedy(x, blank):
    """Greedy CTC decode: the argmax path with runs merged and blanks dropped."""
    path = np.argmax(np.asarray(x, np.float32), axis=1)
    keep = np.flatnonzero((path != blank) & np.concatenate(([True], path[1:] != path[:-1])))
    return [int(v) for v in path[keep]]


def peaky_logits(rng, T, V, blank, delim, min_pause, n_pauses, loud=8.0, letters=None):
    """Seeded logits with one clear winner per frame: words of letters (each held 1-3 frames, repeats separated by a blank),
    a delimiter after each word, and `n_pauses` planted pauses of 2 * min_pause .. 4 * min_pause quiet frames spread over the
    sequence, none at its start or end.  Returns (x (T, V) fp32, the argmax path)."""
    letters = [v for v in range(V) if v not in (blank, delim)] if letters is None else list(letters)
    path = []
    pause_at = set(int(p) for p in np.linspace(T / (n_pauses + 1), T * n_pauses / (n_pauses + 1), n_pauses))
    while len(path) < T:
        for _ in range(int(rng.integers(2, 6))):
            c = int(rng.choice(letters))
            if path and path[-1] == c:
                path.append(blank)
            path.extend([c] * int(rng.integers(1, 4)))
            if rng.random() < 0.3:
                path.append(blank)
        path.extend([delim] * int(rng.integers(1, 3)))
        due = [p for p in pause_at if p <= len(path)]
        for p in due:
            pause_at.discard(p)
            path.extend([blank] * int(rng.integers(2 * min_pause, 4 * min_pause + 1)))
    path = np.asarray(path[:T - 2] + [letters[0], delim][:max(0, min(2, T))], np.int64)[:T]
    x = (0.25 * rng.standard_normal((T, V))).astype(np.float32)      # (|noise| << loud: every frame's winner leads by > loud / 2)
    x[np.arange(T), path] += np.float32(loud)
    return x, path
