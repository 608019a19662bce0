"""The resampler's definition in fp64 numpy (include/w2v2.h, w2v2_resample_design / w2v2_resample).

design(rate_in, rate_out, zeros, rolloff, beta) -> (L, M, K, lead, table64): the polyphase Kaiser-windowed-sinc table.
apply(x, L, M, K, lead, table) -> (out64, mag64): every output as its sum over the K taps, and the sum of the taps' magnitudes,
which scales the rounding bound of an fp32 evaluation.  tests/test_resample_cpu.py pins both against scipy's resample_poly."""

from math import ceil, gcd

import numpy as np


def ratio(rate_in, rate_out):
    g = gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g          # L, M


def out_length(n, L, M):
    return -(-int(n) * L // M)


def design(rate_in, rate_out=16000, zeros=32, rolloff=0.95, beta=12.0):
    L, M = ratio(rate_in, rate_out)
    if L == M:
        return L, M, 1, 0, np.ones((1, 1), np.float64)
    fc = min(L, M) * rolloff / M
    width = int(ceil(zeros / fc))
    K, lead = 2 * width, width - 1
    t = np.arange(K, dtype=np.float64)[None, :]
    r = np.arange(L, dtype=np.float64)[:, None]
    u = (t - lead) - r / L
    s = u * fc
    inside = np.abs(s) < zeros
    a = np.pi * s
    sinc = np.where(s == 0.0, 1.0, np.sin(a) / np.where(s == 0.0, 1.0, a))
    sw = np.where(inside, s / zeros, 0.0)
    table = fc * sinc * np.i0(beta * np.sqrt(1.0 - sw * sw)) / np.i0(beta)
    return L, M, K, lead, np.where(inside, table, 0.0)


def apply(x, L, M, K, lead, table):
    """out[n] = sum_t table[r][t] x[q - lead + t] with q = n M // L, r = n M % L and x zero outside; mag[n] the same sum of
    |table| |x|.  `table` may hold integers (the index tests)."""
    x = np.asarray(x, np.float64)
    table = np.asarray(table, np.float64).reshape(L, K)
    n = np.arange(out_length(len(x), L, M), dtype=np.int64)
    q, r = n * M // L, n * M % L
    lo = int(min(0, (q - lead).min()))
    hi = int(max(len(x), (q - lead).max() + K))
    xp = np.zeros(hi - lo, np.float64)
    xp[-lo:-lo + len(x)] = x
    out, mag = np.zeros(len(n), np.float64), np.zeros(len(n), np.float64)
    for t in range(K):
        c, v = table[r, t], xp[q - lead + t - lo]
        out += c * v
        mag += np.abs(c) * np.abs(v)
    return out, mag
