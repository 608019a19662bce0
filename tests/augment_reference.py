"""The definitions of w2v2_fir and w2v2_mix in numpy (include/w2v2.h).

fir(x, h, d) -> (y64, mag64): y[n] = sum_k h[k] x[n + d - k] for n in [0, len(x)) with x zero outside, in fp64 (integer inputs stay
exact), and the same sum of |h| |x|, which scales the rounding bound of an fp32 evaluation.
fir_chain32(x, h, d): the same outputs as ONE fp32 chain in ascending k from +0, the order the kernel is held to.  Each step is
float32(acc + float32(h[k] * x[.])): where every product is exact in fp32 (the bit tests choose such data) that IS fmaf.
sumsq, fir_gain, noise_window, mix_gain, mix: the powers in fp64 and what follows from them.
tests/test_augment_cpu.py pins fir against numpy.convolve."""

import numpy as np


def _padded(x, K, d, dtype):
    """x behind K - 1 - d zeros and in front of d zeros, so that x[n + d - k] = xp[n + K - 1 - k]."""
    xp = np.zeros(len(x) + K - 1, dtype)
    xp[K - 1 - d:K - 1 - d + len(x)] = x
    return xp


def fir(x, h, d):
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    K = len(h)
    assert x.ndim == 1 and h.ndim == 1 and 0 <= d < K
    xp = _padded(x, K, d, np.float64)
    out, mag = np.zeros(len(x), np.float64), np.zeros(len(x), np.float64)
    for k in range(K):
        v = xp[K - 1 - k:K - 1 - k + len(x)]
        out += h[k] * v
        mag += abs(h[k]) * np.abs(v)
    return out, mag


def fir_chain32(x, h, d, descending=False):
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    K = len(h)
    xp = _padded(x, K, d, np.float32)
    acc = np.zeros(len(x), np.float32)
    for k in (range(K - 1, -1, -1) if descending else range(K)):
        acc = acc + h[k] * xp[K - 1 - k:K - 1 - k + len(x)]
        assert acc.dtype == np.float32
    return acc


def sumsq(x):
    return float(np.sum(np.asarray(x, np.float64) ** 2))


def fir_gain(x, y):
    """g of match_power: sqrt(Px / Py), 1 when either power is 0 (y: the unscaled output)."""
    px, py = sumsq(x), sumsq(y)
    return 1.0 if px == 0.0 or py == 0.0 else float(np.sqrt(px / py))


def noise_window(noise, offset, n):
    noise = np.asarray(noise)
    return noise[(offset + np.arange(n, dtype=np.int64)) % len(noise)]


def mix_gain(x, v, scale):
    px, pv = sumsq(x), sumsq(v)
    return 0.0 if px == 0.0 or pv == 0.0 else float(np.sqrt(px / pv) * scale)


def mix(x, v, g):
    """x + g v in fp64"""
    return np.asarray(x, np.float64) + float(g) * np.asarray(v, np.float64)
