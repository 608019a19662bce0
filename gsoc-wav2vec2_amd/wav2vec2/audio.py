"""Sampling rates: a polyphase Kaiser-windowed-sinc resampler with a rational ratio on the device.

The model, the window plan and every timestamp assume 16 000 samples per second.  This module brings audio of any rate there:

``resampled_length``  samples that ``n`` samples become;
``Resampler``         one designed filter (``w2v2_resample_design``), applied to one waveform or a list in ONE
                      ``w2v2_resample`` call (csrc/resample.hip);
``resample``          the one-shot form over a small cache of ``Resampler``s;
``speed_perturb``     utterances played 0.9x / 1.1x for CTC fine-tuning: the same kernel, one filter per distinct factor, one call.

The exact definition (the filter, the output length, the order of the fp32 sum) is in include/w2v2.h and, in fp64 numpy, in
tests/resample_reference.py.  Every waveform is computed as if it were alone, and a ratio of one returns the input's bits.
"""

import ctypes as C
import functools
from fractions import Fraction
from math import gcd

import numpy as np

from . import _native as N


def _rate(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
        raise ValueError(f"{what} must be a positive integer, got {value!r}")
    return int(value)


def resampled_length(n, rate_in, rate_out=16000):
    """ceil(n * rate_out / rate_in): the samples that ``n`` samples at ``rate_in`` become at ``rate_out``."""
    rate_in, rate_out = _rate(rate_in, "rate_in"), _rate(rate_out, "rate_out")
    n = int(n)
    if n < 0:
        raise ValueError(f"a length of {n} samples")
    g = gcd(rate_in, rate_out)
    return -(-n * (rate_out // g) // (rate_in // g))


def _as_parts(waves, what="waves"):
    """(single, list of 1-D torch tensors) of one waveform or a non-empty list of them (numpy, torch on any device)."""
    import torch
    single = isinstance(waves, (np.ndarray, torch.Tensor))
    if single:
        waves = [waves]
    elif not isinstance(waves, (list, tuple)) or not len(waves):
        raise ValueError(f"`{what}` must be a 1-D waveform or a non-empty list of them")
    parts = []
    for i, w in enumerate(waves):
        if not isinstance(w, torch.Tensor):
            w = torch.as_tensor(np.asarray(w, dtype=np.float32))
        if w.dim() != 1:
            raise ValueError(f"waveform {i} must be 1-D, got shape {tuple(w.shape)}")
        if w.shape[0] < 1:
            raise ValueError(f"waveform {i} is empty")
        parts.append(w)
    return single, parts


def _apply(parts, resamplers, filter_of):
    """ONE w2v2_resample call: parts[i] through resamplers[filter_of[i]].  Returns views of one device buffer."""
    import torch
    from .modeling import DeviceTensor, _require_gpu
    _require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    parts = [p.to(device=dev, dtype=torch.float32) for p in parts]
    wave = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
    in_len = np.asarray([p.shape[0] for p in parts], np.int64)
    in0 = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.int64)
    out_len = [-(-int(n) * resamplers[k].L // resamplers[k].M) for n, k in zip(in_len, filter_of)]
    out0 = np.concatenate(([0], np.cumsum(out_len)[:-1])).astype(np.int64)
    out = torch.empty(int(sum(out_len)), dtype=torch.float32, device=dev)
    filters = (N.W2V2ResampleFilter * len(resamplers))()
    tables = [r._table(dev) for r in resamplers]          # (kept alive until the call is enqueued)
    for f, r, t in zip(filters, resamplers, tables):
        f.table, f.L, f.M, f.K, f.lead = t.data_ptr(), r.L, r.M, r.taps, r.lead
    which = np.asarray(filter_of, np.int32)
    N.check(N.load().w2v2_resample(N.ptr(wave), len(parts), N.ptr(in0), N.ptr(in_len), N.ptr(which), filters, len(resamplers),
                                   N.ptr(out), N.ptr(out0), N.current_stream()), "w2v2_resample")
    return list(torch.split(DeviceTensor.wrap(out), out_len))


class Resampler:
    """The filter from ``rate_in`` to ``rate_out`` samples per second: ``zeros`` zero crossings of the sinc on each side of
    its centre at the lower of the two rates, cut off at ``rolloff`` of the lower Nyquist frequency, under a Kaiser window of
    shape ``beta``.  ``r(waves)``: one 1-D waveform or a list (numpy, torch on the CPU or the GPU) -> a tensor or a list of
    tensors on the device, views of one buffer as ``predict_packed`` returns them; waveform i has
    ``resampled_length(len_i, rate_in, rate_out)`` samples.  ``r.L`` / ``r.M``: the reduced ratio ``rate_out / rate_in``;
    ``r.taps``: taps per output; ``r.lead``: taps before the output's own position; ``r.table``: the (L, taps) fp32 table."""

    def __init__(self, rate_in, rate_out=16000, zeros=32, rolloff=0.95, beta=12.0):
        self.rate_in, self.rate_out = _rate(rate_in, "rate_in"), _rate(rate_out, "rate_out")
        self.zeros, self.rolloff, self.beta = _rate(zeros, "zeros"), float(rolloff), float(beta)
        if not 0.0 < self.rolloff <= 1.0:
            raise ValueError(f"rolloff {rolloff} outside (0, 1]")
        if not (np.isfinite(self.beta) and self.beta >= 0.0):
            raise ValueError(f"beta {beta}: a finite value >= 0")
        lib = N.load()
        size = [C.c_int32() for _ in range(4)]
        args = (self.rate_in, self.rate_out, self.zeros, self.rolloff, self.beta, *(C.byref(v) for v in size))
        N.check(lib.w2v2_resample_design(*args, None, 0), "w2v2_resample_design")
        self.L, self.M, self.taps, self.lead = (int(v.value) for v in size)
        if self.L > N.RESAMPLE_MAX_L or self.L * self.taps > N.RESAMPLE_MAX_TABLE:
            raise ValueError(f"{self.rate_in} -> {self.rate_out} Hz reduces to {self.L} / {self.M} with {self.taps} taps: at most "
                             f"{N.RESAMPLE_MAX_L} phases and {N.RESAMPLE_MAX_TABLE} table entries")
        self.table = np.empty((self.L, self.taps), np.float32)
        N.check(lib.w2v2_resample_design(*args, N.ptr(self.table), self.table.size), "w2v2_resample_design")
        self._device_tables = {}

    def _table(self, dev):
        import torch
        t = self._device_tables.get(dev.index)
        if t is None:
            t = self._device_tables[dev.index] = torch.from_numpy(self.table).to(dev)
        return t

    def __call__(self, waves):
        single, parts = _as_parts(waves)
        out = _apply(parts, [self], [0] * len(parts))
        return out[0] if single else out


@functools.lru_cache(maxsize=16)
def _cached(rate_in, rate_out, zeros, rolloff, beta):
    return Resampler(rate_in, rate_out, zeros, rolloff, beta)


def resample(waves, rate_in, rate_out=16000, zeros=32, rolloff=0.95, beta=12.0):
    """``Resampler(rate_in, rate_out, zeros, rolloff, beta)(waves)``; the sixteen filters used last are kept."""
    return _cached(_rate(rate_in, "rate_in"), _rate(rate_out, "rate_out"), _rate(zeros, "zeros"), float(rolloff), float(beta))(waves)


def speed_ratio(factor):
    """(L, M) of a speed factor: ``L / M = 1 / Fraction(factor).limit_denominator(100)``, so 0.9 -> (10, 9), 1.1 -> (10, 11)."""
    factor = float(factor)
    if not (np.isfinite(factor) and factor > 0.0):
        raise ValueError(f"a speed factor must be positive, got {factor}")
    f = Fraction(factor).limit_denominator(100)
    if f.numerator < 1:
        raise ValueError(f"the speed factor {factor} is below 1 / 100")
    return f.denominator, f.numerator


def speed_perturb(waves, factors=(0.9, 1.0, 1.1), seed=None, choices=None):
    """Speed perturbation, the standard augmentation of CTC fine-tuning: utterance i is played ``f_i`` times faster, pitch
    included, and has ``ceil(len_i L / M)`` samples, ``L / M = speed_ratio(f_i)`` (``ceil(len_i / f_i)`` for a factor that is
    such a fraction).  ``f_i`` is ``factors[choices[i]]`` when ``choices`` is given, else drawn per utterance from ``factors``
    with ``numpy.random.default_rng(seed)``.  A factor of one takes the copy filter and returns the input's bits.  All
    utterances go through ONE ``w2v2_resample`` call, one filter per distinct factor.  ``waves``: a list of 1-D waveforms.
    Returns ``(list of device tensors, list of the factors chosen)``; normalise and pad with ``batchify`` afterwards."""
    if isinstance(waves, np.ndarray) or not isinstance(waves, (list, tuple)) or not len(waves):
        raise ValueError("`waves` must be a non-empty list of 1-D waveforms")
    factors = [float(f) for f in factors]
    if not factors:
        raise ValueError("`factors` is empty")
    ratios = [speed_ratio(f) for f in factors]
    if choices is None:
        choices = np.random.default_rng(seed).integers(0, len(factors), size=len(waves))
    choices = [int(c) for c in choices]
    if len(choices) != len(waves) or any(not 0 <= c < len(factors) for c in choices):
        raise ValueError(f"`choices`: one index into the {len(factors)} factors per utterance")
    _, parts = _as_parts(list(waves))
    distinct = sorted({ratios[c] for c in choices})
    # (playing M / L times faster is resampling from M to L samples per second and reading the result at the old rate)
    resamplers = [_cached(M, L, 32, 0.95, 12.0) for L, M in distinct]
    out = _apply(parts, resamplers, [distinct.index(ratios[c]) for c in choices])
    return out, [factors[c] for c in choices]
