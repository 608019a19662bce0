"""Sampling rates and waveform augmentation on the device.

A polyphase Kaiser-windowed-sinc resampler with a rational ratio:

The model, the window plan and every timestamp assume 16 000 samples per second.  This module brings audio of any rate there:

``resampled_length``  samples that ``n`` samples become;
``Resampler``         one designed filter (``w2v2_resample_design``), applied to one waveform or a list in ONE
                      ``w2v2_resample`` call (csrc/resample.hip);
``resample``          the one-shot form over a small cache of ``Resampler``s;
``speed_perturb``     utterances played 0.9x / 1.1x for CTC fine-tuning: the same kernel, one filter per distinct factor, one call.

The exact definition (the filter, the output length, the order of the fp32 sum) is in include/w2v2.h and, in fp64 numpy, in
tests/resample_reference.py.  Every waveform is computed as if it were alone, and a ratio of one returns the input's bits.

Augmentation for fine-tuning, in the order of the Kaldi recipes (speed, then reverberation, then noise):

``rir_delay``, ``trim_rir``  host helpers: the direct path of a room impulse response, and its cut at the -60 dB point;
``reverberate``       every utterance convolved with its own impulse response in ONE ``w2v2_fir`` call (csrc/augment.hip);
``add_noise``         a stretch of a noise recording added at a drawn signal-to-noise ratio in ONE ``w2v2_mix`` call;
``Augment``           the three stages with all draws from one generator, reproducible from the ``info`` it returns.

Their definitions are in include/w2v2.h and, in numpy, in tests/augment_reference.py.
"""

import copy
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


# ---- augmentation: reverberation and additive noise ----

def _as_filter(h, what):
    h = np.asarray(h)
    if h.ndim != 1:
        raise ValueError(f"{what} must be 1-D, got shape {tuple(h.shape)}")
    if h.shape[0] < 1:
        raise ValueError(f"{what} is empty")
    if not np.isfinite(h).all():
        raise ValueError(f"{what} holds a value that is not finite")
    return h


def rir_delay(h):
    """The index of the largest ``|h|`` (the first, if several are equal): the direct path of a room impulse response."""
    return int(np.argmax(np.abs(_as_filter(h, "the impulse response"))))


def trim_rir(h, tail_db=-60.0, max_taps=8000):
    """``h`` cut where its backward-integrated energy (Schroeder's curve, ``E[n] = sum_{k >= n} h[k]^2``) has fallen ``tail_db``
    below the total: the first ``n`` with ``E[n] < 10^(tail_db / 10) E[0]`` samples are kept.  It is cut at ``max_taps`` at the
    latest and never before the direct path (``rir_delay(h) + 1`` samples are always kept, even beyond ``max_taps``).
    ``max_taps = 8000`` is a convention -- half a second at 16 kHz, beyond which a room's tail is below the noise of most
    recordings -- not a limit of the kernel, which takes 65 536 taps.  Returns a float32 copy."""
    h = _as_filter(h, "the impulse response")
    max_taps = int(max_taps)
    if max_taps < 1:
        raise ValueError(f"max_taps = {max_taps} (need at least 1)")
    if not float(tail_db) < 0.0:
        raise ValueError(f"tail_db = {tail_db} (need a negative number of decibels)")
    e = np.cumsum((h.astype(np.float64) ** 2)[::-1])[::-1]
    if e[0] <= 0.0:
        raise ValueError("the impulse response is all zero")
    below = np.flatnonzero(e < 10.0 ** (float(tail_db) / 10.0) * e[0])
    cut = int(below[0]) if below.size else len(h)
    cut = max(min(cut, max_taps), rir_delay(h) + 1)
    return np.ascontiguousarray(h[:cut], np.float32)


class _Bank:
    """A list of 1-D fp32 arrays back to back in one buffer, uploaded once per device and kept."""

    def __init__(self, items, what):
        if isinstance(items, np.ndarray) or not isinstance(items, (list, tuple)) or not len(items):
            raise ValueError(f"`{what}` must be a non-empty list of 1-D arrays")
        self.items = [np.ascontiguousarray(_as_filter(a, f"{what}[{i}]"), np.float32) for i, a in enumerate(items)]
        self.lengths = np.asarray([len(a) for a in self.items], np.int64)
        self.starts = np.concatenate(([0], np.cumsum(self.lengths)[:-1])).astype(np.int64)
        self.flat = np.concatenate(self.items)
        self._device = {}

    def __len__(self):
        return len(self.items)

    def on(self, dev):
        import torch
        t = self._device.get(dev.index)
        if t is None:
            t = self._device[dev.index] = torch.from_numpy(self.flat).to(dev)
        return t


class _RirBank(_Bank):
    """Impulse responses after ``trim_rir``, with their direct paths."""

    def __init__(self, rirs, tail_db=-60.0, max_taps=8000):
        if isinstance(rirs, np.ndarray) or not isinstance(rirs, (list, tuple)) or not len(rirs):
            raise ValueError("`rirs` must be a non-empty list of 1-D impulse responses")
        super().__init__([trim_rir(h, tail_db, max_taps) for h in rirs], "rirs")
        if int(self.lengths.max()) > N.FIR_MAX_TAPS:
            raise ValueError(f"an impulse response of {int(self.lengths.max())} taps: at most {N.FIR_MAX_TAPS}")
        self.delays = np.asarray([rir_delay(h) for h in self.items], np.int32)


def _wave_list(waves):
    if isinstance(waves, np.ndarray) or not isinstance(waves, (list, tuple)) or not len(waves):
        raise ValueError("`waves` must be a non-empty list of 1-D waveforms")
    return _as_parts(list(waves))[1]


def _choices(choices, count, n, what):
    choices = [int(c) for c in choices]
    if len(choices) != n or any(not 0 <= c < count for c in choices):
        raise ValueError(f"`choices`: one index into the {count} {what} per utterance")
    return choices


def _on_device(parts):
    """(device, one contiguous fp32 buffer of the parts back to back, lengths, starts)"""
    import torch
    from .modeling import _require_gpu
    _require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    parts = [p.to(device=dev, dtype=torch.float32) for p in parts]
    wave = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
    lens = np.asarray([p.shape[0] for p in parts], np.int64)
    return dev, wave, lens, np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)


def reverberate(waves, rirs, choices=None, seed=None, align=True, match_power=True, tail_db=-60.0, max_taps=8000):
    """Reverberation: utterance i convolved with the room impulse response ``rirs[choices[i]]`` -- drawn per utterance with
    ``numpy.random.default_rng(seed)`` when ``choices`` is None -- after ``trim_rir(h, tail_db, max_taps)``.  The output has the
    input's length.  ``align=True`` takes the response's direct path (``rir_delay``) as time zero, so that the speech stays where
    its labels and timestamps expect it; ``align=False`` delays it by the direct path.  ``match_power=True`` scales each output
    to its input's power.  All utterances go through ONE ``w2v2_fir`` call: each output sample is one fp32 chain over the taps
    on the matrix pipe, and each utterance is computed as if it were alone.  ``waves``: a list of 1-D waveforms (numpy, torch
    on the CPU or the GPU).  Returns ``(list of device tensors, views of one buffer; list of the choices)``."""
    import torch
    from .modeling import DeviceTensor
    parts = _wave_list(waves)
    bank = rirs if isinstance(rirs, _RirBank) else _RirBank(rirs, tail_db, max_taps)
    if choices is None:
        choices = np.random.default_rng(seed).integers(0, len(bank), size=len(parts))
    choices = _choices(choices, len(bank), len(parts), "impulse responses")
    dev, wave, lens, starts = _on_device(parts)
    out = torch.empty_like(wave)
    pick = np.asarray(choices, np.int64)
    taps0, ntaps = bank.starts[pick], bank.lengths[pick].astype(np.int32)
    delay = np.ascontiguousarray(bank.delays[pick] if align else np.zeros(len(parts)), np.int32)
    N.check(N.load().w2v2_fir(N.ptr(wave), len(parts), N.ptr(starts), N.ptr(lens), N.ptr(bank.on(dev)), N.ptr(taps0), N.ptr(ntaps),
                              N.ptr(delay), N.ptr(out), N.ptr(starts), int(bool(match_power)), None, N.current_stream()), "w2v2_fir")
    return list(torch.split(DeviceTensor.wrap(out), lens.tolist())), choices


def _snr_range(snr_db):
    lo, hi = (snr_db, snr_db) if np.isscalar(snr_db) else snr_db
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise ValueError(f"snr_db = {snr_db!r}: a finite number of decibels or a (low, high) pair of them")
    return lo, hi


def _offset_ranges(lens, noise_lens):
    """The count of admissible offsets of each utterance: a noise longer than the utterance starts where it still covers the
    utterance without wrapping; a shorter one starts anywhere and wraps."""
    return [int(m - n + 1) if m > n else int(m) for n, m in zip(lens, noise_lens)]


def _draw_noise(rng, lens, bank_lengths, lo, hi, choices=None):
    """choices, offsets, snrs of len(lens) utterances, in this order of draws: n integers (unused where `choices` is given), n
    uniforms in [0, 1) (offset = floor(u * the count of admissible offsets)), n uniforms in [lo, hi)."""
    n = len(lens)
    drawn = [int(c) for c in rng.integers(0, len(bank_lengths), size=n)]
    choices = drawn if choices is None else choices
    u = rng.random(n)
    ranges = _offset_ranges(lens, [bank_lengths[c] for c in choices])
    offsets = [min(int(v * r), r - 1) for v, r in zip(u, ranges)]
    snrs = [float(v) for v in rng.uniform(lo, hi, size=n)]
    return choices, offsets, snrs


def add_noise(waves, noises, snr_db=(5.0, 20.0), choices=None, offsets=None, snrs=None, seed=None):
    """Additive noise: utterance i gets ``noises[c_i]`` from sample ``o_i`` on, wrapping around at the recording's end, at a gain
    that makes the signal-to-noise ratio of the powers ``s_i`` decibels.  What is not given is drawn with
    ``numpy.random.default_rng(seed)`` in this order: the choices (integers), the offsets (uniform over the starts from which a
    longer noise covers the utterance without wrapping; anywhere in a shorter one), the ratios (uniform in ``snr_db = (low,
    high)``; a scalar means fixed).  All utterances go through ONE ``w2v2_mix`` call.  ``waves``: a list of 1-D waveforms.
    Returns ``(list of device tensors, views of one buffer; list of (choice, offset, snr))``."""
    import torch
    from .modeling import DeviceTensor
    parts = _wave_list(waves)
    bank = noises if isinstance(noises, _Bank) else _Bank(noises, "noises")
    lo, hi = _snr_range(snr_db)
    n = len(parts)
    if choices is not None:
        choices = _choices(choices, len(bank), n, "noise recordings")
    choices, drawn_offsets, drawn_snrs = _draw_noise(np.random.default_rng(seed), [p.shape[0] for p in parts], bank.lengths, lo, hi, choices)
    offsets = drawn_offsets if offsets is None else offsets
    offsets = [int(o) for o in offsets]
    if len(offsets) != n or any(not 0 <= o < bank.lengths[c] for o, c in zip(offsets, choices)):
        raise ValueError("`offsets`: one start inside its noise recording per utterance")
    snrs = [float(v) for v in (drawn_snrs if snrs is None else snrs)]
    if len(snrs) != n or not np.isfinite(snrs).all():
        raise ValueError("`snrs`: one finite number of decibels per utterance")
    dev, wave, lens, starts = _on_device(parts)
    out = torch.empty_like(wave)
    pick = np.asarray(choices, np.int64)
    scale = np.asarray([10.0 ** (-v / 20.0) for v in snrs], np.float64)
    noise0, noise_len, first = bank.starts[pick], bank.lengths[pick], np.asarray(offsets, np.int64)      # (held until the call returns)
    N.check(N.load().w2v2_mix(N.ptr(wave), n, N.ptr(starts), N.ptr(lens), N.ptr(bank.on(dev)), N.ptr(noise0), N.ptr(noise_len),
                              N.ptr(first), N.ptr(scale), N.ptr(out), N.ptr(starts), None, N.current_stream()), "w2v2_mix")
    return list(torch.split(DeviceTensor.wrap(out), lens.tolist())), list(zip(choices, offsets, snrs))


def _prob(p, what):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{what} = {p} outside [0, 1]")
    return p


class Augment:
    """Speed perturbation, then reverberation, then additive noise -- the order of the Kaldi recipes -- on the device:
    ``waves, info = aug(waves)`` for a list of 1-D waveforms.  Every utterance is played at a factor drawn from ``speed`` (None:
    no such stage), is reverberated with probability ``rir_prob`` by an impulse response drawn from ``rirs`` (None: no such
    stage) and gets noise with probability ``noise_prob`` from a recording drawn from ``noises`` (None: no such stage) at a
    ratio uniform in ``snr_db``.  Each stage is one kernel call over the utterances it selects; an utterance a stage does not
    select passes through with its bits.  The impulse responses (after ``trim_rir``) and the noise recordings are uploaded once
    per device and kept.

    All draws come from ONE ``numpy.random.default_rng(seed)``, which lives as long as the object, in this order per call of n
    utterances: n speed choices (integers; if there is a speed stage); n uniforms (reverberated where below ``rir_prob``) and n
    impulse-response choices (if there are rirs); n uniforms (noise where below ``noise_prob``), n noise choices, n uniforms for
    the offsets and n ratios (if there are noises).  The counts do not depend on what is selected.  An offset depends on the
    utterance's length AFTER the speed stage (``add_noise``).

    ``aug.plan(lengths)`` returns what the next call on utterances of these lengths will draw, without drawing it and without
    touching the device.  ``info`` is that plan: a dict of ``lengths`` (the input's), ``speed_choices`` and ``speed`` (the
    factors), ``rir`` (per utterance the choice, or None) and ``noise`` (per utterance ``(choice, offset, snr)``, or None).
    Feeding it back through the explicit arguments of ``speed_perturb``, ``reverberate`` and ``add_noise`` reproduces the bits."""

    def __init__(self, speed=(0.9, 1.0, 1.1), rirs=None, rir_prob=0.5, noises=None, noise_prob=0.5, snr_db=(5.0, 20.0), seed=0,
                 tail_db=-60.0, max_taps=8000):
        self.speed = None if speed is None else [float(f) for f in speed]
        if self.speed is not None:
            if not self.speed:
                raise ValueError("`speed` is empty")
            self._ratios = [speed_ratio(f) for f in self.speed]
        self.rir_prob, self.noise_prob = _prob(rir_prob, "rir_prob"), _prob(noise_prob, "noise_prob")
        self.snr_db = _snr_range(snr_db)
        self.rirs = None if rirs is None else _RirBank(rirs, tail_db, max_taps)
        self.noises = None if noises is None else _Bank(noises, "noises")
        self._rng = np.random.default_rng(seed)

    def _draw(self, rng, lengths):
        n = len(lengths)
        info = {"lengths": [int(v) for v in lengths], "speed_choices": None, "speed": None, "rir": [None] * n, "noise": [None] * n}
        lens = info["lengths"]
        if self.speed is not None:
            picks = [int(c) for c in rng.integers(0, len(self.speed), size=n)]
            info["speed_choices"], info["speed"] = picks, [self.speed[c] for c in picks]
            lens = [-(-m * self._ratios[c][0] // self._ratios[c][1]) for m, c in zip(lens, picks)]
        if self.rirs is not None:
            take, which = rng.random(n) < self.rir_prob, rng.integers(0, len(self.rirs), size=n)
            info["rir"] = [int(c) if t else None for t, c in zip(take, which)]
        if self.noises is not None:
            take = rng.random(n) < self.noise_prob
            drawn = _draw_noise(rng, lens, self.noises.lengths, *self.snr_db)
            info["noise"] = [(c, o, s) if t else None for t, c, o, s in zip(take, *drawn)]
        return info

    def plan(self, lengths):
        lengths = [int(v) for v in lengths]
        if not lengths or min(lengths) < 1:
            raise ValueError("`lengths`: a non-empty list of positive sample counts")
        return self._draw(copy.deepcopy(self._rng), lengths)

    def __call__(self, waves):
        parts = _wave_list(waves)
        info = self._draw(self._rng, [p.shape[0] for p in parts])
        out = list(parts)
        if self.speed is not None:
            out, _ = speed_perturb(out, self.speed, choices=info["speed_choices"])
        mine = [i for i, c in enumerate(info["rir"]) if c is not None]
        if mine:
            done, _ = reverberate([out[i] for i in mine], self.rirs, choices=[info["rir"][i] for i in mine])
            for i, t in zip(mine, done):
                out[i] = t
        mine = [i for i, c in enumerate(info["noise"]) if c is not None]
        if mine:
            c, o, s = zip(*(info["noise"][i] for i in mine))
            done, _ = add_noise([out[i] for i in mine], self.noises, choices=c, offsets=o, snrs=s)
            for i, t in zip(mine, done):
                out[i] = t
        if self.speed is None:          # (the speed stage puts every utterance on the device; without it the untouched ones follow here)
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            out = [t.to(device=dev, dtype=torch.float32) for t in out]
        return out, info
