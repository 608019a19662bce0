"""The resampler off the GPU: the fp64 reference (tests/resample_reference.py) pinned against scipy's
resample_poly and against the zero-stuffed convolution it abbreviates; the default filter's pass band and stop band on tones;
w2v2_resample_design and w2v2_resample_length from the library (host code, no device); the host logic of wav2vec2.audio."""

import ctypes as C

import numpy as np
import pytest

import resample_reference as R
from wav2vec2 import _native as N

RATES = [48000, 44100, 22050, 14400, 17600, 8000]
LENGTHS = [1, 7, 399, 4001]
W2V2_EINVAL = -1


def prototype(L, K, lead, table):
    """The filter of the zero-stuffed formulation, p[(t - lead) L - r] = table[r][t], centred in an odd-length array."""
    c = max(lead * L + L - 1, (K - 1 - lead) * L)
    p = np.zeros(2 * c + 1, np.float64)
    t, r = np.meshgrid(np.arange(K), np.arange(L))
    p[c + (t - lead) * L - r] = table[r, t]
    return p, c


@pytest.mark.parametrize("rate", RATES)
def test_reference_equals_scipy_resample_poly(rate):
    signal = pytest.importorskip("scipy.signal")
    L, M, K, lead, table = R.design(rate)
    p, _ = prototype(L, K, lead, table)
    for n in LENGTHS:
        x = np.random.default_rng(n).standard_normal(n)
        out, _ = R.apply(x, L, M, K, lead, table)
        ref = signal.resample_poly(x, L, M, window=p) / L
        assert out.shape == ref.shape == (R.out_length(n, L, M),)
        err = np.abs(out - ref).max()
        print(f"{rate} -> 16000, {n} samples: max |reference - resample_poly / L| = {err:.2e}")
        assert err <= 1e-13


@pytest.mark.parametrize("rate", RATES)
def test_reference_equals_the_zero_stuffed_convolution(rate):
    """No scipy needed: out[n] = sum_k p[n M - k L] x[k], the convolution of the zero-stuffed signal read at every M-th sample."""
    L, M, K, lead, table = R.design(rate)
    p, c = prototype(L, K, lead, table)
    for n in LENGTHS[:3]:
        x = np.random.default_rng(n).standard_normal(n)
        out, _ = R.apply(x, L, M, K, lead, table)
        k = np.arange(n)
        ref = np.empty_like(out)
        for i in range(len(out)):
            j = c + i * M - k * L
            ok = (j >= 0) & (j < len(p))
            ref[i] = np.sum(p[j[ok]] * x[ok])
        assert np.abs(out - ref).max() <= 1e-13


def _tone(rate, freq, seconds=0.5):
    return np.sin(2.0 * np.pi * freq * np.arange(int(rate * seconds)) / rate + 0.3)


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
@pytest.mark.parametrize("fraction", [0.1, 0.5, 0.8])
def test_default_filter_passes_tones(rate, fraction):
    """A tone at `fraction` of the lower Nyquist comes out as the same tone at 16 kHz: the largest error over the middle half of
    0.5 s is at most -100 dB of the amplitude, with the table rounded to fp32 as the device holds it."""
    L, M, K, lead, table = R.design(rate)
    freq = fraction * min(rate, 16000) / 2.0
    out, _ = R.apply(_tone(rate, freq), L, M, K, lead, table.astype(np.float32))
    n = np.arange(len(out))
    ideal = np.sin(2.0 * np.pi * freq * n / 16000.0 + 0.3)
    mid = slice(len(out) // 4, 3 * len(out) // 4)
    db = 20.0 * np.log10(np.abs(out - ideal)[mid].max())
    print(f"{rate} -> 16000, tone at {fraction} of Nyquist: error {db:.1f} dB")
    assert db <= -100.0


@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("fraction", [1.1, 1.5])
def test_default_filter_stops_what_would_alias(rate, fraction):
    L, M, K, lead, table = R.design(rate)
    out, _ = R.apply(_tone(rate, fraction * 8000.0), L, M, K, lead, table.astype(np.float32))
    mid = slice(len(out) // 4, 3 * len(out) // 4)
    db = 20.0 * np.log10(np.abs(out)[mid].max())
    print(f"{rate} -> 16000, tone at {fraction} of the new Nyquist: {db:.1f} dB")
    assert db <= -100.0


# ---- the library's host code ----

def lib_design(rate_in, rate_out=16000, zeros=32, rolloff=0.95, beta=12.0, capacity=None, with_table=True):
    lib = N.load()
    size = [C.c_int32() for _ in range(4)]
    args = (rate_in, rate_out, zeros, rolloff, beta, *(C.byref(v) for v in size))
    rc = lib.w2v2_resample_design(*args, None, 0)
    L, M, K, lead = (v.value for v in size)
    if rc or not with_table:
        return rc, (L, M, K, lead), None
    table = np.zeros((L, K), np.float32)
    rc = lib.w2v2_resample_design(*args, N.ptr(table), table.size if capacity is None else capacity)
    return rc, (L, M, K, lead), table


def ulps(a, b):
    i, j = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(np.where(i < 0, -(i & 0x7FFFFFFF), i) - np.where(j < 0, -(j & 0x7FFFFFFF), j))


@pytest.mark.parametrize("rates", [(r, 16000) for r in RATES] + [(16000, 8000), (9, 10), (11, 10), (16000, 44100)])
def test_library_design_equals_the_reference(rates):
    rc, sizes, table = lib_design(*rates)
    assert rc == 0, N.last_error()
    L, M, K, lead, table64 = R.design(*rates)
    assert sizes == (L, M, K, lead)
    worst = int(ulps(table, table64.astype(np.float32)).max())
    print(f"{rates}: L {L} M {M} K {K} lead {lead}; table within {worst} ulp of the fp64 reference rounded to fp32")
    assert worst <= 1
    assert np.abs(table.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6


def test_library_design_other_parameters_and_the_copy():
    rc, sizes, table = lib_design(44100, 16000, zeros=8, rolloff=0.9, beta=6.0)
    L, M, K, lead, table64 = R.design(44100, 16000, 8, 0.9, 6.0)
    assert rc == 0 and sizes == (L, M, K, lead) and ulps(table, table64.astype(np.float32)).max() <= 1
    for rate in (16000, 1, 44100):
        rc, sizes, table = lib_design(rate, rate)
        assert rc == 0 and sizes == (1, 1, 1, 0) and table.tolist() == [[1.0]]


def test_library_design_rejects():
    rc, (L, M, K, lead), _ = lib_design(48000, with_table=False)
    assert rc == 0 and (L, M, K, lead) == (1, 3, 204, 101)
    rc, _, _ = lib_design(48000, capacity=L * K - 1)
    assert rc == W2V2_EINVAL and "table_capacity" in N.last_error()
    rc, _, _ = lib_design(16000, capacity=0)
    assert rc == W2V2_EINVAL and "table_capacity" in N.last_error()
    for kw, msg in [(dict(rate_in=0), "rates"), (dict(rate_in=48000, rate_out=-1), "rates"), (dict(rate_in=48000, zeros=0), "zeros"),
                    (dict(rate_in=48000, rolloff=0.0), "rolloff"), (dict(rate_in=48000, rolloff=1.5), "rolloff"),
                    (dict(rate_in=48000, beta=-1.0), "beta"), (dict(rate_in=48000, beta=float("nan")), "beta")]:
        rc, _, _ = lib_design(**kw)
        assert rc == W2V2_EINVAL and msg in N.last_error(), (kw, N.last_error())
    lib = N.load()
    assert lib.w2v2_resample_design(48000, 16000, 32, 0.95, 12.0, None, None, None, None, None, 0) == W2V2_EINVAL


def test_library_length_is_the_ceiling():
    lib = N.load()
    big = (1 << 31) - 1
    for n, L, M in [(0, 1, 3), (1, 1, 3), (2, 1, 3), (3, 1, 3), (4, 1, 3), (1, 160, 441), (440, 160, 441), (441, 160, 441), (442, 160, 441),
                    (7, 2, 1), (big, 4096, 1), (big, 1, big), (big, 4095, 4096), (1 << 40, 10, 9), (5, 1, 1)]:
        assert lib.w2v2_resample_length(n, L, M) == -(-n * L // M), (n, L, M)
    for n, L, M in [(-1, 1, 3), (5, 0, 3), (5, 1, 0)]:
        assert lib.w2v2_resample_length(n, L, M) == -1


# ---- wav2vec2.audio: what needs no device ----

def test_resampled_length_and_resampler_attributes():
    from wav2vec2.audio import Resampler, resampled_length
    assert resampled_length(48000, 48000) == 16000 and resampled_length(48001, 48000) == 16001
    assert resampled_length(441, 44100) == 160 and resampled_length(442, 44100) == 161
    assert resampled_length(5, 8000) == 10 and resampled_length(0, 8000) == 0 and resampled_length(7, 16000) == 7
    r = Resampler(44100)
    assert (r.L, r.M, r.taps, r.lead) == (160, 441, 186, 92) and r.table.shape == (160, 186) and r.table.dtype == np.float32
    assert [Resampler(x).taps for x in RATES] == [204, 186, 94, 68, 76, 68]
    for bad in (0, -8000, 44100.0, None):
        with pytest.raises(ValueError):
            Resampler(bad)
        with pytest.raises(ValueError):
            resampled_length(10, bad)
    with pytest.raises(ValueError):
        Resampler(48000, 0)
    with pytest.raises(ValueError):
        Resampler(16001, 16000 * 4099)        # 4099 x 16000 and 16001 share no factor: more phases than the kernel takes


def test_speed_ratio():
    from wav2vec2.audio import speed_ratio
    assert speed_ratio(0.9) == (10, 9) and speed_ratio(1.1) == (10, 11) and speed_ratio(1.0) == (1, 1)
    assert speed_ratio(0.95) == (20, 19) and speed_ratio(1.05) == (20, 21) and speed_ratio(2) == (1, 2) and speed_ratio(0.5) == (2, 1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 0.001):
        with pytest.raises(ValueError):
            speed_ratio(bad)
    # the length rule: ceil(len / f) for factors that are such fractions
    for f in (0.9, 1.1, 1.0, 0.95):
        L, M = speed_ratio(f)
        for n in (1, 9, 10, 11, 16000, 16001):
            assert R.out_length(n, L, M) == -(-n * L // M) == int(np.ceil(n * L / M))


def test_speed_perturb_argument_errors_need_no_device():
    from wav2vec2.audio import speed_perturb
    x = np.zeros(100, np.float32)
    for args, kw in [(([],), {}), ((x,), {}), (([x],), dict(factors=())), (([x],), dict(factors=(0.0, 1.0))), (([x],), dict(factors=(-1.1,))),
                     (([x],), dict(choices=[3])), (([x, x],), dict(choices=[0])), (([np.zeros((2, 50), np.float32)],), {}),
                     (([np.zeros(0, np.float32)],), {})]:
        with pytest.raises(ValueError):
            speed_perturb(*args, **kw)


def test_speed_perturb_draws_are_those_of_the_seeded_generator():
    """What speed_perturb(seed=s) chooses: default_rng(s).integers over the factors, one per utterance (the GPU test checks
    that the call returns these)."""
    draws = np.random.default_rng(3).integers(0, 3, size=8)
    assert np.array_equal(draws, np.random.default_rng(3).integers(0, 3, size=8))
    assert set(draws.tolist()) <= {0, 1, 2}
