"""The host side of the augmentation (wav2vec2.audio: rir_delay, trim_rir, Augment.plan, the argument checks) and
tests/augment_reference.py itself against numpy.convolve.  No device is needed."""

import numpy as np
import pytest

import augment_reference as A
from wav2vec2 import _native as N
from wav2vec2.audio import Augment, add_noise, reverberate, rir_delay, trim_rir


@pytest.mark.parametrize("K,n", [(1, 1), (1, 9), (5, 3), (37, 150), (129, 64)])
def test_reference_convolution_agrees_with_numpy(K, n):
    rng = np.random.default_rng(K + n)
    x, h = rng.integers(-8, 9, size=n).astype(np.float64), rng.integers(-3, 4, size=K).astype(np.float64)
    full = np.convolve(x, h)                                   # full[m] = sum_k h[k] x[m - k]
    mags = np.convolve(np.abs(x), np.abs(h))
    for d in sorted({0, K // 2, K - 1}):
        y, mag = A.fir(x, h, d)
        assert np.array_equal(y, full[d:d + n]) and np.array_equal(mag, mags[d:d + n])
        assert np.array_equal(A.fir_chain32(x, h, d), full[d:d + n].astype(np.float32))


def test_reference_chain_is_the_fma_chain_and_pins_the_order():
    """On integers times powers of two every product is exact in fp32, so float32(acc + h x) is the fmaf: the emulation equals a
    chain in exact rational arithmetic rounded once per step, and the descending chain differs from the ascending one."""
    from fractions import Fraction
    rng = np.random.default_rng(137)
    dy = lambda n: (rng.integers(-2047, 2048, size=n) * 2.0 ** rng.integers(-12, 13, size=n)).astype(np.float32)
    x, h, d = dy(150), dy(37), 18
    got = A.fir_chain32(x, h, d)
    for n in range(0, 150, 7):
        acc = np.float32(0.0)
        for k in range(37):
            i = n + d - k
            xv = Fraction(float(x[i])) if 0 <= i < 150 else Fraction(0)
            exact = Fraction(float(acc)) + Fraction(float(h[k])) * xv
            acc = np.float32(float(exact))          # (two roundings, fp64 then fp32, are one for a sum of two fp32 numbers: 53 >= 2 * 24 + 2)
        assert acc == got[n]
    assert (A.fir_chain32(x, h, d, descending=True) != got).sum() > 30


def test_reference_gains():
    x = np.asarray([3.0, 4.0], np.float32)
    assert A.sumsq(x) == 25.0 and A.fir_gain(x, 2 * x) == 0.5 and A.fir_gain(x, 0 * x) == 1.0 and A.fir_gain(0 * x, x) == 1.0
    assert A.mix_gain(x, 2 * x, 0.1) == pytest.approx(0.05) and A.mix_gain(x, 0 * x, 1.0) == 0.0 and A.mix_gain(0 * x, x, 1.0) == 0.0
    assert A.noise_window(np.arange(5), 3, 9).tolist() == [3, 4, 0, 1, 2, 3, 4, 0, 1]


def test_rir_delay_and_trim():
    h = np.zeros(100)
    h[[3, 17, 40]] = [0.5, -2.0, 1.0]
    assert rir_delay(h) == 17 and rir_delay(-h) == 17 and rir_delay([1.0, -1.0]) == 0
    # a geometric response a^k: E[n] / E[0] = a^(2n) (its own tail beyond N is below 1e-30), so the -60 dB point is the first n
    # with a^(2n) < 1e-6
    a, N_ = 0.99, 6000
    g = a ** np.arange(N_)
    want = int(np.ceil(-6.0 / (2.0 * np.log10(a))))
    cut = len(trim_rir(g))
    assert abs(cut - want) <= 1 and a ** (2 * (cut + 1)) < 1e-6 <= a ** (2 * (cut - 1)), (cut, want)
    assert abs(len(trim_rir(g, tail_db=-30.0)) - int(np.ceil(-3.0 / (2.0 * np.log10(a))))) <= 1
    t = trim_rir(g)
    assert t.dtype == np.float32 and np.array_equal(t, g[:cut].astype(np.float32))
    assert len(trim_rir(g, max_taps=100)) == 100 and len(trim_rir(g, max_taps=10 ** 6)) == cut
    # never before the direct path: a late peak after an early decay, and a max_taps below it
    late = np.concatenate((g[:3000], [50.0], np.zeros(10)))
    assert len(trim_rir(late, max_taps=8000)) == 3001 and len(trim_rir(late, max_taps=100)) == 3001
    assert len(trim_rir(np.ones(20000))) == 8000                # max_taps defaults to half a second
    for bad in (np.zeros(10), np.zeros((2, 5)), np.zeros(0), [1.0, np.nan]):
        with pytest.raises(ValueError):
            trim_rir(bad)
    with pytest.raises(ValueError):
        trim_rir(g, max_taps=0)
    with pytest.raises(ValueError):
        trim_rir(g, tail_db=3.0)


def banks():
    rng = np.random.default_rng(30)
    rirs = [rng.standard_normal(k) * np.exp(-np.arange(k) / 50.0) for k in (900, 2500, 300)]
    noises = [rng.standard_normal(n).astype(np.float32) for n in (500, 30000, 4001)]
    return rirs, noises


def test_augment_plan_is_deterministic():
    rirs, noises = banks()
    lengths = [3000, 4001, 1, 2500, 900, 7777, 9000, 10]
    a, b = Augment(rirs=rirs, noises=noises, seed=3), Augment(rirs=rirs, noises=noises, seed=3)
    plan = a.plan(lengths)
    assert plan == a.plan(lengths) == b.plan(lengths)
    assert plan != Augment(rirs=rirs, noises=noises, seed=4).plan(lengths)
    assert plan["lengths"] == lengths and len(plan["speed"]) == len(plan["rir"]) == len(plan["noise"]) == len(lengths)
    assert set(plan["speed"]) <= {0.9, 1.0, 1.1} and plan["speed"] == [a.speed[c] for c in plan["speed_choices"]]
    ratio = {0.9: (10, 9), 1.0: (1, 1), 1.1: (10, 11)}
    for n, f, r, v in zip(lengths, plan["speed"], plan["rir"], plan["noise"]):
        assert r is None or 0 <= r < 3
        if v is not None:
            c, o, snr = v
            m, after = len(noises[c]), -(-n * ratio[f][0] // ratio[f][1])       # offsets see the length after the speed stage
            assert 0 <= o < m and 5.0 <= snr < 20.0 and (o + after <= m or m <= after)
    # the number of draws does not depend on what is selected
    none = Augment(rirs=rirs, rir_prob=0.0, noises=noises, noise_prob=0.0, seed=3).plan(lengths)
    assert none["speed_choices"] == plan["speed_choices"] and none["rir"] == [None] * 8 and none["noise"] == [None] * 8
    every = Augment(rirs=rirs, rir_prob=1.0, noises=noises, noise_prob=1.0, seed=3).plan(lengths)
    assert None not in every["rir"] and None not in every["noise"]
    assert all(p is None or p == e for p, e in zip(plan["rir"], every["rir"]))
    assert all(p is None or p == e for p, e in zip(plan["noise"], every["noise"]))
    off = Augment(speed=None, seed=3).plan(lengths)
    assert off["speed"] is None and off["rir"] == [None] * 8
    with pytest.raises(ValueError):
        a.plan([])
    with pytest.raises(ValueError):
        a.plan([10, 0])


def test_argument_errors_need_no_device():
    rirs, noises = banks()
    waves = [np.zeros(100, np.float32) + 1.0]
    for bad in ([], np.zeros((2, 100), np.float32), [np.zeros((2, 100), np.float32)], [np.zeros(0, np.float32)]):
        with pytest.raises(ValueError):
            reverberate(bad, rirs)
        with pytest.raises(ValueError):
            add_noise(bad, noises)
    for bad in ([], [np.zeros(50)], [np.zeros((2, 5))]):
        with pytest.raises(ValueError):
            reverberate(waves, bad)
    with pytest.raises(ValueError):
        reverberate(waves, rirs, choices=[3])
    with pytest.raises(ValueError):
        add_noise(waves, noises, choices=[-1])
    with pytest.raises(ValueError):
        add_noise(waves, noises, snr_db=float("nan"))
    with pytest.raises(ValueError):
        add_noise(waves, noises, snrs=[float("inf")])
    with pytest.raises(ValueError):
        reverberate(waves, [np.ones(N.FIR_MAX_TAPS + 1)], tail_db=-200.0, max_taps=10 ** 6)
    for kw in (dict(rir_prob=1.01), dict(noise_prob=-0.5), dict(speed=()), dict(snr_db=float("inf")), dict(rirs=[]), dict(noises=[])):
        with pytest.raises(ValueError):
            Augment(**kw)


def test_prototypes_and_constants():
    assert "w2v2_fir" in N.PROTOTYPES and "w2v2_mix" in N.PROTOTYPES
    assert len(N.PROTOTYPES["w2v2_fir"][1]) == 13 and len(N.PROTOTYPES["w2v2_mix"][1]) == 13
    assert (N.FIR_TILE, N.FIR_CHUNK, N.FIR_MAX_TAPS) == (8192, 2048, 65536)
    lib = N.load()
    assert hasattr(lib, "w2v2_fir") and hasattr(lib, "w2v2_mix")
    import wav2vec2
    for name in ("reverberate", "add_noise", "Augment", "rir_delay", "trim_rir"):
        assert name in wav2vec2.__all__ and hasattr(wav2vec2, name)
