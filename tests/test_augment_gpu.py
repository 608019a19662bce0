"""Reverberation and additive noise on the GPU (w2v2_fir, w2v2_mix, csrc/augment.hip) against
tests/augment_reference.py: the index arithmetic exactly on integer data, the ascending fp32 chain bit for bit, real filters against
fp64 within the bound of a length-K fp32 chain, isolation and position independence bitwise, the gains, identities, the Python
surface (wav2vec2.audio) and the C ABI's argument errors.  The harness is the one of tests/test_resample_gpu.py."""

import numpy as np
import pytest

import augment_reference as A

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def consts():
    from wav2vec2 import _native as N
    assert N.FIR_TILE == 8192 and N.FIR_CHUNK == 2048 and N.FIR_MAX_TAPS == 65536
    return N.FIR_TILE, N.FIR_CHUNK


def layout(lens, out_lens, in_off, out_off, shift, order):
    """Segment i starts in_off[i % 3] floats behind a 64-float (256-byte) boundary of the input buffer (moved by `shift`) and its
    output out_off[i % 3] floats behind one of the output buffer; `order` lays the segments out in another order."""
    n = len(lens)
    in0, out0 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ci, co = 64 + shift, 64
    for i in (range(n) if order is None else order):
        in0[i] = -(-ci // 64) * 64 + shift + in_off[i % 3]
        out0[i] = -(-co // 64) * 64 + out_off[i % 3]
        ci, co = in0[i] + lens[i], out0[i] + out_lens[i]
    return in0, out0, int(ci) + 64, int(co) + 64


def packed(torch, arrays, starts, total):
    """The arrays at their starts in a buffer of NaN, on the device."""
    host = np.full(total, np.nan, np.float32)
    for s, a in zip(arrays, starts):
        host[a:a + len(s)] = s
    return torch.from_numpy(host).cuda()


def collect(y, out0, lens):
    got = y.cpu().numpy()
    rest = np.ones(len(got), bool)
    outs = []
    for a, m in zip(out0, lens):
        outs.append(got[a:a + m].copy())
        rest[a:a + m] = False
    assert (got[rest] == SENTINEL).all(), "a float outside the segments' output ranges was written"
    return outs


def run_fir(torch, segs, filters, match_power=False, in_off=(0, 1, 3), out_off=(3, 0, 1), shift=0, order=None, want_gain=True):
    """One w2v2_fir call.  segs: 1-D float32 arrays; filters: one (taps, delay) per segment.  The input between the segments and
    the taps between the filters are NaN; the output is pre-filled with a sentinel that must survive everywhere outside the
    segments' ranges.  Returns (outputs, gains)."""
    from wav2vec2 import _native as N
    n = len(segs)
    lens = np.asarray([len(s) for s in segs], np.int64)
    in0, out0, ni, no = layout(lens, lens, in_off, out_off, shift, order)
    x = packed(torch, segs, in0, ni)
    ntaps = np.asarray([len(h) for h, _ in filters], np.int32)
    taps0 = (np.concatenate(([0], np.cumsum(ntaps + 5)[:-1])) + 3 + shift).astype(np.int64)
    taps = packed(torch, [np.asarray(h, np.float32) for h, _ in filters], taps0, int(taps0[-1] + ntaps[-1] + 7))
    delay = np.asarray([d for _, d in filters], np.int32)
    y = torch.full((no,), SENTINEL, dtype=torch.float32, device="cuda")
    gain = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device="cuda") if want_gain else None
    N.check(N.load().w2v2_fir(N.ptr(x), n, N.ptr(in0), N.ptr(lens), N.ptr(taps), N.ptr(taps0), N.ptr(ntaps), N.ptr(delay), N.ptr(y),
                              N.ptr(out0), int(match_power), N.ptr(gain), N.current_stream()), "w2v2_fir")
    g = None
    if want_gain:
        g = gain.cpu().numpy()
        assert (g[n:] == SENTINEL).all()
        g = g[:n]
    return collect(y, out0, lens), g


def run_mix(torch, segs, noises, offsets, scales, in_off=(0, 1, 3), out_off=(3, 0, 1), shift=0):
    """One w2v2_mix call: segment i with its own noise recording noises[i] from offsets[i] on at scales[i]."""
    from wav2vec2 import _native as N
    n = len(segs)
    lens = np.asarray([len(s) for s in segs], np.int64)
    in0, out0, ni, no = layout(lens, lens, in_off, out_off, shift, None)
    x = packed(torch, segs, in0, ni)
    nlen = np.asarray([len(v) for v in noises], np.int64)
    noise0 = (np.concatenate(([0], np.cumsum(nlen + 5)[:-1])) + 3).astype(np.int64)
    v = packed(torch, noises, noise0, int(noise0[-1] + nlen[-1] + 7))
    y = torch.full((no,), SENTINEL, dtype=torch.float32, device="cuda")
    gain = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device="cuda")
    offsets, scales = np.asarray(offsets, np.int64), np.asarray(scales, np.float64)      # (held until the call returns)
    N.check(N.load().w2v2_mix(N.ptr(x), n, N.ptr(in0), N.ptr(lens), N.ptr(v), N.ptr(noise0), N.ptr(nlen), N.ptr(offsets), N.ptr(scales),
                              N.ptr(y), N.ptr(out0), N.ptr(gain), N.current_stream()), "w2v2_mix")
    g = gain.cpu().numpy()
    assert (g[n:] == SENTINEL).all()
    return collect(y, out0, lens), g[:n]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1. index arithmetic, exact ----

@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 63, 64, 65, "chunk-32", "chunk-31", "chunk-30", "chunk-1", "chunk", "chunk+1"])
def test_integer_filters_are_exact(torch_mod, K):
    """Integer taps in [-3, 3] on integer samples in [-8, 8]: every partial sum stays below 2^24 (2049 * 24), so fp32 is exact in
    any order and the result must EQUAL the integer convolution.  A dropped or shifted edge tap shows here and nowhere else; the
    edge taps are +-3.  K around the kernel's chunk of the contraction -- which runs over j in [0, K + 31), hence also K + 31
    around it -- and lengths around the block's tile."""
    T, C = consts()
    if isinstance(K, str):
        K = C + int(K[5:] or 0)
    rng = np.random.default_rng(K)
    lens = [1, 31, 32, 33, T - 1, T, T + 1]
    segs, filters = [], []
    for d in sorted({0, K // 2, K - 1}):
        for n in lens:
            h = rng.integers(-3, 4, size=K).astype(np.float32)
            h[0], h[-1] = rng.choice([-3.0, 3.0], size=2)
            segs.append(rng.integers(-8, 9, size=n).astype(np.float32))
            filters.append((h, d))
    outs, gains = run_fir(torch_mod, segs, filters)
    assert (gains == 1.0).all()
    for s, (h, d), o in zip(segs, filters, outs):
        ref = A.fir(s, h, d)[0]
        bad = np.flatnonzero(o != ref)
        assert bad.size == 0, f"K {K} delay {d}, {len(s)} samples: {bad.size} outputs differ, first at {bad[:5]}"


# ---- 2. the chain, bit for bit ----

def dyadic(rng, n):
    return (rng.integers(-2047, 2048, size=n) * 2.0 ** rng.integers(-12, 13, size=n)).astype(np.float32)


@pytest.mark.parametrize("K", [37, 64, 129])
def test_the_ascending_chain_bit_for_bit(torch_mod, K):
    """Taps and samples are integers in [-2047, 2047] times 2^e, e in [-12, 12]: every product is exact in fp32, so numpy's
    float32(acc + h[k] * x[.]) IS the fmaf, and the ascending-k chain must be matched as values.  (The descending chain differs
    from it at most outputs, so this pins the order.)"""
    T, _ = consts()
    rng = np.random.default_rng(100 + K)
    segs = [dyadic(rng, n) for n in (150, 1000, T + 5)]
    filters = [(dyadic(rng, K), d) for d in (0, K // 2, K - 1)]
    outs, _ = run_fir(torch_mod, segs, filters)
    differs = 0
    for s, (h, d), o in zip(segs, filters, outs):
        ref = A.fir_chain32(s, h, d)
        bad = np.flatnonzero(o != ref)
        assert bad.size == 0, f"K {K} delay {d}, {len(s)} samples: {bad.size} outputs leave the chain, first at {bad[:5]}"
        differs += int((A.fir_chain32(s, h, d, descending=True) != ref).sum())
    assert differs > 0, "the data do not tell the ascending chain from the descending one"


# ---- 3. real filters against fp64 ----

def mixed_scales(rng, n):
    return (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 100.0], size=n)).astype(np.float32)


@pytest.mark.parametrize("K", [4000, 16000])
def test_decaying_filters_within_the_chain_bound(torch_mod, K):
    """|got - ref| <= 1.01 (K + 1) 2^-24 sum_k |h[k] x[.]|: the textbook bound of a length-K fp32 chain (K roundings of the running
    sum of at most 2^-24 relative each, one more for the margin of the fp64 reference itself), as tests/test_resample_gpu.py."""
    from wav2vec2.audio import rir_delay, trim_rir
    T, _ = consts()
    rng = np.random.default_rng(K)
    raw = rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 5.0))
    h = trim_rir(raw, max_taps=K)
    assert K // 2 < len(h) <= K and h.dtype == np.float32
    d = rir_delay(h)
    segs = [mixed_scales(rng, n) for n in (1000, T + 100)]
    outs, _ = run_fir(torch_mod, segs, [(h, d), (h, 0)])
    worst = 0.0
    for s, dd, o in zip(segs, (d, 0), outs):
        ref, mag = A.fir(s, h, dd)
        bound = 1.01 * (len(h) + 1) * 2.0 ** -24 * mag
        err = np.abs(o.astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    print(f"{len(h)} taps: largest error is {100 * worst:.1f} % of the bound")


# ---- 4. isolation and position independence, bitwise ----

def test_segments_are_computed_as_if_alone(torch_mod):
    T, C = consts()
    rng = np.random.default_rng(5)
    lens = [700, 1, 2 * T + 3, 33, 2500]
    taps = [300, C + 70, 129, 5, 1000]
    segs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    filters = [((rng.standard_normal(k) * np.exp(-np.arange(k) / 200.0)).astype(np.float32), d)
               for k, d in zip(taps, (0, 17, 128, 4, 500))]
    for match_power in (False, True):
        together, gains = run_fir(torch_mod, segs, filters, match_power)
        again, gains2 = run_fir(torch_mod, segs, filters, match_power)
        for i in range(len(segs)):
            assert same_bits(again[i], together[i]) and gains[i] == gains2[i], f"segment {i}, the same call twice"
            alone, g = run_fir(torch_mod, [segs[i]], [filters[i]], match_power)
            assert same_bits(alone[0], together[i]) and g[0] == gains[i], f"segment {i} alone"
        rev = list(range(len(segs)))[::-1]
        laid, g = run_fir(torch_mod, segs, filters, match_power, order=rev, shift=1, in_off=(3, 3, 0), out_off=(1, 0, 0))
        for i in range(len(segs)):
            assert same_bits(laid[i], together[i]) and g[i] == gains[i], f"segment {i} elsewhere in the buffers"
    poisoned = list(segs)
    poisoned[1] = np.full(1, np.nan, np.float32)
    poisoned[3] = np.full(33, np.nan, np.float32)
    got, _ = run_fir(torch_mod, poisoned, filters, True)
    for i in (0, 2, 4):
        assert same_bits(got[i], together[i]), f"segment {i} beside NaN neighbours"


def test_mix_segments_are_computed_as_if_alone(torch_mod):
    rng = np.random.default_rng(6)
    lens = [700, 1, 9000, 33]
    segs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    noises = [rng.standard_normal(n).astype(np.float32) for n in (100, 5, 20000, 33)]
    offsets, scales = [99, 2, 15000, 0], [0.5, 1.0, 0.1, 2.0]
    together, gains = run_mix(torch_mod, segs, noises, offsets, scales)
    for i in range(len(segs)):
        alone, g = run_mix(torch_mod, [segs[i]], [noises[i]], [offsets[i]], [scales[i]], shift=1)
        assert same_bits(alone[0], together[i]) and g[0] == gains[i], f"segment {i} alone"


# ---- 5. gains ----

def test_match_power_gain_and_output(torch_mod):
    """gain_dev against fp64 within 2^-23 relative (one fp32 rounding, 2^-24, doubled; the fp64 sums' own error is below
    len * 2^-53); given the device's g, the output is float32(g) * float32(y) exactly, y from a call without match_power."""
    rng = np.random.default_rng(7)
    segs = [rng.standard_normal(n).astype(np.float32) for n in (10000, 4097, 50)]
    filters = [((rng.standard_normal(k) * np.exp(-np.arange(k) / 100.0)).astype(np.float32), d) for k, d in ((800, 3), (64, 0), (200, 199))]
    plain, ones = run_fir(torch_mod, segs, filters, False)
    scaled, gains = run_fir(torch_mod, segs, filters, True)
    assert (ones == 1.0).all()
    for s, y, o, g in zip(segs, plain, scaled, gains):
        ref = A.fir_gain(s, y)
        assert abs(float(g) - ref) <= 2.0 ** -23 * ref, (float(g), ref)
        assert same_bits(o, np.float32(g) * y)
        assert abs(10 * np.log10(A.sumsq(o) / A.sumsq(s))) < 1e-5
    quiet, _ = run_fir(torch_mod, segs, filters, True, want_gain=False)          # gain_dev may be NULL
    assert all(same_bits(a, b) for a, b in zip(quiet, scaled))


def test_mix_gain_output_and_snr(torch_mod):
    """gain_dev against fp64 within 2^-23 relative; given the device's g, |out - (x + g v)| <= 1.01 * 2^-24 |x + g v| formed in
    fp64 (one fmaf); and the meaning: the measured SNR is within 0.01 dB of the requested one on unit-scale data of 10^4 samples.
    Wrap-around: noises of 7, 64 and len - 1 samples, offsets 0 and noise_len - 1."""
    rng = np.random.default_rng(8)
    n = 10000
    cases = [(m, o, snr) for m in (7, 64, n - 1, 3 * n) for o, snr in ((0, 5.0), (m - 1, 20.0))]
    segs = [rng.standard_normal(n).astype(np.float32) for _ in cases]
    noises = [rng.standard_normal(m).astype(np.float32) for m, _, _ in cases]
    offsets = [o for _, o, _ in cases]
    scales = [10.0 ** (-snr / 20.0) for _, _, snr in cases]
    outs, gains = run_mix(torch_mod, segs, noises, offsets, scales)
    for x, v_all, (m, o, snr), sc, out, g in zip(segs, noises, cases, scales, outs, gains):
        v = A.noise_window(v_all, o, n)
        ref = A.mix_gain(x, v, sc)
        assert abs(float(g) - ref) <= 2.0 ** -23 * ref, (m, o, float(g), ref)
        want = A.mix(x, v, g)
        assert (np.abs(out.astype(np.float64) - want) <= 2.0 ** -24 * 1.01 * np.abs(want)).all(), (m, o)
        got_snr = 10 * np.log10(A.sumsq(x) / A.sumsq(out.astype(np.float64) - x.astype(np.float64)))
        assert abs(got_snr - snr) < 0.01, (m, o, got_snr, snr)


def test_zero_powers(torch_mod):
    rng = np.random.default_rng(9)
    x = rng.standard_normal(500).astype(np.float32)
    x[:3] = [0.0, -0.0, 1e-40]
    zeros = np.zeros(500, np.float32)
    outs, gains = run_mix(torch_mod, [x, zeros, x], [np.zeros(40, np.float32), x[:77].copy(), x[:77].copy()], [5, 5, 5], [1.0, 1.0, 0.0])
    assert gains.tolist() == [0.0, 0.0, 0.0]                                      # Pv = 0, Px = 0, scale = 0
    assert same_bits(outs[0], x) and same_bits(outs[1], zeros) and same_bits(outs[2], x)
    h = np.asarray([0.5, 0.25], np.float32)
    outs, gains = run_fir(torch_mod, [zeros, x], [(h, 0), (np.zeros(4, np.float32), 1)], True)
    assert gains.tolist() == [1.0, 1.0]                                           # Px = 0, Py = 0
    assert (outs[0] == 0.0).all() and (outs[1] == 0.0).all()


# ---- 6. identities ----

def test_delta_filter_identities(torch_mod):
    T, _ = consts()
    rng = np.random.default_rng(10)
    h = np.asarray([0.0, 0.0, 1.0, 0.0], np.float32)
    segs = [rng.standard_normal(n).astype(np.float32) for n in (1, 2, 3, 100, T + 9)]
    outs, gains = run_fir(torch_mod, segs, [(h, 2)] * len(segs), True)
    assert (gains == 1.0).all()
    for s, o in zip(segs, outs):
        assert same_bits(o, s)
    outs, _ = run_fir(torch_mod, segs, [(h, 0)] * len(segs), False)
    for s, o in zip(segs, outs):
        assert same_bits(o, np.concatenate((np.zeros(2, np.float32), s))[:len(s)])


# ---- 7. the Python surface ----

@pytest.fixture(scope="module")
def banks():
    rng = np.random.default_rng(30)
    rirs = []
    for k, lead in ((900, 0), (2500, 40), (300, 7)):
        h = rng.standard_normal(k) * np.exp(-np.arange(k) / (k / 8.0)) * 0.3
        h[lead] = 1.5
        rirs.append(h.astype(np.float32))
    noises = [rng.standard_normal(n).astype(np.float32) for n in (500, 30000, 4001)]
    waves = [rng.standard_normal(n).astype(np.float32) for n in (3000, 4001, 1, 2500, 900, 7777, 9000, 10)]
    return rirs, noises, waves


def one_buffer(torch, out, waves):
    assert [int(t.shape[0]) for t in out] == [len(w) for w in waves]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in out)
    assert len({t.untyped_storage().data_ptr() for t in out}) == 1


def test_reverberate_against_the_reference(torch_mod, banks):
    torch = torch_mod
    from wav2vec2.audio import reverberate, rir_delay, trim_rir
    rirs, _, waves = banks
    out, choices = reverberate(waves, rirs, seed=4)
    assert choices == [int(c) for c in np.random.default_rng(4).integers(0, len(rirs), size=len(waves))]
    one_buffer(torch, out, waves)
    for w, c, o in zip(waves, choices, out):
        h = trim_rir(rirs[c])
        d = rir_delay(h)
        assert d == (0, 40, 7)[c]
        y, mag = A.fir(w, h, d)
        ref = A.fir_gain(w, y) * y
        # the chain's bound, one rounding more for the gain and one for the product with it
        assert (np.abs(o.cpu().numpy() - ref) <= 1.01 * (len(h) + 3) * 2.0 ** -24 * A.fir_gain(w, y) * mag).all()
    again, _ = reverberate([torch.from_numpy(w).cuda() for w in waves], rirs, choices=choices)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    plain, _ = reverberate(waves[:2], rirs, choices=[1, 1], align=False, match_power=False)
    h = trim_rir(rirs[1])
    for w, o in zip(waves, plain):
        y, mag = A.fir(w, h, 0)
        assert (np.abs(o.cpu().numpy() - y) <= 1.01 * (len(h) + 1) * 2.0 ** -24 * mag).all()
    short, _ = reverberate(waves[:1], rirs, choices=[1], max_taps=100)
    y, mag = A.fir(waves[0], trim_rir(rirs[1], max_taps=100), 40)
    assert (np.abs(short[0].cpu().numpy() - A.fir_gain(waves[0], y) * y) <= 1.01 * 103 * 2.0 ** -24 * A.fir_gain(waves[0], y) * mag).all()


def test_add_noise_against_the_reference(torch_mod, banks):
    torch = torch_mod
    from wav2vec2.audio import add_noise
    _, noises, waves = banks
    out, draws = add_noise(waves, noises, seed=5)
    one_buffer(torch, out, waves)
    assert len(draws) == len(waves)
    for w, (c, o, snr), t in zip(waves, draws, out):
        assert 0 <= c < len(noises) and 5.0 <= snr < 20.0
        assert 0 <= o <= max(len(noises[c]) - len(w), 0) or (len(noises[c]) <= len(w) and 0 <= o < len(noises[c]))
        v = A.noise_window(noises[c], o, len(w))
        g = A.mix_gain(w, v, 10.0 ** (-snr / 20.0))
        want = A.mix(w, v, g)
        # one fmaf on the sum, and a gain within 2^-23 of the fp64 one (test_mix_gain_output_and_snr)
        bound = 1.01 * (2.0 ** -24 * np.abs(want) + 2.0 ** -23 * np.abs(g * v.astype(np.float64)))
        assert (np.abs(t.cpu().numpy().astype(np.float64) - want) <= bound).all()
    c, o, s = zip(*draws)
    again, draws2 = add_noise(waves, noises, choices=c, offsets=o, snrs=s)
    assert draws2 == draws and all(torch.equal(a, b) for a, b in zip(out, again))
    fixed, draws3 = add_noise(waves[:3], noises, snr_db=10.0, seed=1)
    assert [d[2] for d in draws3] == [10.0] * 3


def test_augment_is_reproducible(torch_mod, banks):
    torch = torch_mod
    from wav2vec2.audio import Augment, add_noise, reverberate, speed_perturb
    rirs, noises, waves = banks
    lengths = [len(w) for w in waves]
    aug = Augment(rirs=rirs, noises=noises, seed=3)
    plan = aug.plan(lengths)
    assert plan == aug.plan(lengths)
    out, info = aug(waves)
    assert info == plan and info["lengths"] == lengths
    assert any(c is None for c in info["rir"]) and any(c is not None for c in info["rir"])
    assert any(c is None for c in info["noise"]) and any(c is not None for c in info["noise"])
    out_b, info_b = Augment(rirs=rirs, noises=noises, seed=3)(waves)
    assert info_b == info and all(torch.equal(a, b) for a, b in zip(out, out_b))
    out_c, info_c = Augment(rirs=rirs, noises=noises, seed=4)(waves)
    assert info_c != info and not all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(out, out_c))
    next_plan = aug.plan(lengths)
    assert next_plan != plan and aug(waves)[1] == next_plan                       # the generator lives on
    # replaying info through the three functions
    cur, factors = speed_perturb(waves, aug.speed, choices=info["speed_choices"])
    assert factors == info["speed"]
    cur = list(cur)
    mine = [i for i, c in enumerate(info["rir"]) if c is not None]
    for i, t in zip(mine, reverberate([cur[i] for i in mine], rirs, choices=[info["rir"][i] for i in mine])[0]):
        cur[i] = t
    mine = [i for i, c in enumerate(info["noise"]) if c is not None]
    c, o, s = zip(*(info["noise"][i] for i in mine))
    for i, t in zip(mine, add_noise([cur[i] for i in mine], noises, choices=c, offsets=o, snrs=s)[0]):
        cur[i] = t
    assert all(torch.equal(a, b) for a, b in zip(out, cur))
    for o, f, n in zip(out, info["speed"], lengths):
        assert int(o.shape[0]) == {0.9: -(-n * 10 // 9), 1.0: n, 1.1: -(-n * 10 // 11)}[f]


def test_augment_unselected_utterances_keep_their_bits(torch_mod, banks):
    torch = torch_mod
    from wav2vec2.audio import Augment
    rirs, noises, waves = banks
    out, info = Augment(speed=None, rirs=rirs, rir_prob=0.0, noises=noises, noise_prob=0.0, seed=1)(waves)
    assert info["speed"] is None and info["rir"] == [None] * len(waves) and info["noise"] == [None] * len(waves)
    assert all(t.is_cuda and torch.equal(t.cpu(), torch.from_numpy(w)) for t, w in zip(out, waves))
    out, info = Augment(speed=(1.0,), rirs=rirs, rir_prob=0.0, noises=noises, noise_prob=0.0, seed=1)(waves)
    assert all(torch.equal(t.cpu(), torch.from_numpy(w)) for t, w in zip(out, waves))
    out, info = Augment(speed=(1.0,), rirs=rirs, rir_prob=1.0, noises=noises, noise_prob=1.0, seed=1)(waves)
    assert None not in info["rir"] and None not in info["noise"]
    assert not any(torch.equal(t.cpu(), torch.from_numpy(w)) for t, w in zip(out, waves))
    out, info = Augment(speed=(1.0,), seed=1)(waves)                              # no banks: no such stages
    assert info["rir"] == [None] * len(waves) and all(torch.equal(t.cpu(), torch.from_numpy(w)) for t, w in zip(out, waves))


def test_python_argument_errors(torch_mod, banks):
    from wav2vec2.audio import Augment, add_noise, reverberate
    rirs, noises, waves = banks
    two_d = np.zeros((2, 100), np.float32)
    for bad in ([], two_d, [two_d], [np.zeros(0, np.float32)]):
        with pytest.raises(ValueError):
            reverberate(bad, rirs)
        with pytest.raises(ValueError):
            add_noise(bad, noises)
        with pytest.raises(ValueError):
            Augment(rirs=rirs)(bad)
    for bad in ([], [two_d], [np.zeros(50, np.float32)], [np.zeros(0, np.float32)]):
        with pytest.raises(ValueError):
            reverberate(waves, bad)
        with pytest.raises(ValueError):
            Augment(rirs=bad)
    for bad in ([], [two_d], [np.zeros(0, np.float32)]):
        with pytest.raises(ValueError):
            add_noise(waves, bad)
        with pytest.raises(ValueError):
            Augment(noises=bad)
    for bad in ([0] * 7, [0] * 7 + [3], [0] * 7 + [-1]):
        with pytest.raises(ValueError):
            reverberate(waves, rirs, choices=bad)
        with pytest.raises(ValueError):
            add_noise(waves, noises, choices=bad)
    with pytest.raises(ValueError):
        add_noise(waves[:1], noises, choices=[0], offsets=[500])
    for bad in (float("nan"), float("inf"), (5.0, float("inf")), (20.0, 5.0)):
        with pytest.raises(ValueError):
            add_noise(waves, noises, snr_db=bad)
        with pytest.raises(ValueError):
            Augment(noises=noises, snr_db=bad)
    with pytest.raises(ValueError):
        add_noise(waves[:1], noises, snrs=[float("nan")])
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Augment(rir_prob=p)
        with pytest.raises(ValueError):
            Augment(noise_prob=p)


# ---- 8. the C ABI's argument errors ----

def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    x = torch.zeros(64, device="cuda")
    y = torch.zeros(64, device="cuda")
    h = torch.ones(8, device="cuda")
    one = np.zeros(1, np.int64)
    neg = np.full(1, -1, np.int64)

    def fir(inp=N.ptr(x), n=1, in0=one, length=(30,), taps=N.ptr(h), taps0=one, ntaps=(4,), delay=(1,), out=N.ptr(y), out0=one):
        ln = None if length is None else np.asarray(length, np.int64)
        nt = None if ntaps is None else np.asarray(ntaps, np.int32)
        dl = None if delay is None else np.asarray(delay, np.int32)
        return lib.w2v2_fir(inp, n, N.ptr(in0), N.ptr(ln), taps, N.ptr(taps0), N.ptr(nt), N.ptr(dl), out, N.ptr(out0), 1, None,
                            N.current_stream())

    assert fir() == 0
    torch.cuda.synchronize()
    for kw, msg in [(dict(inp=None), "null"), (dict(in0=None), "null"), (dict(length=None), "null"), (dict(taps=None), "null"),
                    (dict(taps0=None), "null"), (dict(ntaps=None), "null"), (dict(delay=None), "null"), (dict(out=None), "null"),
                    (dict(out0=None), "null"), (dict(n=0), "n = 0"), (dict(length=(0,)), "len_host"), (dict(length=(1 << 31,)), "len_host"),
                    (dict(ntaps=(0,)), "ntaps"), (dict(ntaps=(65537,)), "ntaps"), (dict(delay=(-1,)), "delay"), (dict(delay=(4,)), "delay"),
                    (dict(in0=neg), "in0"), (dict(taps0=neg), "taps0"), (dict(out0=neg), "out0")]:
        assert fir(**kw) == -1, kw
        assert msg in N.last_error(), (kw, N.last_error())

    def mix(inp=N.ptr(x), n=1, in0=one, length=(30,), noise=N.ptr(h), noise0=one, noise_len=(8,), offset=(7,), scale=(0.5,), out=N.ptr(y),
            out0=one):
        arr = lambda v, t: None if v is None else np.asarray(v, t)
        ln, nl, of, sc = arr(length, np.int64), arr(noise_len, np.int64), arr(offset, np.int64), arr(scale, np.float64)
        return lib.w2v2_mix(inp, n, N.ptr(in0), N.ptr(ln), noise, N.ptr(noise0), N.ptr(nl), N.ptr(of), N.ptr(sc), out, N.ptr(out0), None,
                            N.current_stream())

    assert mix() == 0
    torch.cuda.synchronize()
    for kw, msg in [(dict(inp=None), "null"), (dict(in0=None), "null"), (dict(length=None), "null"), (dict(noise=None), "null"),
                    (dict(noise0=None), "null"), (dict(noise_len=None), "null"), (dict(offset=None), "null"), (dict(scale=None), "null"),
                    (dict(out=None), "null"), (dict(out0=None), "null"), (dict(n=0), "n = 0"), (dict(length=(0,)), "len_host"),
                    (dict(length=(1 << 31,)), "len_host"), (dict(noise_len=(0,)), "noise_len"), (dict(offset=(-1,)), "offset"),
                    (dict(offset=(8,)), "offset"), (dict(scale=(float("nan"),)), "scale"), (dict(scale=(-1.0,)), "scale"),
                    (dict(in0=neg), "in0"), (dict(noise0=neg), "noise0"), (dict(out0=neg), "out0")]:
        assert mix(**kw) == -1, kw
        assert msg in N.last_error(), (kw, N.last_error())
