"""The resampler on the GPU (w2v2_resample, csrc/resample.hip) against tests/resample_reference.py: the index
arithmetic bit for bit on integer data, the designed filters against fp64 within the bound of a length-K fp32 dot product,
isolation and position independence bitwise, several filters in one call, the Python surface (wav2vec2.audio), the model's
`sampling_rate=` / `normalize=` arguments, and the C ABI's argument errors."""

import numpy as np
import pytest

import helpers as H
import resample_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
RATES = [48000, 44100, 22050, 14400, 17600, 8000]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def tile():
    from wav2vec2 import _native as N
    assert N.RESAMPLE_TILE == 2048
    return N.RESAMPLE_TILE


def len_for(out_len, L, M):
    """The shortest input whose output has at least `out_len` samples (exactly that many when L <= M)."""
    n = (out_len - 1) * M // L + 1
    assert out_len <= R.out_length(n, L, M) <= out_len + -(-L // M)
    return n


def run(torch, segs, filters, filter_of=None, in_off=(0, 1, 3), out_off=(3, 0, 1), shift=0, order=None):
    """One w2v2_resample call.  segs: 1-D float32 arrays; filters: (table (L, K) float32, M, lead).  Segment i starts
    in_off[i % 3] floats behind a 64-float boundary of the input buffer (moved by `shift`) and its output out_off[i % 3] floats
    behind one of the output buffer; `order` lays the segments out in another order.  The input between the segments is NaN, the
    output is pre-filled with a sentinel that must survive everywhere outside the segments' ranges.  Returns the outputs."""
    from wav2vec2 import _native as N
    lib = N.load()
    n = len(segs)
    which = [0] * n if filter_of is None else list(filter_of)
    out_len = [R.out_length(len(s), filters[k][0].shape[0], filters[k][1]) for s, k in zip(segs, which)]
    in0, out0 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ci, co = 64 + shift, 64
    for i in (range(n) if order is None else order):
        in0[i] = -(-ci // 64) * 64 + shift + in_off[i % 3]
        out0[i] = -(-co // 64) * 64 + out_off[i % 3]
        ci, co = in0[i] + len(segs[i]), out0[i] + out_len[i]
    host = np.full(ci + 64, np.nan, np.float32)
    for s, a in zip(segs, in0):
        host[a:a + len(s)] = s
    x = torch.from_numpy(host).cuda()
    y = torch.full((int(co) + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    tables = [torch.from_numpy(np.ascontiguousarray(f[0], np.float32)).cuda() for f in filters]
    fs = (N.W2V2ResampleFilter * len(filters))()
    for f, t, (tab, M, lead) in zip(fs, tables, filters):
        f.table, f.L, f.M, f.K, f.lead = t.data_ptr(), tab.shape[0], M, tab.shape[1], lead
    in_len = np.asarray([len(s) for s in segs], np.int64)
    fo = None if filter_of is None else np.asarray(which, np.int32)
    N.check(lib.w2v2_resample(N.ptr(x), n, N.ptr(in0), N.ptr(in_len), N.ptr(fo), fs, len(filters), N.ptr(y), N.ptr(out0),
                              N.current_stream()), "w2v2_resample")
    got = y.cpu().numpy()
    rest = np.ones(len(got), bool)
    outs = []
    for a, m in zip(out0, out_len):
        outs.append(got[a:a + m].copy())
        rest[a:a + m] = False
    assert (got[rest] == SENTINEL).all(), "a float outside the segments' output ranges was written"
    return outs


# ---- 1. index arithmetic, bit for bit ----

@pytest.mark.parametrize("K", [1, 2, 68, 204, 512])
@pytest.mark.parametrize("L,M", [(1, 3), (160, 441), (2, 1), (320, 441), (10, 9), (10, 11), (1, 1), (3, 1), (7, 32)])
def test_integer_tables_are_exact(torch_mod, L, M, K):
    """Integer taps in [-7, 7] on integer samples in [-15, 15]: every partial sum stays below 2^24 (512 * 105), so fp32 is exact in
    any order and the result must EQUAL the integer reference.  A dropped or shifted edge tap shows here; under the designed
    filters, whose edge taps are 1e-6 of the centre, it would hide inside the rounding bound.  The edge taps are +-7."""
    T = tile()
    rng = np.random.default_rng(1000 * L + 10 * M + K)
    for lead in sorted({0, max(K // 2 - 1, 0), K - 1}):
        table = rng.integers(-7, 8, size=(L, K)).astype(np.float32)
        table[:, 0] = np.where(rng.integers(0, 2, L) > 0, 7.0, -7.0)
        table[:, -1] = np.where(rng.integers(0, 2, L) > 0, 7.0, -7.0)
        lens = [1, 2, max(lead, 1), K, K + 1] + [len_for(x, L, M) for x in (T - 1, T, T + 1, 2 * T + 1)] + [5 * T * M // L + 3]
        segs = [rng.integers(-15, 16, size=n).astype(np.float32) for n in lens]
        outs = run(torch_mod, segs, [(table, M, lead)])
        for n, s, o in zip(lens, segs, outs):
            ref, _ = R.apply(s, L, M, K, lead, table)
            assert o.shape == ref.shape
            bad = np.flatnonzero(o != ref)
            assert bad.size == 0, f"L {L} M {M} K {K} lead {lead}, {n} samples: {bad.size} outputs differ, first at {bad[:5]}"


@pytest.mark.parametrize("L,M,K,lead,path", [(1, 9, 512, 255, "fewer outputs per block"), (4, 101, 68, 33, "fewer outputs per block"),
                                             (1, 300, 68, 33, "direct"), (3, 2, 16000, 7999, "direct")])
def test_integer_tables_where_the_span_exceeds_the_lds(torch_mod, L, M, K, lead, path):
    """The same exact check on the kernel's two other paths: a ratio or a K whose input span per 2048 outputs is beyond the LDS
    gets fewer outputs per block, and one that cannot stage even 64 outputs reads its samples from global memory.  K = 16000 still
    keeps every partial sum below 2^24 (16000 * 105)."""
    T = tile()
    rng = np.random.default_rng(K + M)
    table = rng.integers(-7, 8, size=(L, K)).astype(np.float32)
    table[:, 0], table[:, -1] = 7.0, -7.0
    lens = [1, 2, K + 1, len_for(T + 1, L, M), len_for(2 * T + 65, L, M)]
    segs = [rng.integers(-15, 16, size=n).astype(np.float32) for n in lens]
    outs = run(torch_mod, segs, [(table, M, lead)])
    for n, s, o in zip(lens, segs, outs):
        ref, _ = R.apply(s, L, M, K, lead, table)
        assert o.shape == ref.shape
        bad = np.flatnonzero(o != ref)
        assert bad.size == 0, f"{path}: L {L} M {M} K {K}, {n} samples: {bad.size} outputs differ, first at {bad[:5]}"


# ---- 2. the designed filters against fp64 ----

def mixed_scales(rng, n):
    return (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 100.0], size=n)).astype(np.float32)


@pytest.mark.parametrize("rate", RATES)
def test_designed_filters_within_the_dot_product_bound(torch_mod, rate):
    """|got - ref| <= 1.01 (K + 1) 2^-24 sum_t |table| |x|, the bound of a length-K fp32 dot product in any order (K roundings of
    the running sum of at most 2^-24 relative each, one more for the margin of the fp64 reference itself)."""
    from wav2vec2.audio import Resampler
    r = Resampler(rate)
    L, M, K, lead, table64 = R.design(rate)
    assert (r.L, r.M, r.taps, r.lead) == (L, M, K, lead)
    rng = np.random.default_rng(rate)
    lens = [1, 333, K + 1, len_for(tile() + 1, L, M), 3 * tile() * M // L + 17]
    segs = [mixed_scales(rng, n) for n in lens]
    outs = r(segs)
    worst = 0.0
    for s, o in zip(segs, outs):
        ref, mag = R.apply(s, L, M, K, lead, r.table)
        got = o.cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape
        bound = 1.01 * (K + 1) * 2.0 ** -24 * mag
        worst = max(worst, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
        assert (np.abs(got - ref) <= bound).all()
    print(f"{rate} -> 16000 ({L} / {M}, {K} taps): largest error is {100 * worst:.1f} % of the bound")


# ---- 3. isolation and position independence ----

@pytest.mark.parametrize("rate_in,rate_out", [(44100, 16000), (9, 10)])
def test_segments_are_computed_as_if_alone(torch_mod, rate_in, rate_out):
    from wav2vec2.audio import Resampler
    r = Resampler(rate_in, rate_out)
    filt = [(r.table, r.M, r.lead)]
    rng = np.random.default_rng(5)
    lens = [700, 1, 4 * tile() * r.M // r.L + 3, 33, 2500]
    segs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    together = run(torch_mod, segs, filt)
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    for i, s in enumerate(segs):
        assert same(run(torch_mod, [s], filt)[0], together[i]), f"segment {i} alone"
    perm = [3, 0, 4, 2, 1]
    permuted = run(torch_mod, [segs[p] for p in perm], filt)
    for k, p in enumerate(perm):
        assert same(permuted[k], together[p]), f"segment {p} at place {k}"
    laid = run(torch_mod, segs, filt, order=perm[::-1], in_off=(3, 3, 0), out_off=(1, 0, 0))
    for i in range(len(segs)):
        assert same(laid[i], together[i]), f"segment {i} elsewhere in the buffers"
    poisoned = list(segs)
    poisoned[1] = np.full(1, np.nan, np.float32)
    poisoned[3] = np.full(33, np.nan, np.float32)
    got = run(torch_mod, poisoned, filt)
    for i in (0, 2, 4):
        assert same(got[i], together[i]), f"segment {i} beside NaN neighbours"
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    shifted = run(torch_mod, segs, filt, shift=1)
    for i in range(len(segs)):
        assert same(shifted[i], together[i]), f"segment {i} with the input one float further"


# ---- 4. several filters in one call ----

def test_three_filters_in_one_call(torch_mod):
    from wav2vec2.audio import Resampler
    rs = [Resampler(9, 10), Resampler(7, 7), Resampler(11, 10)]
    assert [(r.L, r.M) for r in rs] == [(10, 9), (1, 1), (10, 11)]
    filters = [(r.table, r.M, r.lead) for r in rs]
    rng = np.random.default_rng(8)
    lens = [3000, 1, 2 * tile() + 77, 5000, 640, 2, 4100]
    which = [0, 1, 2, 1, 2, 0, 0]
    segs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    segs[3][:4] = [0.0, -0.0, 1e-40, -1e-40]              # the copy keeps signed zeros and subnormals
    mixed = run(torch_mod, segs, filters, filter_of=which)
    for k in range(3):
        mine = [i for i, w in enumerate(which) if w == k]
        alone = run(torch_mod, [segs[i] for i in mine], [filters[k]])
        for i, o in zip(mine, alone):
            assert np.array_equal(o.view(np.int32), mixed[i].view(np.int32)), f"segment {i} with filter {k}"
    for i in (1, 3):
        assert np.array_equal(mixed[i].view(np.int32), segs[i].view(np.int32))


# ---- 5. the Python surface ----

def test_resampler_inputs_and_views(torch_mod):
    torch = torch_mod
    from wav2vec2.audio import Resampler, resample, resampled_length
    rng = np.random.default_rng(11)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (4410, 1, 30000)]
    r = Resampler(44100)
    a = r(waves)
    assert isinstance(a, list) and [int(t.shape[0]) for t in a] == [resampled_length(len(w), 44100) for w in waves] == [1600, 1, 10885]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in a)
    assert len({t.untyped_storage().data_ptr() for t in a}) == 1
    b = r([torch.from_numpy(w) for w in waves])
    c = r([torch.from_numpy(w).cuda() for w in waves])
    d = resample(waves, 44100)
    e = resample([w.astype(np.float64) for w in waves], 44100, 16000)
    for others in (b, c, d, e):
        for t, u in zip(a, others):
            assert torch.equal(t, u)
    for i, w in enumerate(waves):
        one = r(w)
        assert isinstance(one, torch.Tensor) and torch.equal(one, a[i])
        assert torch.equal(resample(torch.from_numpy(w).cuda(), 44100), a[i])
    assert torch.equal(resample(waves[2], 16000), torch.from_numpy(waves[2]).cuda())
    for bad in ([], np.zeros((2, 100), np.float32), [np.zeros((2, 100), np.float32)], [np.zeros(0, np.float32)], "abc"):
        with pytest.raises(ValueError):
            r(bad)
    for rate in (0, -1, 1.5):
        with pytest.raises(ValueError):
            resample(waves, rate)


def test_speed_perturb(torch_mod):
    torch = torch_mod
    from wav2vec2.audio import Resampler, speed_perturb
    rng = np.random.default_rng(12)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (3000, 4001, 1, 2500, 900, 7777, 16000, 10)]
    factors = (0.9, 1.0, 1.1)
    out, chosen = speed_perturb(waves, seed=3)
    draws = np.random.default_rng(3).integers(0, 3, size=len(waves))
    assert chosen == [factors[d] for d in draws]
    again, chosen2 = speed_perturb(waves, seed=3)
    assert chosen2 == chosen and all(torch.equal(a, b) for a, b in zip(out, again))
    ratio = {0.9: (10, 9), 1.0: (1, 1), 1.1: (10, 11)}
    assert len({t.untyped_storage().data_ptr() for t in out}) == 1
    for w, o, f in zip(waves, out, chosen):
        L, M = ratio[f]
        assert int(o.shape[0]) == -(-len(w) * L // M) == int(np.ceil(len(w) / f - 1e-9))
        expect = torch.from_numpy(w).cuda() if f == 1.0 else Resampler(M, L)(w)
        assert torch.equal(o, expect)
    picks = [2, 2, 0, 1, 1, 0, 2, 1]
    out, chosen = speed_perturb(waves, choices=picks)
    assert chosen == [factors[p] for p in picks]
    assert [int(o.shape[0]) for o in out] == [-(-len(w) * ratio[f][0] // ratio[f][1]) for w, f in zip(waves, chosen)]
    out, chosen = speed_perturb(waves[:2], factors=(1.0,), seed=0)
    assert chosen == [1.0, 1.0] and all(torch.equal(o, torch.from_numpy(w).cuda()) for o, w in zip(out, waves))
    with pytest.raises(ValueError):
        speed_perturb(waves, factors=(1.0, 0.0))
    with pytest.raises(ValueError):
        speed_perturb([])


# ---- 6. the model's entry points ----

WINDOW, MARGIN = 6400, 640
WINDOW_S, MARGIN_S = WINDOW / 16000.0, MARGIN / 16000.0


@pytest.fixture(scope="module")
def model(torch_mod):
    import wav2vec2
    m = wav2vec2.Wav2Vec2ForCTC(H.case_config("tiny_base"), input_shape=(1, 2048))
    m.set_weights(H.case_weights("tiny_base"))
    return m


def test_predict_packed_sampling_rate_and_normalize(torch_mod, model):
    torch = torch_mod
    from wav2vec2.audio import resample
    from wav2vec2.longform import normalize_windows
    rng = np.random.default_rng(20)
    waves48 = [(3.0 * rng.standard_normal(n) + 0.5).astype(np.float32) for n in (9000, 24001, 4803)]
    at16 = resample(waves48, 48000)
    assert [int(t.shape[0]) for t in at16] == [3000, 8001, 1601]
    ref = model.predict_packed(at16)
    got = model.predict_packed(waves48, sampling_rate=48000)
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, ref))
    # None and 16000 are today's call
    waves16 = [rng.standard_normal(n).astype(np.float32) for n in (3000, 5001)]
    today = model.predict_packed(waves16)
    for kw in (dict(sampling_rate=None), dict(sampling_rate=16000), dict(sampling_rate=16000, normalize=False)):
        assert all(torch.equal(a, b) for a, b in zip(model.predict_packed(waves16, **kw), today))
    # normalize=True: each utterance over its own resampled samples, by w2v2_op_normalize_windows
    lens = np.asarray([int(t.shape[0]) for t in at16], np.int64)
    flat = normalize_windows(torch.cat(at16), np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
    ref = model.predict_packed(list(torch.split(flat, lens.tolist())))
    got = model.predict_packed(waves48, sampling_rate=48000, normalize=True)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert not torch.equal(got[0], model.predict_packed(waves48, sampling_rate=48000)[0])
    with pytest.raises(ValueError):
        model.predict_packed(waves48, sampling_rate=0)
    with pytest.raises(ValueError):
        model.predict_packed([waves48[0][:900]], sampling_rate=48000)      # 300 samples at 16 kHz: below the receptive field


def test_predict_long_sampling_rate(torch_mod, model):
    torch = torch_mod
    from wav2vec2.audio import resample
    rng = np.random.default_rng(21)
    rec = rng.standard_normal(60000).astype(np.float32)
    ref = model.predict_long(resample(rec, 44100), WINDOW_S, MARGIN_S)
    got = model.predict_long(rec, WINDOW_S, MARGIN_S, sampling_rate=44100)
    assert got.shape[0] == model.num_frames(-(-60000 * 160 // 441)) and torch.equal(got, ref)
    both = model.predict_long([rec, rec[:30000]], WINDOW_S, MARGIN_S, sampling_rate=44100)
    assert torch.equal(both[0], ref)
    rec16 = rng.standard_normal(20000).astype(np.float32)
    today = model.predict_long(rec16, WINDOW_S, MARGIN_S)
    for rate in (None, 16000):
        assert torch.equal(model.predict_long(rec16, WINDOW_S, MARGIN_S, sampling_rate=rate), today)


def test_times_are_preserved_from_48_khz(torch_mod, model):
    """The same sound at 16 kHz and at 48 kHz gives the same number of frames and pauses at the same frames.

    The 16 kHz recording is noise bursts between silences, band-limited below 4 kHz (made at 8 kHz and brought to 16 kHz by the
    fp64 reference, so that the way to 48 kHz and back loses nothing but the filters' -120 dB); the 48 kHz recording is the fp64
    reference's upsampling of it.  A frame is `quiet` where one label leads (margin 0): the tiny random model knows no blank,
    and any label that pauses serves the comparison.  The pause cuts agree within one frame."""
    from wav2vec2.longform import pause_cuts
    rng = np.random.default_rng(22)
    base = np.zeros(20000)
    for a, b in [(1500, 4000), (6500, 7600), (9000, 13000), (15500, 18000)]:
        base[a:b] = rng.standard_normal(b - a)
    L, M, K, lead, table = R.design(8000, 16000)
    rec16 = R.apply(base, L, M, K, lead, table)[0].astype(np.float32)
    L, M, K, lead, table = R.design(16000, 48000)
    rec48 = R.apply(rec16, L, M, K, lead, table)[0].astype(np.float32)
    assert len(rec16) == 40000 and len(rec48) == 120000
    lo = model.predict_long(rec16, WINDOW_S, MARGIN_S)
    hi = model.predict_long(rec48, WINDOW_S, MARGIN_S, sampling_rate=48000)
    assert lo.shape == hi.shape and lo.shape[0] == model.num_frames(40000)
    print(f"max |logits(48 kHz) - logits(16 kHz)| = {float((lo - hi).abs().max()):.3e}")
    # the label that stands in for the blank is chosen on the 16 kHz logits alone: the most frequent argmax that pauses at all
    counts = np.bincount(lo.argmax(dim=1).cpu().numpy(), minlength=lo.shape[1])
    for blank in np.argsort(-counts, kind="stable"):
        a = pause_cuts([lo], blank=int(blank), margin=0.0, min_pause=3)[0]
        if a.count:
            break
    assert a.count >= 1, "no label of the 16 kHz logits leads for three frames in a row"
    b = pause_cuts([hi], blank=int(blank), margin=0.0, min_pause=3)[0]
    print(f"label {blank}: cuts at 16 kHz {a.cuts.tolist()}, at 48 kHz {b.cuts.tolist()}")
    assert a.count == b.count and np.abs(a.cuts - b.cuts).max() <= 1


# ---- 7. the C ABI's argument errors ----

def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    x = torch.zeros(64, device="cuda")
    y = torch.zeros(256, device="cuda")
    tab = torch.ones(8, device="cuda")
    one = np.zeros(1, np.int64)

    def call(inp=N.ptr(x), n=1, in0=one, in_len=(30,), filter_of=None, table=tab.data_ptr(), L=2, M=3, K=4, lead=1, n_filters=1,
             filters=True, out=N.ptr(y), out0=one):
        fs = (N.W2V2ResampleFilter * 1)()
        fs[0].table, fs[0].L, fs[0].M, fs[0].K, fs[0].lead = table, L, M, K, lead
        il = None if in_len is None else np.asarray(in_len, np.int64)
        fo = None if filter_of is None else np.asarray(filter_of, np.int32)
        return lib.w2v2_resample(inp, n, N.ptr(in0), N.ptr(il), N.ptr(fo), fs if filters else None, n_filters, out, N.ptr(out0),
                                 N.current_stream())

    assert call() == 0
    torch.cuda.synchronize()
    neg = np.full(1, -1, np.int64)
    for kw, msg in [(dict(inp=None), "null"), (dict(out=None), "null"), (dict(in0=None), "null"), (dict(in_len=None), "null"),
                    (dict(out0=None), "null"), (dict(filters=False), "null"), (dict(table=None), "table_dev"),
                    (dict(n=0), "n = 0"), (dict(n_filters=0), "n_filters"), (dict(in_len=(0,)), "in_len"),
                    (dict(in_len=(1 << 31,)), "in_len"), (dict(in0=neg), "in0"), (dict(out0=neg), "out0"),
                    (dict(filter_of=(1,)), "filter_of"), (dict(filter_of=(-1,)), "filter_of"), (dict(L=0), ".L"), (dict(M=0), ".M"),
                    (dict(K=0), ".K"), (dict(lead=-1), "lead"), (dict(lead=4), "lead"), (dict(L=4097, K=1, lead=0), ".L"),
                    (dict(L=4096, K=1025), "table entries")]:
        assert call(**kw) == -1, kw
        assert msg in N.last_error(), (kw, N.last_error())
    assert call(filter_of=(0,)) == 0
    torch.cuda.synchronize()
