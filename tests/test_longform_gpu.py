"""Long recordings on the GPU: the windowed forward (w2v2_forward_windows / predict_long) against alone runs,
bit for bit; the per-window normalisation against the fp64 formula; the pause cuts (w2v2_ctc_pause_cuts) against the numpy
reference, exactly; decode_long / transcribe_long against the pieces they are made of.

Two cases of the plan cannot be built from window = 6400, margin = 640 samples and use the nearest legal parameters instead:
a last window that owns no frame exists only for a margin of one frame (tests/test_longform_cpu.py), so that length runs
with margin = 320; and a window of 312 frames is 100 160 samples, 100 000 being no multiple of the 320-sample hop."""

import os

import numpy as np
import pytest

import helpers as H
import longform_reference as R

pytestmark = pytest.mark.gpu

WINDOW, MARGIN = 6400, 640
WINDOW_S, MARGIN_S = WINDOW / 16000.0, MARGIN / 16000.0


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def models(torch_mod):
    import wav2vec2
    out = {}
    for name in ("tiny_base", "tiny_robust"):
        cfg = H.case_config(name)
        m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
        m.set_weights(H.case_weights(name))
        out[name] = m
    return out


def noise(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def alone(m, w):
    return m(np.asarray(w, np.float32)[None]).numpy()[0]


def long_rows(m, wave, window=WINDOW, margin=MARGIN, **kw):
    from wav2vec2.longform import predict_long
    return predict_long(m, wave, normalize=kw.pop("normalize", False), window=window, margin=margin, **kw)


def alone_packed(m, w):
    return m.predict_packed([np.asarray(w, np.float32)])[0].numpy()


def check_windows_alone(m, wave, window, margin, run=alone, equal=True):
    """predict_long's rows against `run` on each window of the plan; returns (plan, rows, largest difference)."""
    from wav2vec2.longform import window_plan
    out = long_rows(m, wave, window, margin).numpy()
    plan = window_plan(len(wave), window, margin, m.config)
    assert out.shape[0] == m.num_frames(len(wave)) == plan[-1].out0 + plan[-1].keepn
    worst, unequal = 0.0, 0
    for w in plan:
        ref = run(m, wave[w.sample0:w.sample0 + w.samples])[w.keep0:w.keep0 + w.keepn]
        got = out[w.out0:w.out0 + w.keepn]
        unequal += not np.array_equal(got, ref)
        worst = max(worst, H.max_err(got, ref))
    print(f"{len(wave)} samples, window {window}: {len(plan)} windows, {unequal} differ from {run.__name__}, max diff {worst:.3e}")
    if equal:
        assert unequal == 0, f"{unequal} of {len(plan)} windows differ from {run.__name__}, max diff {worst:.3e}"
    return plan, out, worst


# ---- windows equal alone runs, bit for bit ----

LENGTHS = [6400, 6401, 6400 + 5120 + 400, 6400 + 5120 + 719, 40000]
WINDOWS = {6400: 1, 6401: 2, 11920: 3, 12239: 3, 40000: 8}
CASES = [("tiny_base", WINDOW, MARGIN), ("tiny_robust", WINDOW, MARGIN), ("tiny_base", 100160, 6400)]


def windows_case(models, name, window, margin, run):
    from wav2vec2.longform import seconds_to_samples
    m = models[name]
    if window != WINDOW:
        assert m.num_frames(window) == 312      # more than the 128-frame pos-conv tile and the 256-query attention tile
        plan, _, worst = check_windows_alone(m, noise(3, 250000), window, margin, run, equal=False)
        assert len(plan) == 3
        return worst
    assert seconds_to_samples(WINDOW_S, MARGIN_S, m.config) == (WINDOW, MARGIN)
    worst = 0.0
    for i, L in enumerate(LENGTHS):
        wave = noise(100 + i, L)
        plan, out, err = check_windows_alone(m, wave, WINDOW, MARGIN, run, equal=False)
        assert len(plan) == WINDOWS[L]
        if L <= WINDOW:
            worst = max(worst, H.max_err(out, run(m, wave)))
        # the public method, in seconds, is the same call
        assert np.array_equal(m.predict_long(wave, WINDOW_S, MARGIN_S, normalize=False).numpy(), out)
        worst = max(worst, err)
    # the last window, [5760, 6460), owns no frame and is dropped
    plan, _, err = check_windows_alone(m, noise(7, 5760 + 700), WINDOW, 320, run, equal=False)
    assert len(plan) == 1 and plan[0].samples == WINDOW
    return max(worst, err)


@pytest.mark.parametrize("name,window,margin", CASES)
def test_windows_equal_alone_runs_bitwise(models, name, window, margin):
    """Every kept row of predict_long against the same row of `model(window_k[None])`, bit for bit.

    The packed stream takes conv0's GroupNorm statistics as fp64 partial sums per 64-row chunk, the dense B = 1 forward in Gram
    form over 2048-row blocks, so predict_packed agrees with the alone run to the fp32 bar only.  The windowed
    forward takes them in the dense form, per window, and carries the alone run's bits for both extractors."""
    worst = windows_case(models, name, window, margin, alone)
    assert worst == 0.0, f"max |windows - model(window[None])| = {worst:.3e}"


@pytest.mark.parametrize("name,window,margin", CASES)
def test_windows_match_alone_packed_runs(models, name, window, margin):
    """The same rows against each window alone through the packed forward, `predict_packed([window_k])`: the fp32 bar, as
    tests/test_packed_gpu.py holds the packed forward to against the alone run (identical bits for the layer-norm extractor)."""
    worst = windows_case(models, name, window, margin, alone_packed)
    assert worst < H.ATOL_AIM
    assert worst == 0.0 or name == "tiny_base"


def test_a_list_of_recordings_gives_each_its_own_result(models):
    m = models["tiny_base"]
    waves = [noise(20, 6400 + 700), noise(21, 20000), noise(22, 500)]
    each = [long_rows(m, w).numpy() for w in waves]
    outs = long_rows(m, waves)
    assert isinstance(outs, list) and len(outs) == 3
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1
    for o, e in zip(outs, each):
        assert np.array_equal(o.numpy(), e)


def test_max_stream_changes_no_bit(models):
    from wav2vec2.longform import group_windows, window_plan
    m = models["tiny_base"]
    wave = noise(30, 40000)
    plan = window_plan(len(wave), WINDOW, MARGIN, m.config)
    max_stream_s = 3 * WINDOW / 16000.0
    assert len(group_windows(plan, int(max_stream_s * 16000), m.config)) >= 3
    assert len(group_windows(plan, int(1200.0 * 16000), m.config)) == 1
    assert np.array_equal(long_rows(m, wave, max_stream_s=max_stream_s).numpy(), long_rows(m, wave).numpy())


# ---- normalisation ----

def ordered(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def normalize_ref(x):
    mean = x.mean(dtype=np.float64)
    var = x.var(dtype=np.float64)
    return ((x.astype(np.float64) - mean) / np.sqrt(var + 1e-5)).astype(np.float32)


def test_normalize_windows_kernel(torch_mod):
    from wav2vec2.longform import normalize_windows
    rng = np.random.default_rng(5)
    wave = rng.standard_normal(220000).astype(np.float32)
    wave[150000:151000] = np.float32(0.37)                                                  # a constant window
    wave[160000:165000] = (1e3 + rng.standard_normal(5000)).astype(np.float32)              # a large DC offset
    windows = [(10, 1), (20, 63), (100, 64), (200, 65), (300, 400), (1000, 4097), (5000, 100003),
               (110000, 3000), (111000, 3000), (150000, 1000), (160000, 5000)]
    s0 = np.array([w[0] for w in windows], np.int64)
    n = np.array([w[1] for w in windows], np.int64)
    got = normalize_windows(torch_mod.from_numpy(wave).cuda(), s0, n).cpu().numpy()
    ref = np.concatenate([normalize_ref(wave[a:a + k]) for a, k in windows])
    assert got.shape == ref.shape and np.isfinite(got).all()
    # fp64 accumulation error sits orders below half an fp32 ulp: a value differs only where the fp64 quotient lies on a
    # rounding boundary, and then by one ulp
    ulp = np.abs(ordered(got) - ordered(ref))
    print(f"normalize_windows: {int((ulp > 0).sum())} of {ulp.size} elements differ, max {int(ulp.max())} ulp")
    assert ulp.max() <= 1
    assert (got == ref).mean() >= 0.999
    off = int(n[:9].sum())
    assert not got[off:off + 1000].any() and got[0] == 0.0            # var = 0: only the eps remains, and x - mean = 0


def test_normalized_windows_match_the_processor(models):
    from wav2vec2 import Wav2Vec2Processor
    from wav2vec2.longform import window_plan
    m = models["tiny_base"]
    proc = Wav2Vec2Processor(is_tokenizer=False)
    wave = (3.0 * noise(40, 20000) + 0.5).astype(np.float32)
    out = long_rows(m, wave, normalize=True).numpy()
    assert np.array_equal(m.predict_long(wave, WINDOW_S, MARGIN_S).numpy(), out)          # normalize=True is the default
    for w in window_plan(len(wave), WINDOW, MARGIN, m.config):
        ref = alone(m, proc(wave[w.sample0:w.sample0 + w.samples]))[w.keep0:w.keep0 + w.keepn]
        err = H.max_err(out[w.out0:w.out0 + w.keepn], ref)
        print(f"window at {w.sample0}: max|windows - processor + alone| = {err:.3e}")
        assert err < H.ATOL_AIM


# ---- precision modes ----

@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_split_modes_match_alone(models, mode):
    m = models["tiny_base"]
    m.set_precision(mode)
    try:
        _, _, worst = check_windows_alone(m, noise(50, 20000), WINDOW, MARGIN, alone, equal=False)
        print(f"{mode}: max|windows - alone| = {worst:.3e}")
        assert worst < H.ATOL_AIM
        assert not m.range_overflow()
    finally:
        m.set_precision("fp32")


def test_bf16_is_refused_by_name(models):
    m = models["tiny_base"]
    m.set_precision("bf16")
    try:
        with pytest.raises(RuntimeError, match="bf16"):
            long_rows(m, noise(51, 8000))
    finally:
        m.set_precision("fp32")


# ---- argument checks of the C entry ----

def test_forward_windows_argument_checks(models, torch_mod):
    from wav2vec2 import _native as N
    m = models["tiny_base"]
    m._finalize()
    lib = N.load()
    wave = torch_mod.from_numpy(noise(60, 20000)).cuda()
    out = torch_mod.empty((200, m.config.vocab_size), device="cuda")

    def call(sample0, samples, keep0, keepn, normalize=0, total=20000):
        a = [np.asarray(v, t) for v, t in ((sample0, np.int64), (samples, np.int64), (keep0, np.int32), (keepn, np.int32))]
        rc = lib.w2v2_forward_windows(m._handle, N.ptr(wave), total, len(sample0), *[N.ptr(v) for v in a], normalize, N.ptr(out),
                                      N.current_stream())
        return rc, N.last_error()

    assert call([0, 6000], [6400, 6400], [0, 2], [10, 10])[0] == 0
    nf = m.num_frames(6400)
    for args, word in [
        (([0, 14000], [6400, 6400], [0, 0], [5, 5]), "window 1"),            # runs past the recording's end
        (([0, -1], [6400, 6400], [0, 0], [5, 5]), "window 1"),               # starts before it
        (([0, 100], [6400, 300], [0, 0], [5, 1]), "window 1"),               # shorter than the receptive field
        (([0, 100], [6400, 6400], [0, 0], [5, 0]), "window 1"),              # keeps no frame
        (([0, 100], [6400, 6400], [0, nf - 4], [5, 5]), "window 1"),         # kept range past the window's frames
        (([0, 100], [6400, 6400], [-1, 0], [5, 5]), "window 0"),
    ]:
        rc, msg = call(*args)
        assert rc != 0 and word in msg, (args, rc, msg)
    assert call([0], [6400], [0], [5], normalize=2)[0] != 0
    assert lib.w2v2_forward_windows(m._handle, N.ptr(wave), 20000, 0, None, None, None, None, 0, N.ptr(out), N.current_stream()) != 0
    m.set_precision("bf16")
    try:
        rc, msg = call([0], [6400], [0], [5])
        assert rc != 0 and "bf16" in msg
    finally:
        m.set_precision("fp32")


# ---- pause cuts ----

def random_logits(rng, T, V, blank, margin):
    """Rows with a clear winner, in runs: quiet blanks (runs of up to 3 chunks), blanks that lead by less than the margin,
    labels; then ties, NaN rows, -inf entries and leads of exactly the margin sprinkled over them."""
    x = rng.standard_normal((T, V)).astype(np.float32)
    if V == 1:                                                   # every frame is quiet, but for the NaN ones
        x[rng.integers(0, T, size=T // 20)] = np.nan
        return x
    t = 0
    while t < T:
        kind = rng.integers(0, 4)
        n = int(rng.integers(1, 3200)) if kind == 0 and rng.random() < 0.2 else int(rng.integers(1, 40))
        win = blank if kind < 2 else int(rng.integers(0, V))
        x[t:t + n, win] = np.float32(12.0)
        if kind == 1 and V > 1:
            x[t:t + n, (blank + 1) % V] = np.float32(11.0)      # argmax the blank, lead 1 < margin
        t += n
    others = [v for v in range(V) if v != blank]
    for t in rng.integers(0, T, size=max(1, T // 50)):
        what = rng.integers(0, 4)
        if what == 0:
            x[t, :] = np.float32(1.0)                            # everything ties: the argmax is label 0
        elif what == 1:
            x[t, rng.integers(0, V)] = np.nan
        elif what == 2:
            x[t, others] = -np.inf
        else:
            x[t, :] = np.float32(0.5)
            x[t, blank] = np.float32(0.5) + np.float32(margin)  # the lead equals the margin exactly
    return x


def device_cuts(torch_mod, parts, **kw):
    from wav2vec2.longform import pause_cuts
    return pause_cuts(parts, **kw)


@pytest.mark.parametrize("min_pause", [1, 8])
@pytest.mark.parametrize("V", [1, 5, 32])
def test_pause_cuts_equal_the_reference(torch_mod, V, min_pause):
    from wav2vec2 import _native as N
    assert N.CUTS_CHUNK == 1024          # its neighbours 1023 and 1025 are in the list
    rng = np.random.default_rng(1000 * V + min_pause)
    blank, margin = (0, 2.0) if V == 1 else (V // 2, 2.0)
    delim = -1 if V == 1 else (blank + 2) % V
    lens = [1, 2, 63, 64, 65, 1023, 1024, 1025, 5000]
    xs = [random_logits(rng, T, V, blank, margin) for T in lens]
    packed = torch_mod.from_numpy(np.concatenate(xs)).cuda()
    parts = list(torch_mod.split(packed, lens))
    for d in sorted({-1, delim}):
        got = device_cuts(torch_mod, parts, blank=blank, delimiter_id=None if d < 0 else d, margin=margin, min_pause=min_pause)
        again = device_cuts(torch_mod, parts, blank=blank, delimiter_id=None if d < 0 else d, margin=margin, min_pause=min_pause)
        total = 0
        for x, g, g2 in zip(xs, got, again):
            c, p = R.pause_cuts(x, blank, d, margin, min_pause)
            assert g.count == len(c) and np.array_equal(g.cuts, c) and np.array_equal(g.pauses, p), (len(x), d)
            assert g2.count == g.count and np.array_equal(g2.cuts, g.cuts) and np.array_equal(g2.pauses, g.pauses)
            total += len(c)
        assert total > 0


def planted(T, V, blank):
    x = np.zeros((T, V), np.float32)
    x[:, (blank + 1) % V] = np.float32(9.0)          # a label everywhere, until something is planted
    return x


def quiet(x, a, b, blank):
    x[a:b, :] = 0.0
    x[a:b, blank] = np.float32(9.0)


def test_pause_cuts_planted_cases(torch_mod):
    V, blank, D, margin = 5, 0, 3, 2.0
    C = 1024
    # 0: pauses that straddle a chunk edge, end exactly at one, start exactly at one; one spanning more than two chunks
    a = planted(8000, V, blank)
    for lo, hi in [(C - 5, C + 5), (2 * C - 10, 2 * C), (3 * C, 3 * C + 7), (4 * C - 3, 6 * C + 9), (7 * C - 1, 7 * C + 1)]:
        quiet(a, lo, hi, blank)
    # 1: a delimiter, then more than two chunks of frames whose argmax is the blank but which are not quiet, then the pause:
    #    the label crosses chunks.  The same behind another label must be refused.
    b = planted(8000, V, blank)
    b[10, :] = 0.0
    b[10, D] = np.float32(9.0)
    b[11:2500, :] = 0.0
    b[11:2500, blank] = np.float32(9.0)
    b[11:2500, 2] = np.float32(8.0)                   # lead 1 < margin
    quiet(b, 2500, 2520, blank)
    b[2520, 2] = np.float32(9.5)                      # a label that is not the delimiter
    b[2521:5000, :] = 0.0
    b[2521:5000, blank] = np.float32(9.0)
    b[2521:5000, 2] = np.float32(8.0)
    quiet(b, 5000, 5030, blank)
    quiet(b, 6000, 6003, blank)
    # 2: ties, NaN, margin equality, -inf
    c = planted(300, V, blank)
    quiet(c, 10, 20, blank)
    c[14, 2] = np.float32(9.0)                        # ties the blank inside a pause: argmax blank, lead 0: splits it
    quiet(c, 40, 50, blank)
    c[45, 4] = np.nan                                 # a NaN row splits a pause, and counts as a label that is not D
    quiet(c, 70, 80, blank)
    c[70:80, blank] = np.float32(2.0)                 # lead exactly the margin
    quiet(c, 100, 110, blank)
    c[100:110, blank] = np.nextafter(np.float32(2.0), np.float32(0.0))      # one ulp short
    quiet(c, 130, 140, blank)
    c[130:140, 1:] = -np.inf                          # lead +inf
    quiet(c, 160, 170, blank)
    c[160:170, :] = -np.inf                           # rows of -inf only: argmax 0 = blank, lead NaN
    quiet(c, 0, 5, blank)                             # a pause at the start
    quiet(c, 290, 300, blank)                         # and at the end: neither counts
    xs = [a, b, c]
    lens = [len(x) for x in xs]
    packed = torch_mod.from_numpy(np.concatenate(xs)).cuda()
    parts = list(torch_mod.split(packed, lens))
    padded = np.zeros((3, max(lens), V), np.float32)
    for i, x in enumerate(xs):
        padded[i, :len(x)] = x
    padded = torch_mod.from_numpy(padded).cuda()
    for d in (-1, D):
        for min_pause in (1, 2, 8):
            kw = dict(blank=blank, delimiter_id=None if d < 0 else d, margin=margin, min_pause=min_pause)
            ref = [R.pause_cuts(x, blank, d, margin, min_pause) for x in xs]
            views = device_cuts(torch_mod, parts, **kw)
            batch = device_cuts(torch_mod, padded, frame_lengths=lens, **kw)
            for i, (rc, rp) in enumerate(ref):
                one = device_cuts(torch_mod, [torch_mod.from_numpy(xs[i]).cuda()], **kw)[0]
                for g in (views[i], batch[i], one):
                    assert g.count == len(rc) and np.array_equal(g.cuts, rc) and np.array_equal(g.pauses, rp), (i, d, min_pause)
    # what the planted cases are there for
    rc, rp = R.pause_cuts(a, blank, -1, margin, 8)
    assert rc.tolist() == [C, 2 * C - 5, 5 * C + 3] and rp.tolist() == [10, 10, 2 * C + 12]
    rc, _ = R.pause_cuts(b, blank, D, margin, 8)
    assert rc.tolist() == [2510]
    assert R.pause_cuts(b, blank, -1, margin, 8)[0].tolist() == [2510, 5015]
    assert R.pause_cuts(c, blank, -1, margin, 1)[0].tolist() == [12, 17, 42, 48, 75, 135]
    # more pauses than slots: the first max_cuts are stored, the count is the true one
    few = device_cuts(torch_mod, parts, blank=blank, margin=margin, min_pause=1, max_cuts=2)
    for g, x in zip(few, xs):
        rc, rp = R.pause_cuts(x, blank, -1, margin, 1)
        assert g.count == len(rc) > 2 and np.array_equal(g.cuts, rc[:2]) and np.array_equal(g.pauses, rp[:2])


def test_pause_cuts_argument_checks(torch_mod):
    from wav2vec2.longform import pause_cuts
    x = torch_mod.zeros((10, 5), device="cuda")
    for kw in (dict(blank=5), dict(blank=0, delimiter_id=0), dict(blank=0, delimiter_id=5), dict(min_pause=0), dict(max_cuts=0)):
        with pytest.raises(ValueError):
            pause_cuts([x], **kw)
    from wav2vec2 import _native as N
    lib = N.load()
    out = torch_mod.empty(8, dtype=torch_mod.int32, device="cuda")
    row0, frames = np.zeros(1, np.int64), np.array([10], np.int32)

    def rc(V=5, n=1, blank=0, delim=-1, margin=2.0, min_pause=1, max_cuts=4, frames=frames):
        return lib.w2v2_ctc_pause_cuts(N.ptr(x), V, n, N.ptr(row0), N.ptr(frames), blank, delim, margin, min_pause, max_cuts, N.ptr(out),
                                       N.ptr(out), N.ptr(out), N.current_stream())

    assert rc() == 0
    for bad in (dict(n=0), dict(V=0), dict(blank=5), dict(blank=-1), dict(delim=5), dict(delim=0), dict(delim=-2), dict(min_pause=0),
                dict(max_cuts=0), dict(margin=float("nan")), dict(frames=np.array([0], np.int32)),
                dict(frames=np.array([(1 << 24) + 1], np.int32))):
        assert rc(**bad) != 0, bad
    torch_mod.cuda.synchronize()


# ---- decoding ----

@pytest.fixture(scope="module")
def tokenizer():
    from wav2vec2 import Wav2Vec2Processor
    return Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))


def test_decode_long_on_planted_logits(torch_mod, tokenizer):
    from wav2vec2.decoding import beam_search
    from wav2vec2.alignment import forced_align, token_spans, word_spans
    from wav2vec2.longform import decode_long
    tokens = tokenizer.get_vocab()
    V, blank, delim = len(tokens), tokens["<pad>"], tokens["|"]
    letters = [i for t, i in tokens.items() if len(t) == 1 and t.isalpha()]
    rng = np.random.default_rng(77)
    T, spf = 1500, 0.02
    x, _ = R.peaky_logits(rng, T, V, blank, delim, 10, n_pauses=5, letters=letters)
    logits = torch_mod.from_numpy(x).cuda()
    kw = dict(blank=blank, min_pause=10, min_frames=100, max_frames=400, seconds_per_frame=spf)
    # greedy: the collapse of the whole matrix
    g = decode_long(logits, tokenizer, beam_width=None, **kw)
    assert len(g.segments) >= 3
    assert list(g.ids) == R.greedy(x, blank)
    assert g.text == tokenizer.decode(g.ids, skip_special_tokens=True, group_tokens=False) and g.words is None
    # the beam: each segment is beam_search on its slice, ids their concatenation
    b = decode_long(logits, tokenizer, beam_width=8, nbest=3, timestamps=True, **kw)
    assert len(b.segments) >= 3
    edges = [int(round(s.start_s / spf)) for s in b.segments] + [T]
    assert edges[0] == 0 and [s.end_s for s in b.segments] == [e * spf for e in edges[1:]]
    slices = [torch_mod.from_numpy(x[s:e].copy()).cuda() for s, e in zip(edges, edges[1:])]
    direct = beam_search(slices, beam_width=8, nbest=3, blank=blank)
    assert [s.transcript.hypotheses for s in b.segments] == direct
    assert list(b.ids) == [i for h in direct for i in h[0].ids]
    assert b.score == sum(h[0].score for h in direct) and b.total == sum(h[0].total for h in direct)
    assert [s.transcript.text for s in b.segments] == [h[0].text(tokenizer) for h in direct]
    # timestamps: the segment-local alignment plus the segment's start
    local = forced_align(slices, [list(h[0].ids) for h in direct], blank=blank)
    vocab = {i: (" " if t == "|" else t) for t, i in tokens.items()}
    expect = []
    for s, a in zip(b.segments, local):
        ws = word_spans(token_spans(a), delim, spf, vocab)
        assert s.transcript.words == ws
        expect.extend(w._replace(start_s=w.start_s + s.start_s, end_s=w.end_s + s.start_s) for w in ws)
    assert b.words == expect and len(b.words) > 3
    assert all(0.0 <= w.start_s < w.end_s <= T * spf for w in b.words)
    assert all(u.end_s <= v.start_s for u, v in zip(b.words, b.words[1:]))
    # a list of recordings gives a list, each as alone
    two = decode_long([logits, logits[:700]], tokenizer, beam_width=8, nbest=3, timestamps=True, **kw)
    assert two[0] == b and two[1] == decode_long(logits[:700].clone(), tokenizer, beam_width=8, nbest=3, timestamps=True, **kw)


def test_transcribe_long_is_predict_long_then_decode_long(models, tokenizer):
    from wav2vec2.longform import decode_long
    m = models["tiny_base"]
    assert m.config.vocab_size == len(tokenizer.get_vocab())
    waves = [noise(90, 9000), noise(91, 14000)]
    got = m.transcribe_long(waves, tokenizer, beam_width=4, nbest=2, timestamps=True, window_s=WINDOW_S, margin_s=MARGIN_S)
    logits = m.predict_long(waves, WINDOW_S, MARGIN_S)
    ref = decode_long(logits, tokenizer, beam_width=4, nbest=2, blank=m.config.pad_id, timestamps=True,
                      seconds_per_frame=320 / 16000.0)
    assert len(got) == 2 and got == ref
    assert all(isinstance(t.text, str) and t.words is not None and len(t.segments) >= 1 for t in got)
