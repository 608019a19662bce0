"""Forced alignment of whole recordings on the GPU (w2v2_ctc_align_long, wav2vec2.alignment.forced_align_long):
the tiled Viterbi against the fp64 numpy reference (tests/align_reference.py) at every tile edge, identical bits with
w2v2_ctc_align where both accept the input, repeats across a strip boundary, exact ties and non-finite logits at tile edges,
a transcript beyond the one-block aligner's 8191 labels, infeasible and bad recordings among good ones, isolation and
determinism, the C ABI's argument and workspace checks, and Wav2Vec2ForCTC.align_long.

Strips of 64 pairs and panels of 8 / 16 / 32 frames put every tile edge through inputs of a few hundred frames."""

import os

import numpy as np
import pytest

import align_reference as AR
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def rand_labels(rng, U, V, blank, rep=0.1):
    pool = np.asarray([v for v in range(V) if v != blank])
    out = []
    for _ in range(U):
        if out and rng.random() < rep:
            out.append(out[-1])
        else:
            out.append(int(rng.choice(pool)))
    return out


def host(al):
    return al.token.cpu().numpy(), al.label_index.cpu().numpy(), al.frame_logp.cpu().numpy(), al.score


def same_bits(a, b):
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u, v)
    assert np.float64(a[3]).tobytes() == np.float64(b[3]).tobytes() or (np.isnan(a[3]) and np.isnan(b[3])), (a[3], b[3])


def assert_matches(got, ref):
    """the bars of test_align_gpu.py (the reference's lse sums in another order); NaNs in the same places"""
    tok, li, fl, sc = got
    rtok, rli, rfl, rsc = ref
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(li, rli)
    np.testing.assert_array_equal(np.isnan(fl), np.isnan(rfl))
    np.testing.assert_allclose(fl, rfl, rtol=0, atol=1e-6, equal_nan=True)
    if np.isfinite(rsc):
        assert abs(sc - rsc) <= 1e-9 * max(1.0, abs(rsc)), (sc, rsc)
    else:
        assert (np.isnan(sc) and np.isnan(rsc)) or sc == rsc, (sc, rsc)


def align_long(torch, xs, labels, blank=0, sp=None, pf=None, **kw):
    from wav2vec2.alignment import forced_align_long
    als = forced_align_long([torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs], labels, blank=blank, strip_pairs=sp,
                            panel_frames=pf, **kw)
    return [host(a) for a in als]


def raw_call(torch, xs, labels, blank=0, sp=0, pf=0, cap=0):
    """the C ABI itself, labels on the device unchecked: (rc, [(token, label_index, frame_logp, score) per recording])"""
    from wav2vec2 import _native as N
    lens = [x.shape[0] for x in xs]
    V = xs[0].shape[1]
    base = torch.from_numpy(np.concatenate(xs)).cuda()
    lab = torch.from_numpy(np.concatenate([np.asarray(l, np.int32) for l in labels] + [np.zeros(1, np.int32)])).cuda()
    row0 = np.cumsum([0] + lens[:-1]).astype(np.int64)
    label0 = np.cumsum([0] + [len(l) for l in labels[:-1]]).astype(np.int64)
    frames = np.asarray(lens, np.int32)
    nlab = np.asarray([len(l) for l in labels], np.int32)
    tot, n = sum(lens), len(xs)
    tok = torch.empty(tot, dtype=torch.int32, device="cuda")
    li = torch.empty_like(tok)
    fl = torch.empty(tot, dtype=torch.float32, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    rc = N.load().w2v2_ctc_align_long(N.ptr(base), V, n, N.ptr(row0), N.ptr(frames), N.ptr(lab), N.ptr(label0), N.ptr(nlab), blank,
                                      N.ptr(tok), N.ptr(li), N.ptr(fl), N.ptr(sc), sp, pf, cap, N.current_stream())
    if rc:
        return rc, None
    out, o = [], 0
    tok, li, fl, sc = tok.cpu().numpy(), li.cpu().numpy(), fl.cpu().numpy(), sc.cpu().numpy()
    for i, T in enumerate(lens):
        out.append((tok[o:o + T], li[o:o + T], fl[o:o + T], float(sc[i])))
        o += T
    return 0, out


# ---- 1. tile edges against the reference --------------------------------------------------------------------------------------
EDGE_US = [0, 1, 62, 63, 64, 65, 127, 128, 129, 200]       # pairs = U + 1: 63 fills one strip of 64, 64 leaves the last blank alone in a second
_edge_cache = {}


def edge_cases(V, blank):
    """(logits, labels) of every case and the reference's outputs, computed once per vocabulary"""
    if V not in _edge_cache:
        rng = np.random.default_rng(1000 + V)
        cases = []
        for U in EDGE_US:
            labels = rand_labels(rng, U, V, blank, rep=0.2)
            for T in (max(1, U + AR.repeats(labels)), max(1, int(2.2 * U) + 1)):       # the forced path, and room to move
                cases.append((rng.standard_normal((T, V)).astype(np.float32) * 3, labels))
        for U in (0, 1, 2, 3):
            for T in (1, 2, 7, 8, 9, 16, 17):
                labels = rand_labels(rng, U, V, blank, rep=0.3)
                if T >= U + AR.repeats(labels):
                    cases.append((rng.standard_normal((T, V)).astype(np.float32) * 3, labels))
        _edge_cache[V] = (cases, [AR.viterbi(x, l, blank) for x, l in cases])
    return _edge_cache[V]


@pytest.mark.parametrize("pf", [8, 16, 32])
@pytest.mark.parametrize("V,blank", [(32, 0), (400, 7)])
def test_tile_edges_match_reference(torch_mod, V, blank, pf):
    cases, refs = edge_cases(V, blank)
    got = align_long(torch_mod, [c[0] for c in cases], [c[1] for c in cases], blank, sp=64, pf=pf)
    for g, r in zip(got, refs):
        assert_matches(g, r)


# ---- 2. the bits of forced_align ------------------------------------------------------------------------------------------------
# (512 x 64 runs 2 pairs per thread; 2048 x 256 is cut to the 1088 pairs the longest recording needs: 8 pairs per thread on 136 of 192 threads)
@pytest.mark.parametrize("sp,pf", [(64, 8), (256, 64), (None, None), (512, 64), (2048, 256)])
def test_equal_bits_with_forced_align(torch_mod, sp, pf):
    from wav2vec2.alignment import forced_align
    rng = np.random.default_rng(42)
    xs, labels = [], []
    for U in (5, 300, 1024):
        l = rand_labels(rng, U, 32, 0)
        T = max(int(2.2 * U) + 1, U + AR.repeats(l))
        xs.append(rng.standard_normal((T, 32)).astype(np.float32) * 2)
        labels.append(l)
    want = [host(a) for a in forced_align([torch_mod.from_numpy(x).cuda() for x in xs], labels)]
    got = align_long(torch_mod, xs, labels, sp=sp, pf=pf)
    for g, w in zip(got, want):
        same_bits(g, w)


# ---- 3. a repeat across a strip boundary ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [63, 64])
def test_repeat_across_a_strip_boundary(torch_mod, at):
    rng = np.random.default_rng(at)
    U, V = 140, 32
    labels = rand_labels(rng, U, V, 0, rep=0.0)
    for k in range(1, U):                                   # no repeat anywhere ...
        while labels[k] == labels[k - 1]:
            labels[k] = int(rng.integers(1, V))
    labels[at + 1] = labels[at]                             # ... but l_at == l_{at + 1}: pair 64 is the first of the second strip
    while labels[at + 2] in (labels[at + 1], labels[at + 3]):
        labels[at + 2] = labels[at + 2] % (V - 1) + 1
    assert AR.repeats(labels) == 1
    T = U + 1
    x = rng.standard_normal((T, V)).astype(np.float32) * 3
    forced = labels[:at + 1] + [0] + labels[at + 1:]        # the only path of U + R frames
    for pf in (8, 16):
        (got,) = align_long(torch_mod, [x], [labels], sp=64, pf=pf)
        assert got[0].tolist() == forced
        assert_matches(got, AR.viterbi(x, labels, 0))


# ---- 4. exact ties, -inf and NaN at tile edges ---------------------------------------------------------------------------------
def test_exact_ties_and_non_finite_logits_at_edges(torch_mod):
    rng = np.random.default_rng(17)
    U, T, V = 150, 400, 8
    labels = rand_labels(rng, U, V, 0, rep=0.3)
    assert T >= U + AR.repeats(labels)
    ties = rng.integers(-2, 3, size=(T, V)).astype(np.float32)
    inf = ties.copy()
    inf[[15, 16, 17, 200, 399], labels[63]] = -np.inf       # a -inf column on some frames, around a panel edge among them
    inf[48, 0] = -np.inf
    nan = ties.copy()
    nan[80, labels[63]] = np.nan                            # step 80 is the last of panel 4 (steps 65 .. 80); pair 63 the last of strip 0
    xs = [ties, inf, nan]
    got = align_long(torch_mod, xs, [labels] * 3, sp=64, pf=16)
    refs = [AR.viterbi(x, labels, 0) for x in xs]
    assert np.isfinite(refs[0][3]) and np.isnan(refs[2][3]) and np.isnan(refs[2][2]).sum() >= 1
    for g, r in zip(got, refs):
        assert_matches(g, r)


# ---- 5. beyond the one-block aligner's limit -----------------------------------------------------------------------------------
def test_beyond_8191_labels(torch_mod):
    from wav2vec2.alignment import forced_align
    rng = np.random.default_rng(8500)
    U, V = 8500, 32
    labels = rand_labels(rng, U, V, 0)
    T = max(int(2.2 * U) + 1, U + AR.repeats(labels))
    x = rng.standard_normal((T, V)).astype(np.float32) * 2
    (got,) = align_long(torch_mod, [x], [labels])
    assert_matches(got, AR.viterbi(x, labels, 0))
    with pytest.raises(ValueError, match="at most 8191"):
        forced_align([torch_mod.from_numpy(x).cuda()], [labels])


# ---- 6. infeasible and bad recordings among good ones ------------------------------------------------------------------------
def test_bad_recordings_leave_neighbours_alone(torch_mod):
    rng = np.random.default_rng(6)
    V = 32
    good_a, good_e = rand_labels(rng, 150, V, 0), rand_labels(rng, 70, V, 0)
    short = rand_labels(rng, 140, V, 0, rep=0.2)
    past_v, is_blank = rand_labels(rng, 200, V, 0), rand_labels(rng, 200, V, 0)
    past_v[130] = V                                         # pairs 128 .. 191 are the third strip of 64
    is_blank[135] = 0
    labels = [good_a, short, past_v, is_blank, good_e]
    Ts = [330, 140 + AR.repeats(short) - 1, 450, 450, 100]
    xs = [rng.standard_normal((T, V)).astype(np.float32) for T in Ts]
    rc, got = raw_call(torch_mod, xs, labels, sp=64, pf=16)
    assert rc == 0
    for i in (0, 4):
        rc, solo = raw_call(torch_mod, [xs[i]], [labels[i]], sp=64, pf=16)
        assert rc == 0
        same_bits(got[i], solo[0])
        assert_matches(got[i], AR.viterbi(xs[i], labels[i], 0))
    tok, li, fl, sc = got[1]
    assert sc == -np.inf and (tok == -1).all() and (li == -1).all() and np.isnan(fl).all()
    for i in (2, 3):
        tok, li, fl, sc = got[i]
        assert np.isnan(sc) and (tok == -1).all() and (li == -1).all() and np.isnan(fl).all()


# ---- 7. isolation and determinism -----------------------------------------------------------------------------------------------
def test_isolation_and_determinism(torch_mod):
    rng = np.random.default_rng(7)
    shapes = [(10, 50), (100, 260), (200, 450), (70, 90)]   # 1 .. 4 strips of 64 pairs, 4 .. 29 panels of 16 frames
    labels = [rand_labels(rng, U, 32, 0) for U, _ in shapes]
    xs = [rng.standard_normal((max(T, U + AR.repeats(l)), 32)).astype(np.float32) for (U, T), l in zip(shapes, labels)]
    ref = align_long(torch_mod, xs, labels, sp=64, pf=16)
    for g, w in zip(align_long(torch_mod, xs, labels, sp=64, pf=16), ref):          # the call repeated
        same_bits(g, w)
    for i in range(len(xs)):                                                         # each one alone
        same_bits(align_long(torch_mod, [xs[i]], [labels[i]], sp=64, pf=16)[0], ref[i])
    perm = [2, 0, 3, 1]
    for g, i in zip(align_long(torch_mod, [xs[i] for i in perm], [labels[i] for i in perm], sp=64, pf=16), perm):
        same_bits(g, ref[i])
    for g, x, l in zip(ref, xs, labels):
        assert_matches(g, AR.viterbi(x, l, 0))


# ---- 8. the C ABI's checks ----------------------------------------------------------------------------------------------------
def test_c_abi_argument_and_workspace_checks(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    from wav2vec2.alignment import forced_align_long
    lib = N.load()
    V = 8
    x = torch.zeros((40, V), device="cuda")
    lab = torch.ones(64, dtype=torch.int32, device="cuda")
    tok = torch.empty(40, dtype=torch.int32, device="cuda")
    li, fl, sc = torch.empty_like(tok), torch.empty(40, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    row0, label0 = np.zeros(1, np.int64), np.zeros(1, np.int64)

    def call(logits=N.ptr(x), n=1, frames=(40,), nlab=(3,), blank=0, r0=row0, tokp=N.ptr(tok), lb0=label0, sp=0, pf=0, cap=0,
             framesp=True):
        fr, nl = np.asarray(frames, np.int32), np.asarray(nlab, np.int32)
        return lib.w2v2_ctc_align_long(logits, V, n, N.ptr(r0), N.ptr(fr) if framesp else None, N.ptr(lab), N.ptr(lb0), N.ptr(nl),
                                       blank, tokp, N.ptr(li), N.ptr(fl), N.ptr(sc), sp, pf, cap, N.current_stream())

    assert call() == 0 and call(sp=64, pf=8) == 0
    torch.cuda.synchronize()
    for kw, msg in [(dict(sp=96), "strip_pairs"), (dict(sp=32), "strip_pairs"), (dict(sp=8256), "strip_pairs"),
                    (dict(pf=12), "panel_frames"), (dict(pf=4), "panel_frames"), (dict(logits=None), "null"),
                    (dict(tokp=None), "null"), (dict(framesp=False), "null"), (dict(n=0), "recordings"),
                    (dict(frames=(0,)), "frames"), (dict(frames=(-1,)), "frames"), (dict(nlab=(-1,)), "labels"),
                    (dict(blank=V), "blank"), (dict(blank=-1), "blank"), (dict(cap=-1), "max_workspace_bytes"),
                    (dict(r0=np.full(1, -1, np.int64)), "negative"), (dict(lb0=np.full(1, -1, np.int64)), "negative")]:
        assert call(**kw) == -1, kw                          # W2V2_EINVAL
        assert msg in N.last_error(), (kw, N.last_error())
    # the workspace: the figure of w2v2_ctc_align_long_workspace is the one the refusal names, and Python raises MemoryError
    fr, nl = np.asarray([40], np.int32), np.asarray([3], np.int32)
    need = lib.w2v2_ctc_align_long_workspace(1, N.ptr(fr), N.ptr(nl), 64, 8)
    assert need > 8 * (40 + 7 + 40) + 40 * 4 // 2
    assert call(sp=64, pf=8, cap=need) == 0
    assert call(sp=64, pf=8, cap=need - 1) == -1
    assert f"{need} bytes" in N.last_error() and "max_workspace_bytes" in N.last_error()
    assert lib.w2v2_ctc_align_long_workspace(1, N.ptr(fr), N.ptr(nl), 96, 8) < 0 and "strip_pairs" in N.last_error()
    # an hour of speech: 2 bits per frame and state dominate
    fr, nl = np.asarray([180000], np.int32), np.asarray([54000], np.int32)
    hour = lib.w2v2_ctc_align_long_workspace(1, N.ptr(fr), N.ptr(nl), 0, 0)
    assert 180000 * 54001 // 2 < hour < 1.2 * 180000 * 54001 // 2      # (the last strip is padded: less than 8192 pairs in 54001)
    with pytest.raises(MemoryError, match=f"40 frames x 3 labels need {need} bytes"):
        forced_align_long(x, [1, 2, 3], strip_pairs=64, panel_frames=8, max_workspace_bytes=need - 1)
    torch.cuda.synchronize()


# ---- 9. model level -------------------------------------------------------------------------------------------------------------
WINDOW_S, MARGIN_S = 6400 / 16000.0, 640 / 16000.0


def test_model_align_long(torch_mod):
    import wav2vec2
    from wav2vec2 import Wav2Vec2Processor
    from wav2vec2.alignment import Alignment, token_spans, word_spans
    cfg = H.case_config("tiny_base")
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights("tiny_base"))
    tokenizer = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))
    tokens = tokenizer.get_vocab()
    assert cfg.vocab_size == len(tokens)
    vocab = {i: (" " if t == "|" else t) for t, i in tokens.items()}
    spf = 320 / 16000.0
    rng = np.random.default_rng(9)
    waves = [rng.standard_normal(16000).astype(np.float32), rng.standard_normal(11000).astype(np.float32)]     # about three and two windows
    texts = ["SO IT GOES ON", "ALL OF IT"]

    def expect(logits, text):
        x = logits.cpu().numpy()
        tok, li, fl, sc = AR.viterbi(x, tokenizer(text), cfg.pad_id)
        return word_spans(token_spans(Alignment(tok, li, fl, sc)), tokens["|"], spf, vocab)

    def check(got, want, text):
        assert [w.text for w in got] == text.split()
        assert [(w.text, w.start_s, w.end_s) for w in got] == [(w.text, w.start_s, w.end_s) for w in want]
        np.testing.assert_allclose([w.score for w in got], [w.score for w in want], rtol=0, atol=1e-6)

    kw = dict(window_s=WINDOW_S, margin_s=MARGIN_S)
    singles = [m.align_long(w, t, tokenizer, **kw) for w, t in zip(waves, texts)]
    for got, w, t in zip(singles, waves, texts):
        check(got, expect(m.predict_long(w, WINDOW_S, MARGIN_S), t), t)
    assert m.align_long(waves, texts, tokenizer, **kw) == singles
    # ids in place of text
    assert m.align_long(waves[0], tokenizer(texts[0]), delimiter_id=tokens["|"], **kw) == \
        [w._replace(text=tuple(tokens[c] for c in w.text)) for w in singles[0]]
    # another sampling rate: the times stay seconds of the recording
    w8 = rng.standard_normal(8000).astype(np.float32)       # one second at 8 kHz
    got = m.align_long(w8, texts[1], tokenizer, sampling_rate=8000, **kw)
    check(got, expect(m.predict_long(w8, WINDOW_S, MARGIN_S, sampling_rate=8000), texts[1]), texts[1])
    assert 0.0 <= got[0].start_s and got[-1].end_s <= 1.0
