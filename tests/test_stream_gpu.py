"""Streaming transcription on the GPU: the resumable beam search (w2v2_ctc_beam_search_stream,
wav2vec2.decoding.BeamStream) and the session on top of it (wav2vec2.streaming, Wav2Vec2ForCTC.stream).

Every equality here is between two runs of this project's own kernels and is BITWISE: labels, lengths, and the fp64 scores and
totals compared as integers.  There is no allowance for fragile utterances: a chunked search that decides anything differently
from the one-call search, or a one-call search that differs from the offline kernel, fails."""

import functools
import math
import os

import numpy as np
import pytest

import bias_reference as B
import helpers as H
import wordlm_reference as WR

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")
NEG = -math.inf
EINVAL = -1

# (V, blank, delimiter, lexicon words, word model order)
VOCABS = {32: (32, 31, 4, 60, 3), 5: (5, 0, 1, 8, 2)}
# no model, a character 3-gram, a word model open / constrained, a phrase bias over no model, over the table and over the word model
FORMS = ["none", "char3", "word", "word_constrained", "bias", "bias_char3", "bias_word"]
WIDTHS = [1, 4, 16, 64]
FRAMES = [1, 2, 9, 50, 300]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def models(V, form):
    """(blank, lm, bias) of one form, seeded"""
    from wav2vec2.decoding import CharNgramLM, ContextBias
    _, blank, delim, nwords, order = VOCABS[V]
    rng = np.random.default_rng(500 + 10 * V + FORMS.index(form))
    base = "none" if form == "bias" else form.replace("bias_", "")
    lm = None
    if base == "char3":
        lm = CharNgramLM(np.log(rng.dirichlet(np.ones(V), V ** 2)).astype(np.float32), 3, alpha=0.8, beta=-0.2)
    elif base.startswith("word"):
        lm = WR.random_model(rng, V, blank, delim, nwords, order, alpha=0.8, beta=0.3,
                             unk_penalty=NEG if base == "word_constrained" else -2.0)
    bias = None
    if form.startswith("bias"):
        whole = form != "bias"
        phrases = B.random_phrases(rng, V, blank, delim, 8, maxlen=4, words=whole)
        if base == "word":                                   # some phrases made of lexicon words
            sp = sorted(lm.lexicon.values())
            phrases[0] = (sp[0] + (delim,) + sp[1], 1.5)
            phrases[1] = (sp[2], 0.75)
            phrases = list({tuple(h): b for h, b in phrases}.items())
        bias = ContextBias(phrases, V, blank, delim, 1.0, whole)
    return blank, lm, bias


def logits_for(V, form, T, seed, peaky):
    """T frames: random or peaky (as tests/test_beam_gpu.py's make_logits); the word forms at T >= 50 spell lexicon words instead when
    `peaky`, so that the constrained search has something to find"""
    blank, lm, _ = models(V, form)
    rng = np.random.default_rng(seed)
    if peaky and "word" in form and T >= 50:
        x = WR.word_logits(rng, lm, T, blank)
        while x.shape[0] < T:
            x = np.concatenate([x, WR.word_logits(rng, lm, T, blank)])
        return np.ascontiguousarray(x[:T])
    return WR.make_logits(rng, T, V, blank, peaky)


def bits(hyps):
    """a hypothesis list as integers: ids, and the bit patterns of score and total"""
    return [(h.ids, int(np.float64(h.score).view(np.int64)), int(np.float64(h.total).view(np.int64))) for h in hyps]


def stream(V, form, n=1, W=16, nbest=1, **kw):
    from wav2vec2.decoding import BeamStream
    blank, lm, bias = models(V, form)
    return BeamStream(n, V, beam_width=W, nbest=nbest, blank=blank, lm=lm, bias=bias, **kw)


def one_call(torch, V, form, x, W, nbest):
    s = stream(V, form, 1, W, nbest)
    step = s.advance([torch.from_numpy(x).cuda()])[0]
    assert step.frames_done == x.shape[0]
    return step


def offline(torch, V, form, x, W, nbest):
    from wav2vec2.decoding import beam_search
    blank, lm, bias = models(V, form)
    return beam_search([torch.from_numpy(x).cuda()], beam_width=W, nbest=nbest, blank=blank, lm=lm, bias=bias)[0]


def schedules(rng, T):
    """the chunkings of T frames: single frames (T <= 50; beyond that they would only add launches), eights, 7 and 9 in turn (which
    cross the ring of 8 frames both ways), random sizes, and a call of no frames in the middle"""
    def cut(sizes):
        out, left = [], T
        for s in sizes:
            if left <= 0:
                break
            out.append(min(s, left))
            left -= out[-1]
        assert sum(out) == T
        return out
    ones = cut([1] * T) if T <= 50 else cut([50] * T)
    rnd = cut([int(v) for v in rng.integers(1, max(2, T // 2 + 1), T)])
    return [ones, cut([8] * T), cut([7, 9] * T), rnd, [T // 2, 0, T - T // 2]]


def run_schedules(torch, s, xd, scheds, every=3):
    """stream k of `s` takes `xd` in the chunks scheds[k]; results are asked for on every `every`-th call and on a last call of no
    frames at all, whose steps are returned"""
    pos = [0] * len(scheds)
    for k in range(max(len(c) for c in scheds)):
        parts = []
        for j, c in enumerate(scheds):
            if k < len(c):
                parts.append(xd[pos[j]:pos[j] + c[k]])
                pos[j] += c[k]
            else:
                parts.append(None)
        s.advance(parts, results=k % every == 0)
    return s.advance([None] * len(scheds))


# ---- 2 and 3: any chunking equals one call, one call equals the offline search ---------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("V", [32, 5])
def test_chunked_equals_one_call_equals_offline(torch_mod, V, form):
    rng = np.random.default_rng(31 * V + FORMS.index(form))
    nonempty = 0
    for W in WIDTHS:
        nbest = min(W, 4)
        for T in FRAMES:
            x = logits_for(V, form, T, 1000 * W + T, peaky=(W + T) % 2 == 0)
            ref = one_call(torch_mod, V, form, x, W, nbest)
            off = offline(torch_mod, V, form, x, W, nbest)
            assert bits(ref.hypotheses) == bits(off), (W, T, "one stream call against the offline search")
            nonempty += bool(off)
            scheds = schedules(rng, T)
            s = stream(V, form, len(scheds), W, nbest)
            steps = run_schedules(torch_mod, s, torch_mod.from_numpy(x).cuda(), scheds)
            for j, st in enumerate(steps):
                assert st.frames_done == T
                assert bits(st.hypotheses) == bits(ref.hypotheses), (W, T, scheds[j][:6])
                assert st.stable_len == ref.stable_len, (W, T, scheds[j][:6])
    assert nonempty >= (1 if form == "word_constrained" else 20)          # (the comparisons are not of empty lists)


# ---- 4: the stable prefix -----------------------------------------------------------------------------------------------------------
def common_prefix(hyps):
    ids = [h.ids for h in hyps]
    n = 0
    while all(len(i) > n for i in ids) and len({i[n] for i in ids}) == 1:
        n += 1
    return n


def follow(torch, V, form, x, W, chunk, whole_beam):
    """feed x in chunks of `chunk` with nbest = W; check the stable prefix after every call; returns [(stable_len, best ids)]"""
    s = stream(V, form, 1, W, W)
    xd = torch.from_numpy(x).cuda()
    seen, last = [], 0
    for a in range(0, x.shape[0], chunk):
        st = s.advance([xd[a:a + chunk]])[0]
        assert st.stable_len >= last, "stable_len decreased"
        last = st.stable_len
        if whole_beam:
            assert st.hypotheses and st.stable_len == common_prefix(st.hypotheses), (a, st.stable_len, common_prefix(st.hypotheses))
        if st.hypotheses:
            assert len(st.hypotheses[0].ids) >= st.stable_len
            seen.append((st.stable_len, st.hypotheses[0].ids))
    if seen:
        final = seen[-1][1]
        for n, ids in seen:
            assert final[:n] == ids[:n], "the final hypothesis does not begin with an earlier stable prefix"
    return seen


@pytest.mark.parametrize("form", ["none", "char3"])
@pytest.mark.parametrize("V", [32, 5])
def test_stable_prefix_is_the_common_prefix_of_the_beam(torch_mod, V, form):
    for W in WIDTHS:
        for peaky in (False, True):
            follow(torch_mod, V, form, logits_for(V, form, 50, 77 + W, peaky), W, 7, whole_beam=True)


@pytest.mark.parametrize("form", ["word", "word_constrained", "bias", "bias_word"])
def test_stable_prefix_holds_in_the_word_and_bias_forms(torch_mod, form):
    for V in (32, 5):
        for W in (4, 16):
            follow(torch_mod, V, form, logits_for(V, form, 60, 5 + W, True), W, 9, whole_beam=False)


def test_stable_prefix_grows_on_peaky_and_stays_zero_on_flat_input(torch_mod):
    """Peaky (V 5, width 4; tests/beam_reference.py on this seed: stable 10 of 17 labels after 50 of 60 frames): at least half of the
    final transcript is stable before the last chunk.  Flat (V 32, width 64; the reference: 0 after 5, 10, 20, 30 and 40 frames, the
    beam keeps prefixes that differ in their first label): it stays 0."""
    x = WR.make_logits(np.random.default_rng(77), 60, 5, 0, True)
    seen = follow(torch_mod, 5, "none", x, 4, 10, whole_beam=True)
    assert len(seen) == 6 and 2 * seen[-2][0] >= len(seen[-1][1]) > 0, [(n, len(i)) for n, i in seen]
    x = WR.make_logits(np.random.default_rng(902), 40, 32, 0, False)
    seen = follow(torch_mod, 32, "none", x, 64, 5, whole_beam=True)
    assert [n for n, _ in seen] == [0] * 8 and len(seen[-1][1]) > 20


# ---- 5: isolation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["none", "word", "bias_char3"])
def test_eight_streams_are_isolated(torch_mod, form):
    torch, V, W, nbest = torch_mod, 32, 16, 4
    rng = np.random.default_rng(8 + FORMS.index(form))
    Ts = [40, 55, 61, 70, 83, 96, 104, 110]
    xs = [logits_for(V, form, T, 300 + T, peaky=T % 2 == 0) for T in Ts]
    xd = [torch.from_numpy(x).cuda() for x in xs]
    refs = [one_call(torch, V, form, x, W, nbest) for x in xs]
    s = stream(V, form, 8, W, nbest)
    pos, call, last = [0] * 8, 0, None
    while any(p < T for p, T in zip(pos, Ts)):
        parts = []
        for i in range(8):
            size = int(rng.integers(1, 24))
            if pos[i] >= Ts[i] or rng.random() < 0.25:
                parts.append(None)
            else:
                parts.append(xd[i][pos[i]:pos[i] + size])
                pos[i] = min(Ts[i], pos[i] + size)
        last = s.advance(parts, results=call % 2 == 0)
        call += 1
        if call == 3:                                        # stream 3 starts again in the middle of the others' work
            assert pos[3] > 0
            s.reset(3)
            pos[3] = 0
    last = s.advance([None] * 8)
    assert call >= 8
    for i, st in enumerate(last):
        assert st.frames_done == Ts[i]
        assert bits(st.hypotheses) == bits(refs[i].hypotheses) and st.stable_len == refs[i].stable_len, i


# ---- 6: the trie buffer grows --------------------------------------------------------------------------------------------------------
def test_node_buffer_doubles_and_keeps_the_result(torch_mod):
    torch, V, W, T = torch_mod, 32, 16, 300
    for form in ("none", "word"):
        x = logits_for(V, form, T, 61, True)
        ref = one_call(torch, V, form, x, W, 4)
        s = stream(V, form, 1, W, 4, initial_frames=16)
        xd = torch.from_numpy(x).cuda()
        caps = [s._cap_frames[0]]
        for a in range(0, T, 20):
            st = s.advance([xd[a:a + 20]], results=a % 40 == 0)[0]
            caps.append(s._cap_frames[0])
        st = s.advance([None])[0]
        assert len(set(caps)) >= 4 and caps[0] == 16 and caps[-1] == 512          # 16 -> 32 -> 64 -> 128 -> 256 -> 512
        assert bits(st.hypotheses) == bits(ref.hypotheses) and st.stable_len == ref.stable_len
        assert bits(st.hypotheses) == bits(offline(torch, V, form, x, W, 4))


def test_node_buffer_cap_raises_before_allocating(torch_mod):
    torch, V, W = torch_mod, 32, 64
    s = stream(V, "none", 2, W, 1, initial_frames=16, max_workspace_bytes=8 * 2 * (32 * W + 1))
    xd = torch.from_numpy(logits_for(V, "none", 40, 3, True)).cuda()
    first = s.advance([xd[:30], xd[:10]])                   # 16 -> 32 frames for stream 0: fits exactly
    with pytest.raises(MemoryError, match="max_workspace_bytes"):
        s.advance([xd[30:40], None])
    assert list(s.frames_done) == [30, 10] and s._cap_frames == [32, 16]
    again = s.advance([None, None])
    assert [bits(a.hypotheses) for a in again] == [bits(a.hypotheses) for a in first]


# ---- 7: bad frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan", "inf", "neginf_row"])
def test_bad_frame_kills_its_stream_only(torch_mod, bad):
    torch, V, W, nbest = torch_mod, 32, 16, 4
    x0 = logits_for(V, "char3", 50, 70, True).copy()
    x1 = logits_for(V, "char3", 50, 71, True)
    good = x0.copy()
    if bad == "nan":
        x0[25, 7] = np.nan
    elif bad == "inf":
        x0[25, 7] = np.inf
    else:
        x0[25, :] = -np.inf
    ref1 = one_call(torch, V, "char3", x1, W, nbest)
    s = stream(V, "char3", 2, W, nbest)
    d0, d1 = torch.from_numpy(x0).cuda(), torch.from_numpy(x1).cuda()
    stable = None
    for k in range(5):                                       # the bad frame sits in chunk 3 of 5
        st = s.advance([d0[10 * k:10 * k + 10], d1[10 * k:10 * k + 10]])
        if k < 2:
            assert st[0].hypotheses and st[0].hypotheses[0].ids
            stable = st[0].stable_len
        else:
            assert st[0].hypotheses == [] and st[0].stable_len == stable, (k, st[0])
    assert s.advance([None, None], results=False)[0].stable_len == stable
    st = s.advance([None, None])
    assert st[0].hypotheses == [] and st[0].stable_len == stable
    assert bits(st[1].hypotheses) == bits(ref1.hypotheses) and st[1].stable_len == ref1.stable_len
    # reset revives it
    s.reset(0)
    st = s.advance([torch.from_numpy(good).cuda(), None])
    assert bits(st[0].hypotheses) == bits(one_call(torch, V, "char3", good, W, nbest).hypotheses)
    assert bits(st[1].hypotheses) == bits(ref1.hypotheses)


def test_stream_dead_from_its_first_call(torch_mod):
    torch, V = torch_mod, 5
    x = logits_for(V, "none", 12, 1, False).copy()
    x[0, 0] = np.nan
    s = stream(V, "none", 1, 4, 2)
    xd = torch.from_numpy(x).cuda()
    for a in (0, 6):
        st = s.advance([xd[a:a + 6]])[0]
        assert st.hypotheses == [] and st.stable_len == 0


# ---- 8: argument checks of the C entry, and calls without results --------------------------------------------------------------------
def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    V, W, nbest, n = 8, 4, 2, 2
    sb = int(lib.w2v2_ctc_beam_stream_state_bytes())
    assert sb > 0 and sb % 256 == 0
    logits = torch.randn(40, V, device="cuda")
    state = torch.zeros((n, sb), dtype=torch.uint8, device="cuda")
    nodes = torch.zeros(2 * (64 * W + 1), dtype=torch.int64, device="cuda")
    labels = torch.full((n, nbest, 64), -7, dtype=torch.int32, device="cuda")
    length = torch.full((n, nbest), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    stable = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ok = dict(logits=N.ptr(logits), V=V, n=n, row0=[0, 20], frames=[20, 20], done=[0, 0], blank=0, W=W, nbest=nbest, table=None, order=1,
              word=None, delim=0, alpha=0.0, beta=0.0, pen=0.0, eos=0, bias=None, state=N.ptr(state), nodes=N.ptr(nodes),
              node0=[0, 64 * W + 1], cap=[64 * W + 1, 64 * W + 1], max_len=64, labels=N.ptr(labels), length=N.ptr(length),
              score=N.ptr(score), total=N.ptr(total), stable=N.ptr(stable))

    def call(**kw):
        a = dict(ok, **kw)
        row0, frames, done = np.asarray(a["row0"], np.int64), np.asarray(a["frames"], np.int32), np.asarray(a["done"], np.int64)
        node0, cap = np.asarray(a["node0"], np.int64), np.asarray(a["cap"], np.int64)
        rc = lib.w2v2_ctc_beam_search_stream(a["logits"], a["V"], a["n"], N.ptr(row0), N.ptr(frames), N.ptr(done), a["blank"], a["W"],
                                             a["nbest"], a["table"], a["order"], a["word"], a["delim"], a["alpha"], a["beta"], a["pen"],
                                             a["eos"], a["bias"], a["state"], a["nodes"], N.ptr(node0), N.ptr(cap), a["max_len"],
                                             a["labels"], a["length"], a["score"], a["total"], a["stable"], N.current_stream())
        return rc, N.last_error()

    for kw, word in [
        (dict(frames=[20, -1]), "stream 1 is given -1 frames"),
        (dict(done=[-1, 0]), "frames done"),
        (dict(done=[45, 0]), "trie nodes"),                                   # (45 + 20) * 4 + 1 > 64 * 4 + 1
        (dict(cap=[20 * W, 64 * W + 1]), "trie nodes"),                       # one node short
        (dict(done=[(2 ** 31 - 1) // W - 19, 0], cap=[2 ** 40, 2 ** 40], max_len=2 ** 30), "too many frames"),
        (dict(done=[2 ** 31, 0], cap=[2 ** 40, 2 ** 40], max_len=2 ** 30), "too many frames"),
        (dict(done=[30, 0], max_len=49), "max_len"),
        (dict(node0=[-1, 0]), "node offset"),
        (dict(state=None), "null"), (dict(nodes=None), "null"), (dict(stable=None), "null"), (dict(logits=None), "null"),
        (dict(length=None), "null"),
        (dict(V=65), "vocabulary"), (dict(blank=8), "blank"), (dict(W=65), "beam width"), (dict(nbest=5), "nbest"), (dict(n=0), "utterances"),
        (dict(order=5), "order"), (dict(alpha=math.nan), "finite"), (dict(row0=[-1, 20]), "negative offset"),
    ]:
        rc, msg = call(**kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (labels == -7).all() and (stable == -7).all() and (state == 0).all(), "a refused call wrote something"
    # the same call, legal: hypotheses, -1 behind them, and max_len = frames_done + frames exactly is enough
    rc, msg = call(max_len=20, labels=N.ptr(labels))
    assert rc == 0, msg
    rc, msg = call()
    assert rc == 0, msg
    lab, ln = labels.cpu().numpy(), length.cpu().numpy()
    for i in range(n):
        for k in range(nbest):
            assert ln[i, k] >= 0 and (lab[i, k, ln[i, k]:] == -1).all() and (lab[i, k, :ln[i, k]] > 0).all()
    # no labels: only the state moves and stable_len is written; length, score and total may be null
    stable.fill_(-7)
    labels.fill_(-7)
    rc, msg = call(done=[20, 20], row0=[0, 0], frames=[0, 0], labels=None, length=None, score=None, total=None)
    assert rc == 0, msg
    assert (labels == -7).all() and (stable.cpu().numpy() >= 0).all()


@pytest.mark.parametrize("form", ["none", "bias_word"])
def test_call_without_results_then_with(torch_mod, form):
    torch, V, W, nbest = torch_mod, 32, 16, 4
    x = logits_for(V, form, 60, 9, True)
    ref = one_call(torch, V, form, x, W, nbest)
    s = stream(V, form, 1, W, nbest)
    xd = torch.from_numpy(x).cuda()
    st = s.advance([xd[:33]], results=False)[0]
    assert st.hypotheses is None and st.frames_done == 33
    mid = s.advance([None])[0]                               # asking for results does not disturb the state
    assert bits(mid.hypotheses) == bits(one_call(torch, V, form, x[:33], W, nbest).hypotheses) and mid.stable_len == st.stable_len
    st = s.advance([xd[33:]])[0]
    assert bits(st.hypotheses) == bits(ref.hypotheses) and st.stable_len == ref.stable_len


def test_python_raises_before_launching(torch_mod):
    torch = torch_mod
    s = stream(32, "none", 2, 4, 1)
    x = torch.zeros((5, 32), device="cuda")
    with pytest.raises(ValueError, match="2 streams"):
        s.advance([x])
    with pytest.raises(ValueError, match="stream 1"):
        s.advance([x, torch.zeros((5, 31), device="cuda")])
    with pytest.raises(ValueError, match="outside"):
        s.reset(2)
    assert list(s.frames_done) == [0, 0]


# ---- the session ---------------------------------------------------------------------------------------------------------------------
WINDOW, MARGIN = 6400, 640
WINDOW_S, MARGIN_S = WINDOW / 16000.0, MARGIN / 16000.0
HOP = WINDOW - 2 * MARGIN
LENGTHS = [4000, WINDOW, 3 * HOP + WINDOW, 3 * HOP + WINDOW + 1, 2 * HOP + WINDOW + 719]


@pytest.fixture(scope="module")
def session_models(torch_mod):
    import wav2vec2
    from wav2vec2.processor import Wav2Vec2Processor
    out = {}
    for name in ("tiny_base", "tiny_robust"):
        m = wav2vec2.Wav2Vec2ForCTC(H.case_config(name), input_shape=(1, 2048))
        m.set_weights(H.case_weights(name))
        out[name] = m
    return out, Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)


def noise(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def chunk_sizes(kind, n, seed):
    if kind == "random":
        rng = np.random.default_rng(seed)
        sizes = []
        while sum(sizes) < n:
            sizes.append(min(int(rng.integers(1, 9000)), n - sum(sizes)))
        return sizes
    return [min(kind, n - a) for a in range(0, n, kind)]


def offline_rows(m, wave):
    from wav2vec2.longform import predict_long
    return predict_long(m, wave, normalize=True, window=WINDOW, margin=MARGIN)


@functools.lru_cache(maxsize=None)
def _recording(i):
    return noise(400 + i, LENGTHS[i])


@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_session_logits_equal_predict_long(session_models, torch_mod, name):
    models_, tok = session_models
    m = models_[name]
    for i in range(len(LENGTHS)):
        wave = _recording(i)
        want = offline_rows(m, wave).numpy()
        for kind in (1600, 5000, "random"):
            s = m.stream(tok, window_s=WINDOW_S, margin_s=MARGIN_S, keep_logits=True)
            assert (s.window, s.margin) == (WINDOW, MARGIN)
            a = 0
            for c in chunk_sizes(kind, len(wave), 17 * i):
                p = s.feed([wave[a:a + c]])[0]
                a += c
                assert p.frames == s.logits(0).shape[0] <= want.shape[0]
                assert np.array_equal(s.logits(0).cpu().numpy(), want[:p.frames])
            s.finish()
            assert np.array_equal(s.logits(0).cpu().numpy(), want), (name, len(wave), kind)


@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_finish_equals_beam_search_on_predict_long(session_models, torch_mod, name):
    from wav2vec2.decoding import beam_search
    models_, tok = session_models
    m = models_[name]
    blank = m.config.pad_id
    waves = [_recording(2), _recording(4)]
    want = []
    for w in waves:
        h = beam_search([offline_rows(m, w)], beam_width=8, nbest=2, blank=blank)[0]
        want.append(h)
    single = []
    for j, (w, size) in enumerate(zip(waves, (1600, 5000))):
        s = m.stream(tok, window_s=WINDOW_S, margin_s=MARGIN_S, beam_width=8, nbest=2)
        stable = [""]
        for a in range(0, len(w), size):
            p = s.feed(w[a:a + size])[0]
            assert p.stable_text.startswith(stable[-1]) and p.text.startswith(p.stable_text)
            stable.append(p.stable_text)
        t = s.finish()[0]
        assert bits(t.hypotheses) == bits(want[j])
        assert t.text == want[j][0].text(tok) and t.texts == [h.text(tok) for h in want[j]] and t.words is None
        assert all(t.text.startswith(x) for x in stable)
        single.append(t)
    # two streams in one session, in different rhythms
    s = m.stream(tok, n_streams=2, window_s=WINDOW_S, margin_s=MARGIN_S, beam_width=8, nbest=2)
    rng = np.random.default_rng(5)
    pos = [0, 0]
    stable = [[""], [""]]
    while any(p < len(w) for p, w in zip(pos, waves)):
        chunks = []
        for j, w in enumerate(waves):
            c = int(rng.integers(1, 7000)) if j == 0 else 3200
            chunks.append(None if pos[j] >= len(w) or (j == 1 and rng.random() < 0.3) else w[pos[j]:pos[j] + c])
            if chunks[-1] is not None:
                pos[j] += len(chunks[-1])
        for j, p in enumerate(s.feed(chunks)):
            assert p.stable_text.startswith(stable[j][-1])
            stable[j].append(p.stable_text)
    for j, t in enumerate(s.finish()):
        assert bits(t.hypotheses) == bits(single[j].hypotheses) and t.text == single[j].text
        assert all(t.text.startswith(x) for x in stable[j])


def test_session_refusals_and_timestamps(session_models, torch_mod):
    from wav2vec2.alignment import forced_align, token_spans, word_spans
    from wav2vec2.processor import WORD_DELIMITER
    models_, tok = session_models
    m = models_["tiny_base"]
    with pytest.raises(ValueError, match="16 kHz"):
        m.stream(tok, sampling_rate=8000)
    s = m.stream(tok, window_s=WINDOW_S, margin_s=MARGIN_S)
    with pytest.raises(ValueError, match="16 kHz"):
        s.feed([noise(1, 100)], sampling_rate=44100)
    m.set_precision("bf16")
    try:
        with pytest.raises(RuntimeError, match="bf16"):
            m.stream(tok, window_s=WINDOW_S, margin_s=MARGIN_S)
        with pytest.raises(RuntimeError, match="bf16"):         # a session opened in fp32 whose model is switched afterwards
            s.feed([noise(2, 3 * WINDOW)])
    finally:
        m.set_precision("fp32")
    s = m.stream(tok, window_s=WINDOW_S, margin_s=MARGIN_S)
    s.feed([_recording(4)])
    with pytest.raises(ValueError, match="keep_logits"):
        s.finish(timestamps=True)
    s = m.stream(tok, window_s=WINDOW_S, margin_s=MARGIN_S, keep_logits=True)
    s.feed([_recording(4)])
    t = s.finish(timestamps=True)[0]
    tokens = tok.get_vocab()
    vocab = {i: (" " if c == WORD_DELIMITER else c) for c, i in tokens.items()}
    ids = t.hypotheses[0].ids
    assert ids and t.words
    a = forced_align([s.logits(0)], [list(ids)], blank=m.config.pad_id)[0]
    assert t.words == word_spans(token_spans(a), tokens[WORD_DELIMITER], 320 / 16000.0, vocab)
    with pytest.raises(RuntimeError, match="finished"):
        s.feed([noise(3, 10)])
