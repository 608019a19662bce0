"""CTC prefix beam search with a word n-gram language model and a lexicon on the GPU (w2v2_ctc_beam_search_words,
wav2vec2.decoding.WordNgramLM) against the fp64 numpy reference (tests/wordlm_reference.py), which scores every prefix from
scratch out of the n-gram dictionary.

The fragility rule is tests/test_beam_gpu.py's: an utterance is FRAGILE when the reference's smallest decision margin is below
tau = beam_reference.tau(T, kmax); non-fragile utterances must match the reference in every label, in order, fragile ones in their
scores only, every score within tau, and at most 5 % of a test's utterances may be fragile (tests/test_wordlm_cpu.py asserts from
the reference alone that none of the utterances used here is)."""

import ctypes
import math
import os

import numpy as np
import pytest

import beam_reference as BR
import helpers as H
import wordlm_reference as WR
from test_beam_gpu import compare, same_bits

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")
NEG = -math.inf


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def run(torch, xs, W, nbest, blank, lm):
    from wav2vec2.decoding import beam_search
    return beam_search([torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs], beam_width=W, nbest=nbest, blank=blank, lm=lm)


def words_of(ids, delim):
    out, cur = [], []
    for c in tuple(ids) + (delim,):
        if c == delim:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    return out


# ---- random, peaky and word-spelling logits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("V,blank,delim,nwords,order", WR.CASES)
def test_logits_match_reference(torch_mod, V, blank, delim, nwords, order, constrained):
    """48 utterances per case (flat, peaky, spelling lexicon words with noise; widths 1, 4, 16, 64, nbest 1, 4, 8), 480 in all.  The
    reference alone on these seeds: 0 fragile, smallest margin 1.3e-5, largest tau 2.3e-10, 4 constrained utterances without a
    hypothesis.  In constrained mode every word of every returned hypothesis is a lexicon word.  Prints its figures before it
    asserts."""
    lm, sets = WR.case_inputs(V, blank, delim, nwords, order, constrained)
    sc = WR.Scorer(lm)
    spellings = set(lm.lexicon.values())
    nfrag, ntot, stats, nohyp = 0, 0, [math.inf, 0.0], 0
    for W, nbest, xs in sets:
        got = run(torch_mod, xs, W, nbest, blank, lm)
        for g, x in zip(got, xs):
            nfrag += compare(g, WR.search(x, W, nbest, blank, lm, sc), x.shape[0], stats)
            ntot += 1
            nohyp += not g
            if constrained:
                assert all(w in spellings for h in g for w in words_of(h.ids, delim)), g
    print(f"V={V} blank={blank} order={order} constrained={constrained}: {ntot} utterances, {nfrag} fragile, {nohyp} without a "
          f"hypothesis, min margin {stats[0]:.3g}, max score error {stats[1]:.3g}")
    assert nfrag <= 0.05 * ntot


# ---- small examples -------------------------------------------------------------------------------------------------------------------
def test_lm_picks_the_word(torch_mod):
    """without a language model the best string is `a|ba` (a is no word); with the lexicon it is `ab|ba`, open and constrained"""
    from wav2vec2.decoding import beam_search
    x = WR.pick_logits()
    xt = torch_mod.from_numpy(x).cuda()
    (plain,) = beam_search([xt], beam_width=16, nbest=1)
    assert plain[0].ids == (2, 1, 3, 2)
    for kw in (dict(unk_penalty=-3.0), dict(unk_penalty=NEG)):
        lm = WR.two_word_model(alpha=1.0, beta=0.0, **kw)
        (g,) = beam_search([xt], beam_width=16, nbest=2, lm=lm)
        ref = WR.search(x, 16, 2, 0, lm)
        assert g[0].ids == (2, 3, 1, 3, 2)
        assert not compare(g, ref, 6, [math.inf, 0.0])


def test_utterance_ends_inside_a_word(torch_mod):
    """the last word is cut: open mode scores what is left as <unk>; constrained mode keeps only hypotheses that end on a whole word
    (or has none); either way the reference's list"""
    rng = np.random.default_rng(77)
    for constrained in (False, True):
        lm = WR.random_model(rng, 32, 0, 4, 60, 2, maxlen=5, alpha=0.7, beta=0.1, unk_penalty=NEG if constrained else -1.5)
        xs = [WR.word_logits(rng, lm, 3, 0, cut=cut) for cut in (2, 3, 4, 5)]
        sc = WR.Scorer(lm)
        stats = [math.inf, 0.0]
        for g, x in zip(run(torch_mod, xs, 16, 4, 0, lm), xs):
            ref = WR.search(x, 16, 4, 0, lm, sc)
            assert not compare(g, ref, x.shape[0], stats)
            assert len(g) == len(ref.hyps)


def test_no_surviving_hypothesis(torch_mod):
    """constrained, one frame that all but forces the letter a: the final beam holds `a` (an unfinished word, removed) and the empty
    prefix at width 2 -- and `a` alone at width 1: no hypothesis, length -1, NaN; a neighbour is unaffected"""
    from wav2vec2.decoding import beam_search
    lm = WR.two_word_model(unk_penalty=NEG)
    x = np.log(np.array([[0.01, 0.01, 0.97, 0.01]])).astype(np.float32)
    y = WR.pick_logits()
    xs = [torch_mod.from_numpy(v).cuda() for v in (x, y)]
    got = beam_search(xs, beam_width=1, nbest=1, lm=lm)
    assert got[0] == [] and WR.search(x, 1, 1, 0, lm).hyps == []
    assert got[1] == beam_search(xs[1:], beam_width=1, nbest=1, lm=lm)[0]
    (g,) = beam_search(xs[:1], beam_width=2, nbest=2, lm=lm)
    assert [h.ids for h in g] == [()] == [k for k, _, _ in WR.search(x, 2, 2, 0, lm).hyps]


# ---- isolation, forms, determinism ------------------------------------------------------------------------------------------------------
def raw(torch, base, row0, lens, W, nbest, blank, lm, **over):
    """the C ABI itself: (labels, length, score, total) on the host"""
    from wav2vec2 import _native as N
    n, V, max_len = len(lens), int(base.shape[1]), max(lens)
    labels = torch.full((n, nbest, max_len), -7, dtype=torch.int32, device="cuda")
    length = torch.full((n, nbest), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    st, _keep = lm.device_arrays(base.device)
    lib = N.load()
    N.check(lib.w2v2_ctc_beam_search_words(N.ptr(base), V, n, N.ptr(np.asarray(row0, np.int64)), N.ptr(np.asarray(lens, np.int32)), blank,
                                           W, nbest, ctypes.byref(st), lm.delimiter, lm.alpha, lm.beta, lm.unk_penalty,
                                           int(lm.score_eos), max_len, N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total),
                                           N.current_stream()))
    return labels.cpu().numpy(), length.cpu().numpy(), score.cpu().numpy(), total.cpu().numpy()


def raw_list(torch, xs, W, nbest, blank, lm):
    lens = [x.shape[0] for x in xs]
    out = raw(torch, torch.from_numpy(np.concatenate(xs)).cuda(), np.cumsum([0] + lens[:-1]), lens, W, nbest, blank, lm)
    assert all((out[0][i][:, lens[i]:] == -1).all() for i in range(len(xs)))
    return [(out[0][i][:, :lens[i]], out[1][i], out[2][i], out[3][i]) for i in range(len(xs))]


def test_isolation_forms_and_determinism(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import beam_search
    rng = np.random.default_rng(31)
    for constrained, W, nbest in [(False, 16, 8), (True, 64, 4)]:
        lm = WR.random_model(rng, 32, 0, 4, 150, 3, alpha=0.5, beta=0.1, unk_penalty=NEG if constrained else -2.0)
        xs = [WR.make_logits(rng, 50, 32, 0, False), WR.word_logits(rng, lm, 2, 0), WR.make_logits(rng, 333, 32, 0, True),
              WR.word_logits(rng, lm, 12, 0), WR.make_logits(rng, 129, 32, 0, True), WR.word_logits(rng, lm, 7, 0)]
        Ts = [x.shape[0] for x in xs]
        ref = raw_list(torch, xs, W, nbest, 0, lm)
        for r in ref:
            assert not (r[0] == -7).any() and not (r[1] == -7).any()                        # every output element written
        assert any((r[1] >= 0).any() for r in ref)
        for g, r in zip(raw_list(torch, xs, W, nbest, 0, lm), ref):                          # two calls
            same_bits(g, r)
        xs2 = list(xs)
        xs2[2] = WR.make_logits(rng, Ts[2], 32, 0, True)                                     # another neighbour
        for i, (g, r) in enumerate(zip(raw_list(torch, xs2, W, nbest, 0, lm), ref)):
            if i != 2:
                same_bits(g, r)
        perm = [3, 0, 5, 2, 1, 4]
        for g, i in zip(raw_list(torch, [xs[i] for i in perm], W, nbest, 0, lm), perm):
            same_bits(g, ref[i])
        for i, x in enumerate(xs):                                                           # alone
            same_bits(raw_list(torch, [x], W, nbest, 0, lm)[0], ref[i])
        # packed views of one storage read in place, a padded (B, Tmax, V) batch with junk behind each utterance, and a list of copies
        base = torch.from_numpy(np.concatenate(xs)).cuda()
        views = list(torch.split(base, Ts))
        Tm = max(Ts)
        pad = rng.standard_normal((len(Ts), Tm, 32)).astype(np.float32) * 50
        for b, x in enumerate(xs):
            pad[b, :x.shape[0]] = x
        a = beam_search(torch.from_numpy(pad).cuda(), beam_width=W, nbest=nbest, frame_lengths=Ts, lm=lm)
        b = run(torch, xs, W, nbest, 0, lm)
        c = beam_search(views, beam_width=W, nbest=nbest, lm=lm)
        assert a == b == c
        for hyps, r in zip(a, ref):
            k = int((r[1] >= 0).sum())
            assert [h.score for h in hyps] == r[2][:k].tolist() and [len(h.ids) for h in hyps] == r[1][:k].tolist()


def test_bad_utterances_leave_neighbours_alone(torch_mod):
    rng = np.random.default_rng(41)
    lm = WR.random_model(rng, 32, 0, 4, 100, 2, alpha=0.6, beta=0.2, unk_penalty=-2.0)
    xs = [WR.make_logits(rng, T, 32, 0, False) for T in (40, 30, 30, 25)] + [WR.word_logits(rng, lm, 4, 0)]
    xs[1][7, 13] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][:, 9] = -np.inf                                    # legal: label 9 can never be emitted
    got = raw_list(torch_mod, xs, 16, 4, 0, lm)
    clean = raw_list(torch_mod, [xs[0], xs[4]], 16, 4, 0, lm)
    same_bits(got[0], clean[0])
    same_bits(got[4], clean[1])
    for i in (1, 2):
        lab, length, sc, tot = got[i]
        assert (length == -1).all() and np.isnan(sc).all() and np.isnan(tot).all() and (lab == -1).all()
    hyps = run(torch_mod, xs, 16, 4, 0, lm)
    assert hyps[1] == [] and hyps[2] == []
    stats = [math.inf, 0.0]
    for i in (0, 3, 4):
        assert not compare(hyps[i], WR.search(xs[i], 16, 4, 0, lm), xs[i].shape[0], stats)
    assert all(9 not in h.ids for h in hyps[3])


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def test_python_raises_before_launching(torch_mod):
    from wav2vec2.decoding import beam_search
    lm = WR.two_word_model()
    x = torch_mod.zeros((2, 5, 4), device="cuda")
    assert len(beam_search(x, beam_width=4, lm=lm)) == 2
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(beam_width=4, nbest=5), dict(blank=1), dict(blank=2), dict(blank=4)):
        with pytest.raises(ValueError):
            beam_search(x, lm=lm, **kw)
    with pytest.raises(ValueError, match="vocabulary"):
        beam_search(torch_mod.zeros((1, 3, 8), device="cuda"), lm=lm)
    with pytest.raises(ValueError, match="CharNgramLM or a WordNgramLM"):
        beam_search(x, lm="arpa")
    lm.arc_word[1], lm.arc_word[2] = lm.arc_word[2], lm.arc_word[1]      # a corrupted model is caught at the upload
    lm._dev.clear()
    with pytest.raises(ValueError, match="state 0|sorted"):
        beam_search(x, beam_width=4, lm=lm)


def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    lm = WR.two_word_model()
    st0, _keep = lm.device_arrays(torch.device("cuda", 0))
    x = torch.zeros((4, 8), device="cuda")
    labels = torch.empty((1, 2, 4), dtype=torch.int32, device="cuda")
    length = torch.empty((1, 2), dtype=torch.int32, device="cuda")
    score = torch.empty((1, 2), dtype=torch.float64, device="cuda")
    total = torch.empty((1, 2), dtype=torch.float64, device="cuda")
    row0 = np.zeros(1, np.int64)

    def call(logits=N.ptr(x), V=4, blank=0, W=4, nbest=2, delim=1, alpha=1.0, beta=0.0, pen=-1.0, max_len=4, lab=N.ptr(labels),
             nolm=False, **fields):
        st = N.W2V2WordLM()
        ctypes.memmove(ctypes.byref(st), ctypes.byref(st0), ctypes.sizeof(st))
        for k, v in fields.items():
            setattr(st, k, v)
        fr = np.asarray([4], np.int32)
        return lib.w2v2_ctc_beam_search_words(logits, V, 1, N.ptr(row0), N.ptr(fr), blank, W, nbest, None if nolm else ctypes.byref(st),
                                              delim, alpha, beta, pen, 1, max_len, lab, N.ptr(length), N.ptr(score), N.ptr(total),
                                              N.current_stream())

    assert call() == 0
    assert call(pen=NEG) == 0
    torch.cuda.synchronize()
    for kw, msg in [(dict(logits=None), "null"), (dict(lab=None), "null"), (dict(nolm=True), "null"), (dict(child=None), "null"),
                    (dict(bstate=None), "null"), (dict(arc_logp=None), "null"), (dict(delim=0), "delimiter"), (dict(delim=4), "delimiter"),
                    (dict(delim=-1), "delimiter"), (dict(n_nodes=0), "sizes"), (dict(n_states=0), "sizes"), (dict(n_arcs=-1), "sizes"),
                    (dict(n_words=0), "sizes"), (dict(order=0), "order"), (dict(order=6), "order"), (dict(alpha=float("nan")), "finite"),
                    (dict(beta=float("inf")), "finite"), (dict(pen=float("nan")), "unk_penalty"), (dict(pen=0.5), "unk_penalty"),
                    (dict(start_state=99), "start state"), (dict(start_state=-1), "start state"), (dict(unk=-1), "unk"),
                    (dict(unk=99), "unk"), (dict(eos=99), "eos"), (dict(n_nodes=2 ** 30), "31 bits"), (dict(W=65), "beam width"),
                    (dict(V=65), "vocabulary"), (dict(blank=4), "blank"), (dict(nbest=0), "nbest"), (dict(max_len=3), "max_len")]:
        assert call(**kw) != 0, kw
        assert msg in N.last_error(), (kw, N.last_error())
    torch.cuda.synchronize()


# ---- model level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_model_transcribe(torch_mod, name):
    import wav2vec2
    from wav2vec2.decoding import WordNgramLM
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 52345, 24000)]
    hosts = [l.cpu().numpy() for l in m.predict_packed(waves)]
    texts = ["the quick brown fox", "jumps over the lazy dog", "the dog jumps", "a fox is a dog"]
    nfrag = ntot = 0
    for kw, unk_penalty in ((dict(beam_width=16, nbest=4), -4.0), (dict(beam_width=64, nbest=1), -1.0), (dict(beam_width=16, nbest=2), NEG)):
        lm = WordNgramLM.from_text(texts, tok, order=3, alpha=0.6, beta=0.2, unk_penalty=unk_penalty)
        sc = WR.Scorer(lm)
        out = m.transcribe(waves, tok, lm=lm, **kw)
        for tr, h in zip(out, hosts):
            ref = WR.search(h, kw["beam_width"], kw["nbest"], cfg.pad_id, lm, sc)
            fragile = ref.margin < BR.tau(h.shape[0], ref.kmax)
            nfrag += fragile
            ntot += 1
            assert tr.words is None and tr.texts == [x.text(tok) for x in tr.hypotheses]
            assert tr.text == (tr.texts[0] if tr.texts else "")
            assert len(tr.hypotheses) == len(ref.hyps)
            if not fragile:
                assert [x.ids for x in tr.hypotheses] == [k for k, _, _ in ref.hyps]
                for x, (k, s, tot) in zip(tr.hypotheses, ref.hyps):
                    t = BR.tau(h.shape[0], ref.kmax)
                    assert abs(x.score - s) <= t and abs(x.total - tot) <= t
        stamped = m.transcribe(waves, tok, lm=lm, timestamps=True, **kw)
        for tr, plain in zip(stamped, out):
            assert tr.hypotheses == plain.hypotheses and tr.text == plain.text
            want = [w for w in tr.text.split(" ") if w] if tr.hypotheses else []
            assert [w.text for w in tr.words] == want
    print(f"{name}: {nfrag} of {ntot} fragile")
    assert nfrag <= 0.05 * ntot
