"""Phrase boosting (contextual biasing) of the CTC prefix beam search on the GPU (w2v2_ctc_beam_search_biased,
wav2vec2.decoding.ContextBias) against the fp64 numpy reference (tests/bias_reference.py), which takes every bias term from the
prefix alone, by brute force over the phrase list.

The fragility rule is tests/test_beam_gpu.py's: an utterance is FRAGILE when the reference's smallest decision margin is below
tau = beam_reference.tau(T, kmax); non-fragile utterances must match the reference in every label, in order, fragile ones in their
scores only, every score within tau, and at most 5 % of a test's utterances may be fragile (tests/test_bias_cpu.py asserts from
the reference alone that none of the utterances used here is)."""

import ctypes
import math
import os

import numpy as np
import pytest

import beam_reference as BR
import bias_reference as B
import helpers as H
import wordlm_reference as WR
from test_beam_gpu import compare, same_bits
from test_beam_gpu import raw_list as raw_list_chars
from test_wordlm_gpu import raw_list as raw_list_words

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")
NEG = -math.inf


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def run(torch, xs, W, nbest, blank, lm, bias):
    from wav2vec2.decoding import beam_search
    return beam_search([torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs], beam_width=W, nbest=nbest, blank=blank, lm=lm,
                       bias=bias)


def lm_args(lm, dev):
    """(table, order, word model struct or None, delim, alpha, beta, unk_penalty, score_eos, what to keep alive) of the C ABI"""
    from wav2vec2 import _native as N
    from wav2vec2.decoding import WordNgramLM
    if isinstance(lm, WordNgramLM):
        st, keep = lm.device_arrays(dev)
        return None, 1, ctypes.byref(st), lm.delimiter, lm.alpha, lm.beta, lm.unk_penalty, int(lm.score_eos), keep
    if lm is not None:
        table = lm.device_table(dev)
        return N.ptr(table), lm.order, None, 0, lm.alpha, lm.beta, 0.0, 0, table
    return None, 1, None, 0, 0.0, 0.0, 0.0, 0, None


def raw(torch, base, row0, lens, W, nbest, blank, lm, bias):
    """the C ABI itself: (labels, length, score, total) on the host"""
    from wav2vec2 import _native as N
    n, V, max_len = len(lens), int(base.shape[1]), max(lens)
    labels = torch.full((n, nbest, max_len), -7, dtype=torch.int32, device="cuda")
    length = torch.full((n, nbest), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    table, order, st, delim, alpha, beta, pen, eos, _keep = lm_args(lm, base.device)
    bst, _keep_bias = bias.device_arrays(base.device)
    N.check(N.load().w2v2_ctc_beam_search_biased(N.ptr(base), V, n, N.ptr(np.asarray(row0, np.int64)), N.ptr(np.asarray(lens, np.int32)),
                                                 blank, W, nbest, table, order, st, delim, alpha, beta, pen, eos, ctypes.byref(bst), max_len,
                                                 N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))
    return labels.cpu().numpy(), length.cpu().numpy(), score.cpu().numpy(), total.cpu().numpy()


def raw_list(torch, xs, W, nbest, blank, lm, bias):
    lens = [x.shape[0] for x in xs]
    out = raw(torch, torch.from_numpy(np.concatenate(xs)).cuda(), np.cumsum([0] + lens[:-1]), lens, W, nbest, blank, lm, bias)
    assert all((out[0][i][:, lens[i]:] == -1).all() for i in range(len(xs)))
    return [(out[0][i][:, :lens[i]], out[1][i], out[2][i], out[3][i]) for i in range(len(xs))]


# ---- 1. random, peaky and phrase-spelling logits against the reference --------------------------------------------------------------
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("vocab", B.VOCABS, ids=lambda v: f"V{v[0]}")
def test_logits_match_reference(torch_mod, vocab, form):
    """84 utterances per case (flat, peaky, spelling bias phrases with noise; T 1, 5, 40, 120; widths 1, 4, 16, 64; nbest 1, 4, 8; a
    bias of 8 phrases and one of about 2 000, whose tables have thousands of rows), 1 008 in all.  The reference alone on these
    seeds: 0 fragile, smallest margin 1.9e-6, largest tau below 1e-9.  Prints its figures before it asserts."""
    V, blank = vocab[0], vocab[1]
    nfrag, ntot, stats, changed = 0, 0, [math.inf, 0.0], 0
    for size in B.SIZES:
        lm, cb, df, sets = B.case_inputs(vocab, form, size)
        rules = B.WordRules(lm) if form.startswith("word") else None
        for W, nbest, xs in sets:
            got = run(torch_mod, xs, W, nbest, blank, lm, cb)
            for g, x in zip(got, xs):
                ref = B.search(x, W, nbest, blank, df, lm, rules)
                nfrag += compare(g, ref, x.shape[0], stats)
                ntot += 1
                changed += bool(g) and g[0].ids != () and cb.score(g[0].ids)[0] != 0.0
    print(f"V={V} {form}: {ntot} utterances, {nfrag} fragile, {changed} best hypotheses with a bonus, min margin {stats[0]:.3g}, "
          f"max score error {stats[1]:.3g}")
    assert nfrag <= 0.05 * ntot
    assert changed >= 4                                      # (the phrase-spelling utterances do earn bonuses)


# ---- 2. a zero-boost bias is the unbiased search, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["none", "char3", "word"])
def test_zero_boost_is_the_unbiased_search(torch_mod, form):
    """labels, lengths, score and total of the biased entry with an all-zero bias of 300 phrases equal those of the existing entry"""
    from wav2vec2.decoding import ContextBias
    vocab = B.VOCABS[1]
    V, blank, delim = vocab[0], vocab[1], vocab[2]
    lm, _, _, _ = B.case_inputs(vocab, form, 8)
    rng = np.random.default_rng(12)
    zero = ContextBias([(h, 0.0) for h, _ in B.random_phrases(rng, V, blank, delim, 300)], V, blank, delim, 1.0, form != "none")
    assert zero.n_states > 500 and not zero.delta.any() and not zero.final.any()
    xs = [WR.make_logits(rng, T, V, blank, pk) for T, pk in [(1, False), (5, True), (40, True), (120, False), (77, True)]]
    if form == "word":
        xs += [WR.word_logits(rng, lm, 4, blank), WR.word_logits(rng, lm, 3, blank, cut=2)]
    for W, nbest in [(1, 1), (16, 8), (64, 4)]:
        plain = raw_list_words(torch_mod, xs, W, nbest, blank, lm) if form == "word" else raw_list_chars(torch_mod, xs, W, nbest, blank, lm)
        for g, r in zip(raw_list(torch_mod, xs, W, nbest, blank, lm, zero), plain):
            same_bits(g, r)


# ---- 3.-5. small examples (tests/test_bias_cpu.py checks what the reference makes of them) --------------------------------------------
def bonus_matches(h, want, ulps=4):
    """total - score against a bonus: two fp64 roundings apart at the most (total = score + fin, then the difference)"""
    return abs((h.total - h.score) - want) <= ulps * 2.0 ** -52 * max(1.0, abs(h.total), abs(h.score))


def test_bias_picks_the_phrase(torch_mod):
    """six frames whose best string `ana` misses the doubled n of `anna`; with the phrase boosted, `anna` comes first"""
    from wav2vec2.decoding import beam_search
    x = B.pick_logits()
    xt = torch_mod.from_numpy(x).cuda()
    (plain,) = beam_search([xt], beam_width=16, nbest=2)
    assert plain[0].ids == (2, 3, 2)
    cb, df = B.make_bias([(B.ANNA, 1.0)], 6, 0)
    (g,) = beam_search([xt], beam_width=16, nbest=2, bias=cb)
    assert g[0].ids == B.ANNA and not compare(g, B.search(x, 16, 2, 0, df), 6, [math.inf, 0.0])
    assert bonus_matches(g[0], cb.score(g[0].ids)[0]) and cb.score(g[0].ids) == (4.0, [(0, 0, 3)])
    assert g[1].total == g[1].score


def test_refund_at_the_end_reorders(torch_mod):
    """the utterance is cut inside `anna`: before the end `an` leads on its credit, the returned order has it second, without any
    bonus; with whole words, the phrase `an` at the very end, with no delimiter frame behind it, gets its bonus"""
    x = B.cut_logits()
    cb, df = B.make_bias([(B.ANNA, 1.0)], 6, 0)
    ref = B.search(x, 8, 4, 0, df)
    assert [p for p, _ in ref.before_final[:2]] == [(2, 3), (2, 5)]
    (g,) = run(torch_mod, [x], 8, 4, 0, None, cb)
    assert not compare(g, ref, 2, [math.inf, 0.0])
    assert [h.ids for h in g[:2]] == [(2, 5), (2, 3)] and bonus_matches(g[1], 0.0)
    cbw, dfw = B.make_bias([((2, 3), 1.0)], 6, 0, 1, 1.0, True)
    (g,) = run(torch_mod, [x], 8, 4, 0, None, cbw)
    assert not compare(g, B.search(x, 8, 4, 0, dfw), 2, [math.inf, 0.0])
    assert g[0].ids == (2, 3) and bonus_matches(g[0], 2.0) and cbw.score((2, 3)) == (2.0, [(0, 0, 1)])


def test_nested_overlapping_and_partial(torch_mod):
    """`annao` with the phrases anna, nn and nao: all three count.  A phrase that needs credit in advance to survive the second frame
    at width 2 is lost with partial = 0 and kept with partial = 1; the reference decides both."""
    x = B.nested_logits()
    cb, df = B.make_bias([(B.ANNA, 1.0), ((3, 3), 0.5), ((3, 2, 4), 0.75)], 6, 0)
    (g,) = run(torch_mod, [x], 8, 2, 0, None, cb)
    assert not compare(g, B.search(x, 8, 2, 0, df), 6, [math.inf, 0.0])
    assert g[0].ids == (2, 3, 3, 2, 4) and bonus_matches(g[0], 7.25) and len(cb.score(g[0].ids)[1]) == 3
    x = B.lookahead_logits()
    got = {}
    for partial in (0.0, 1.0):
        cb, df = B.make_bias([(B.ANNA, 1.0)], 6, 0, None, partial)
        (g,) = run(torch_mod, [x], 2, 2, 0, None, cb)
        assert not compare(g, B.search(x, 2, 2, 0, df), 6, [math.inf, 0.0])
        got[partial] = [h.ids for h in g]
    assert B.ANNA not in got[0.0] and got[1.0][0] == B.ANNA


# ---- 6. isolation, forms, determinism --------------------------------------------------------------------------------------------------
def test_isolation_forms_and_determinism(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import beam_search
    vocab = B.VOCABS[1]
    V, blank = vocab[0], vocab[1]
    for form, W, nbest in [("none", 16, 8), ("word_constrained", 64, 4)]:
        lm, cb, df, _ = B.case_inputs(vocab, form, 2000)
        rng = np.random.default_rng(31)
        xs = [WR.make_logits(rng, 50, V, blank, False), B.phrase_logits(rng, df, V, blank, 2), WR.make_logits(rng, 333, V, blank, True),
              B.phrase_logits(rng, df, V, blank, 9), WR.make_logits(rng, 129, V, blank, True), B.phrase_logits(rng, df, V, blank, 5)]
        Ts = [x.shape[0] for x in xs]
        ref = raw_list(torch, xs, W, nbest, blank, lm, cb)
        for r in ref:
            assert not (r[0] == -7).any() and not (r[1] == -7).any()                        # every output element written
        assert any((r[1] >= 0).any() for r in ref)
        for g, r in zip(raw_list(torch, xs, W, nbest, blank, lm, cb), ref):                  # two calls
            same_bits(g, r)
        xs2 = list(xs)
        xs2[2] = WR.make_logits(rng, Ts[2], V, blank, True)                                  # another neighbour
        for i, (g, r) in enumerate(zip(raw_list(torch, xs2, W, nbest, blank, lm, cb), ref)):
            if i != 2:
                same_bits(g, r)
        perm = [3, 0, 5, 2, 1, 4]
        for g, i in zip(raw_list(torch, [xs[i] for i in perm], W, nbest, blank, lm, cb), perm):
            same_bits(g, ref[i])
        for i, x in enumerate(xs):                                                           # alone
            same_bits(raw_list(torch, [x], W, nbest, blank, lm, cb)[0], ref[i])
        # packed views of one storage read in place, a padded (B, Tmax, V) batch with junk behind each utterance, and a list of copies
        base = torch.from_numpy(np.concatenate(xs)).cuda()
        views = list(torch.split(base, Ts))
        pad = rng.standard_normal((len(Ts), max(Ts), V)).astype(np.float32) * 50
        for b, x in enumerate(xs):
            pad[b, :x.shape[0]] = x
        a = beam_search(torch.from_numpy(pad).cuda(), beam_width=W, nbest=nbest, blank=blank, frame_lengths=Ts, lm=lm, bias=cb)
        b = run(torch, xs, W, nbest, blank, lm, cb)
        c = beam_search(views, beam_width=W, nbest=nbest, blank=blank, lm=lm, bias=cb)
        assert a == b == c
        for hyps, r in zip(a, ref):
            k = int((r[1] >= 0).sum())
            assert [h.score for h in hyps] == r[2][:k].tolist() and [len(h.ids) for h in hyps] == r[1][:k].tolist()


def test_bad_utterances_leave_neighbours_alone(torch_mod):
    vocab = B.VOCABS[1]
    V, blank = vocab[0], vocab[1]
    lm, cb, df, _ = B.case_inputs(vocab, "char3", 2000)
    rng = np.random.default_rng(41)
    xs = [WR.make_logits(rng, T, V, blank, False) for T in (40, 30, 30, 25)] + [B.phrase_logits(rng, df, V, blank, 4)]
    xs[1][7, 13] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][:, 9] = -np.inf                                    # legal: label 9 can never be emitted
    got = raw_list(torch_mod, xs, 16, 4, blank, lm, cb)
    clean = raw_list(torch_mod, [xs[0], xs[4]], 16, 4, blank, lm, cb)
    same_bits(got[0], clean[0])
    same_bits(got[4], clean[1])
    for i in (1, 2):
        lab, length, sc, tot = got[i]
        assert (length == -1).all() and np.isnan(sc).all() and np.isnan(tot).all() and (lab == -1).all()
    hyps = run(torch_mod, xs, 16, 4, blank, lm, cb)
    assert hyps[1] == [] and hyps[2] == []
    stats = [math.inf, 0.0]
    for i in (0, 3, 4):
        assert not compare(hyps[i], B.search(xs[i], 16, 4, blank, df, lm), xs[i].shape[0], stats)
    assert all(9 not in h.ids for h in hyps[3])


def test_no_surviving_hypothesis(torch_mod):
    """constrained word model, one frame that all but forces the letter a: at width 1 the final beam holds `a` alone, an unfinished
    word: no hypothesis, length -1, NaN, with a bias as without; a neighbour is unaffected"""
    from wav2vec2.decoding import beam_search
    lm = WR.two_word_model(unk_penalty=NEG)
    cb, df = B.make_bias([((2, 3), 1.0), ((3, 2), 0.5)], 4, 0, 1, 1.0, True)
    x = np.log(np.array([[0.01, 0.01, 0.97, 0.01]])).astype(np.float32)
    y = WR.pick_logits()
    xs = [torch_mod.from_numpy(v).cuda() for v in (x, y)]
    got = beam_search(xs, beam_width=1, nbest=1, lm=lm, bias=cb)
    assert got[0] == [] and B.search(x, 1, 1, 0, df, lm).hyps == []
    assert got[1] == beam_search(xs[1:], beam_width=1, nbest=1, lm=lm, bias=cb)[0]
    lab, length, sc, tot = raw_list(torch_mod, [x], 1, 1, 0, lm, cb)[0]
    assert length.tolist() == [-1] and np.isnan(sc).all() and np.isnan(tot).all() and (lab == -1).all()
    # width 2: the credit for the first letter of `ba` puts `b` in front of the empty prefix: again nothing; width 3 keeps the empty one
    (g,) = beam_search(xs[:1], beam_width=2, nbest=2, lm=lm, bias=cb)
    assert g == [] == B.search(x, 2, 2, 0, df, lm).hyps
    (g,) = beam_search(xs[:1], beam_width=3, nbest=3, lm=lm, bias=cb)
    assert [h.ids for h in g] == [()] == [k for k, _, _ in B.search(x, 3, 3, 0, df, lm).hyps]
    (g,) = beam_search(xs[1:], beam_width=16, nbest=2, lm=lm, bias=cb)
    assert g[0].ids == (2, 3, 1, 3, 2) and not compare(g, B.search(y, 16, 2, 0, df, lm), 6, [math.inf, 0.0])


# ---- 7. argument checks -----------------------------------------------------------------------------------------------------------------
def test_python_raises_before_launching(torch_mod):
    from wav2vec2.decoding import CharNgramLM, ContextBias, beam_search
    from wav2vec2.longform import decode_long
    cb = ContextBias.from_ids([(2, 3)], 6, 0, delimiter=1)
    x = torch_mod.zeros((2, 5, 6), device="cuda")
    assert len(beam_search(x, beam_width=4, bias=cb)) == 2
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(beam_width=4, nbest=5), dict(blank=2), dict(blank=5), dict(bias="anna"),
               dict(lm=WR.random_model(np.random.default_rng(1), 6, 0, 4, 5, 2)), dict(lm=CharNgramLM(np.zeros((1, 4), np.float32), 1))):
        with pytest.raises(ValueError):
            beam_search(x, **{"bias": cb, **kw})
    with pytest.raises(ValueError, match="vocabulary"):
        beam_search(torch_mod.zeros((1, 3, 8), device="cuda"), bias=cb)
    with pytest.raises(ValueError, match="greedy"):
        decode_long(x[0], beam_width=None, bias=cb)
    cb.next[1, 2] = 99                                       # a corrupted table is caught at the upload
    cb._dev.clear()
    with pytest.raises(ValueError, match="out of range"):
        beam_search(x, beam_width=4, bias=cb)


def test_c_abi_argument_errors(torch_mod):
    """each returns W2V2_EINVAL with its message and leaves the outputs as they were"""
    torch = torch_mod
    from wav2vec2 import _native as N
    from wav2vec2.decoding import CharNgramLM, ContextBias
    lib = N.load()
    dev = torch.device("cuda", 0)
    lm = WR.two_word_model()
    st0, _keep = lm.device_arrays(dev)
    cb = ContextBias.from_ids([(2, 3), (3, 2, 2)], 4, 0, delimiter=1)
    b0, _keep_bias = cb.device_arrays(dev)
    table = CharNgramLM(np.zeros((4, 4), np.float32), 2).device_table(dev)
    x = torch.zeros((4, 8), device="cuda")
    labels = torch.full((1, 2, 4), -7, dtype=torch.int32, device="cuda")
    length = torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
    score = torch.full((1, 2), -7.0, dtype=torch.float64, device="cuda")
    total = torch.full((1, 2), -7.0, dtype=torch.float64, device="cuda")
    row0 = np.zeros(1, np.int64)

    def call(logits=N.ptr(x), V=4, blank=0, W=4, nbest=2, tab=None, order=1, word=False, delim=1, alpha=1.0, beta=0.0, pen=-1.0, max_len=4,
             lab=N.ptr(labels), nobias=False, frames=(4,), wordfields=(), **fields):
        b = N.W2V2CtcBias()
        ctypes.memmove(ctypes.byref(b), ctypes.byref(b0), ctypes.sizeof(b))
        for k, v in fields.items():
            setattr(b, k, v)
        st = N.W2V2WordLM()
        ctypes.memmove(ctypes.byref(st), ctypes.byref(st0), ctypes.sizeof(st))
        for k, v in wordfields:
            setattr(st, k, v)
        fr = np.asarray(frames, np.int32)
        return lib.w2v2_ctc_beam_search_biased(logits, V, 1, N.ptr(row0), N.ptr(fr), blank, W, nbest, tab, order,
                                               ctypes.byref(st) if word else None, delim, alpha, beta, pen, 1,
                                               None if nobias else ctypes.byref(b), max_len, lab, N.ptr(length), N.ptr(score), N.ptr(total),
                                               N.current_stream())

    for kw, msg in [(dict(nobias=True), "null bias"), (dict(next=None), "null bias array"), (dict(delta=None), "null bias array"),
                    (dict(final=None), "null bias array"), (dict(n_states=0), "bias states"), (dict(n_states=(1 << 20) + 1), "bias states"),
                    (dict(start_state=-1), "bias start state"), (dict(start_state=cb.n_states), "bias start state"),
                    (dict(n_states=1 << 20, V=2048), "31 bits"), (dict(word=True, tab=N.ptr(table)), "both"),
                    # the checks of the character form's entry
                    (dict(logits=None), "null"), (dict(lab=None), "null"), (dict(frames=(0,)), "frames"), (dict(blank=4), "blank"),
                    (dict(W=0), "beam width"), (dict(W=65), "beam width"), (dict(nbest=0), "nbest"), (dict(V=65), "vocabulary"),
                    (dict(max_len=3), "max_len"), (dict(order=0), "order"), (dict(tab=N.ptr(table), order=5), "order"),
                    (dict(alpha=float("nan")), "finite"),
                    # and of the word form's
                    (dict(word=True, delim=0), "delimiter"), (dict(word=True, delim=4), "delimiter"), (dict(word=True, pen=0.5), "unk_penalty"),
                    (dict(word=True, wordfields=(("child", None),)), "null language model array"),
                    (dict(word=True, wordfields=(("order", 6),)), "order"), (dict(word=True, wordfields=(("unk", -1),)), "unk"),
                    (dict(word=True, W=65), "beam width"), (dict(word=True, beta=float("inf")), "finite")]:
        assert call(**kw) == -1, kw                          # W2V2_EINVAL
        assert msg in N.last_error(), (kw, N.last_error())
    torch.cuda.synchronize()
    assert (labels == -7).all() and (length == -7).all() and (score == -7.0).all() and (total == -7.0).all()
    assert call() == 0 and call(word=True) == 0 and call(word=True, pen=NEG) == 0 and call(tab=N.ptr(table), order=2) == 0
    assert call(word=True, delim=9) != 0 and call(delim=9) == 0          # delim is ignored without a word model
    torch.cuda.synchronize()
    assert not (length == -7).any()


# ---- 8. model level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_model_transcribe(torch_mod, name):
    import wav2vec2
    from wav2vec2.decoding import ContextBias, beam_search
    from wav2vec2.longform import decode_long
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 52345, 24000)]
    logits = m.predict_packed(waves)
    # phrases out of what the model says without a bias (second hypotheses, so that the bias has something to change), and two texts
    plain = m.transcribe(waves, tok, beam_width=8, nbest=4)
    phrases = [(h.ids[:k], 1.5) for tr in plain for h in tr.hypotheses[1:3] for k in (2, 4) if len(h.ids) >= k]
    assert len(phrases) >= 4
    b = ContextBias.from_ids(phrases, cfg.vocab_size, cfg.pad_id)
    df = B.Definition(phrases, cfg.vocab_size, cfg.pad_id)
    out = m.transcribe(waves, tok, beam_width=8, nbest=4, bias=b)
    direct = beam_search(logits, beam_width=8, nbest=4, blank=cfg.pad_id, bias=b)
    assert [tr.hypotheses for tr in out] == direct
    assert [tr.hypotheses for tr in out] != [tr.hypotheses for tr in plain]
    nfrag = 0
    for tr, l in zip(out, logits):
        h = l.cpu().numpy()
        nfrag += compare(tr.hypotheses, B.search(h, 8, 4, cfg.pad_id, df), h.shape[0], [math.inf, 0.0])
        assert tr.texts == [x.text(tok) for x in tr.hypotheses] and tr.text == tr.texts[0]
    assert nfrag <= 1
    words = ContextBias.from_phrases(["the dog", ("fox", 3.0)], tok)
    assert [tr.hypotheses for tr in m.transcribe(waves, tok, beam_width=8, nbest=4, bias=words)] == \
        beam_search(logits, beam_width=8, nbest=4, blank=cfg.pad_id, bias=words)
    with pytest.raises(ValueError, match="greedy"):
        m.transcribe(waves, tok, beam_width=None, bias=b)
    ev = m.evaluate(waves, ["the dog", "a fox", "the fox is a dog", "dog"], tok, beam_width=8, nbest=4, bias=b)
    assert [tr.hypotheses for tr in ev.transcripts] == direct and ev.wer.rate >= 0
    # long form: every segment restarts the bias
    rec = [rng.standard_normal(9000).astype(np.float32), rng.standard_normal(14000).astype(np.float32)]
    kw = dict(window_s=0.4, margin_s=0.04)
    got = m.transcribe_long(rec, tok, beam_width=4, nbest=2, bias=b, **kw)
    ref = decode_long(m.predict_long(rec, 0.4, 0.04), tok, beam_width=4, nbest=2, blank=cfg.pad_id, seconds_per_frame=320 / 16000.0, bias=b)
    assert len(got) == 2 and got == ref
    assert m.evaluate_long(rec, ["the dog", "a fox"], tok, beam_width=4, nbest=2, bias=b, **kw).wer.rate >= 0
