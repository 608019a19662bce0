"""Phrase boosting of the CTC beam search on the host (wav2vec2.decoding.ContextBias; tests/bias_reference.py): the compiled
automaton against the brute-force definition, the sum of the table values along a prefix, ``score`` and its matches, the reference
search against every frame path and against the unbiased references, every ValueError, and the share of fragile utterances among
the inputs of tests/test_bias_gpu.py."""

import math
import os

import numpy as np
import pytest

import beam_reference as BR
import bias_reference as B
import wordlm_reference as WR
from wav2vec2.decoding import CharNgramLM, ContextBias, _check_args
from wav2vec2.processor import Wav2Vec2Processor

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")
NEG = -math.inf


def tok():
    return Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)


def state_ids(cb, df):
    """{state string: state number}: every phrase prefix walked from the root"""
    ids = {}
    for s in df.prefixes:
        k = 0
        for c in s:
            k = int(cb.next[k, c])
        ids[s] = k
    return ids


# ---- the automaton against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("V,blank,delim,n", [(6, 0, 1, 12), (6, 5, 1, 40), (32, 31, 4, 60), (32, 0, 4, 300)])
def test_tables_equal_the_definition(V, blank, delim, n, whole):
    """random phrase sets with a one-label phrase, a doubled label, a phrase nested in another and one whose suffix is another's
    prefix (bias_reference.random_phrases): for every state string and every label, `next` is the brute-force longest suffix and
    `delta` / `final` are the fp32 roundings of the definition"""
    rng = np.random.default_rng(10 * V + n + whole)
    for partial in (1.0, 0.5, 0.0, 0.3):
        phrases = B.random_phrases(rng, V, blank, delim, n, maxlen=5, words=whole)
        cb, df = B.make_bias(phrases, V, blank, delim, partial, whole)
        ids = state_ids(cb, df)
        assert len(set(ids.values())) == len(ids) == cb.n_states and ids[()] == 0
        assert cb.start_state == ids[df.state(())]
        for s, k in ids.items():
            for c in range(V):
                if c == blank:
                    assert cb.next[k, c] == k and cb.delta[k, c] == 0
                    continue
                assert cb.next[k, c] == ids[df.state_of(s + (c,))], (s, c)
                assert float(cb.delta[k, c]) == df.delta(s, c), (s, c)
            assert float(cb.final[k]) == df.final(s), s
        cb.validate()


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("V,blank,delim", [(6, 0, 1), (32, 31, 4)])
def test_sum_along_a_prefix_is_the_completed_bonus(V, blank, delim, whole):
    """boosts are multiples of 0.25 and partial is 1, 0.5 or 0, so every term is exact in fp32: for 2 000 random prefixes of up to
    16 labels the fp64 sum of the table values along the prefix plus `final` EQUALS C(p) -- with whole_words, C of the prefix with
    the end counted as a delimiter.  The partial credits cancel exactly."""
    rng = np.random.default_rng(5 + V + whole)
    labels = [c for c in range(V) if c != blank]
    nonzero = 0
    for partial in (1.0, 0.5, 0.0):
        phrases = B.random_phrases(rng, V, blank, delim, 30, maxlen=4, words=whole)
        cb, df = B.make_bias(phrases, V, blank, delim, partial, whole)
        few = [c for h, _ in phrases[:6] for c in h] + [delim]
        for trial in range(667):
            pool = few if trial % 2 else labels                # (half of the prefixes over the phrases' own letters, so that phrases occur)
            p = tuple(int(c) for c in rng.choice(pool, int(rng.integers(0, 17))))
            s, acc = cb.start_state, 0.0
            for c in p:
                acc = acc + float(cb.delta[s, c])
                s = int(cb.next[s, c])
            want = df.completed(p, at_end=True)
            assert acc + float(cb.final[s]) == want, (p, partial)
            assert cb.score(p)[0] == want and cb.score(p)[1] == df.matches(p)
            nonzero += want > 0
    assert nonzero > 100                                     # (the inputs do exercise phrases: a prefix in 20 at the least earns a bonus)


# ---- score and matches, by hand ------------------------------------------------------------------------------------------------------
def test_score_and_matches_by_hand():
    t = tok()
    ids = tuple(t("ANNA KARENINA"))
    assert len(ids) == 13
    cb = ContextBias.from_phrases(["Anna", ("karenina", 1.5)], t)
    assert cb.whole_words and cb.delimiter == ids[4] and cb.start_state == cb.next[0, cb.delimiter]
    assert cb.score(ids) == (2.0 * 4 + 1.5 * 8, [(0, 0, 3), (1, 5, 12)])
    assert cb.score(ids[:4]) == (8.0, [(0, 0, 3)])                       # the end of the utterance closes the word
    assert cb.score(ids[:3]) == (0.0, [])
    assert cb.score(tuple(t("JOANNA KARENINAS"))) == (0.0, [])           # whole words only
    both = ContextBias.from_phrases(["anna karenina", "ANNA"], t, boost=1.0)
    assert both.score(ids) == (13.0 + 4.0, [(1, 0, 3), (0, 0, 12)])      # the delimiter between the words is counted; nested: both
    # ANNOUNCE against ANNA: three labels of credit, given back at the O
    inner = ContextBias.from_phrases(["ANNA"], t, boost=2.0, whole_words=False)
    a = tuple(t("ANNOUNCE"))
    s, acc, trace = inner.start_state, 0.0, []
    for c in a:
        acc += float(inner.delta[s, c])
        s = int(inner.next[s, c])
        trace.append(acc)
    assert trace == [2.0, 4.0, 6.0, 0.0, 0.0, 0.0, 0.0, 0.0] and inner.score(a) == (0.0, [])
    assert inner.score(tuple(t("ANN"))) == (0.0, [])                    # the end of the utterance takes the credit back as well
    assert inner.score(tuple(t("JOANNA ANNAS"))) == (16.0, [(0, 2, 5), (0, 7, 10)])
    half = ContextBias.from_phrases(["ANNA"], t, boost=2.0, partial=0.5, whole_words=False)
    assert [float(half.delta[k, c]) for k, c in zip([0, 1, 2, 3], a[:3] + (a[0],))] == [1.0, 1.0, 1.0, 5.0]


# ---- the reference search ------------------------------------------------------------------------------------------------------------
def bias_of(df, p, final=True):
    """the fp64 sum of the definition's fp32 terms along the transcript p"""
    acc, s = 0.0, df.state(())
    for c in p:
        acc = acc + df.delta(s, c)
        s = df.state_of(s + (c,))
    return acc + df.final(s) if final else acc


@pytest.mark.parametrize("whole", [False, True])
def test_reference_equals_brute_force(whole):
    """V = 4, T = 1 .. 5, a beam wide enough that nothing is pruned, no language model: every transcript of every frame path, its
    exact score plus the bias of the transcript, in rank order"""
    rng = np.random.default_rng(17 + whole)
    for T in (1, 2, 3, 4, 5):
        phrases = B.random_phrases(rng, 4, 0, 1, 6, maxlen=3, words=whole)
        cb, df = B.make_bias(phrases, 4, 0, 1, 0.5 if T % 2 else 1.0, whole)
        x = WR.make_logits(rng, T, 4, 0, T > 2)
        want = sorted(((k, s, s + bias_of(df, k)) for k, s, _ in BR.brute_force(x, 0)), key=lambda z: -z[2])
        got = B.search(x, 1000, len(want), 0, df)
        assert [k for k, _, _ in got.hyps] == [k for k, _, _ in want]
        for (k, s, tot), (_, s2, tot2) in zip(got.hyps, want):
            assert abs(s - s2) < 1e-12 and abs(tot - tot2) < 1e-12


def test_zero_boost_reference_is_the_unbiased_reference():
    rng = np.random.default_rng(23)
    lm = CharNgramLM(np.log(rng.dirichlet(np.ones(6), 36)).astype(np.float32), 3, alpha=0.8, beta=-0.2)
    wlm = WR.random_model(rng, 6, 0, 1, 12, 2, alpha=0.8, beta=0.3, unk_penalty=-2.0)
    cb, df = B.make_bias([(h, 0.0) for h, _ in B.random_phrases(rng, 6, 0, 1, 20)], 6, 0, 1, 1.0, True)
    assert not cb.delta.any() and not cb.final.any()
    for T in (1, 7, 40):
        x = WR.make_logits(rng, T, 6, 0, True)
        assert B.search(x, 4, 4, 0, df).hyps == BR.search(x, 4, 4, 0).hyps
        assert B.search(x, 4, 4, 0, df, lm).hyps == BR.search(x, 4, 4, 0, lm.table, 3, lm.alpha, lm.beta).hyps
        assert B.search(x, 4, 4, 0, df, wlm).hyps == WR.search(x, 4, 4, 0, wlm).hyps


def test_worked_examples():
    """what tests/test_bias_gpu.py expects of its hand-made logits, from the reference alone; none of them fragile"""
    def solid(r, T):
        assert r.margin >= 1e3 * BR.tau(T, r.kmax)
        return [k for k, _, _ in r.hyps]

    cb, df = B.make_bias([(B.ANNA, 1.0)], 6, 0)
    x = B.pick_logits()
    assert solid(BR.search(x, 16, 2), 6)[0] == (2, 3, 2)
    r = B.search(x, 16, 2, 0, df)
    assert solid(r, 6) == [B.ANNA, (2, 3, 2)] and abs((r.hyps[0][2] - r.hyps[0][1]) - cb.score(B.ANNA)[0]) < 1e-12
    r = B.search(B.cut_logits(), 8, 4, 0, df)                            # the refund at the end re-orders
    assert [p for p, _ in r.before_final[:2]] == [(2, 3), (2, 5)] and solid(r, 2)[:2] == [(2, 5), (2, 3)]
    assert r.hyps[1][2] == r.hyps[1][1]
    cbw, dfw = B.make_bias([((2, 3), 1.0)], 6, 0, 1, 1.0, True)          # whole words: the end of the utterance closes the word
    r = B.search(B.cut_logits(), 8, 4, 0, dfw)
    assert solid(r, 2)[0] == (2, 3) and abs((r.hyps[0][2] - r.hyps[0][1]) - 2.0) < 1e-12 and cbw.score((2, 3)) == (2.0, [(0, 0, 1)])
    cb3, df3 = B.make_bias([(B.ANNA, 1.0), ((3, 3), 0.5), ((3, 2, 4), 0.75)], 6, 0)
    r = B.search(B.nested_logits(), 8, 2, 0, df3)
    assert solid(r, 6)[0] == (2, 3, 3, 2, 4) and cb3.score(r.hyps[0][0]) == (4.0 + 1.0 + 2.25, [(1, 1, 2), (0, 0, 3), (2, 2, 4)])
    assert abs((r.hyps[0][2] - r.hyps[0][1]) - 7.25) < 1e-12
    lost = solid(B.search(B.lookahead_logits(), 2, 2, 0, B.make_bias([(B.ANNA, 1.0)], 6, 0, None, 0.0)[1]), 6)
    kept = solid(B.search(B.lookahead_logits(), 2, 2, 0, B.make_bias([(B.ANNA, 1.0)], 6, 0, None, 1.0)[1]), 6)
    assert B.ANNA not in lost and kept[0] == B.ANNA


# ---- the GPU tests' inputs: the share of fragile utterances, from the reference alone -------------------------------------------------
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("vocab", B.VOCABS, ids=lambda v: f"V{v[0]}")
def test_gpu_inputs_are_not_fragile(vocab, form):
    """tests/test_bias_gpu.py compares labels only where the reference's smallest decision margin is at least tau (the rule of
    tests/test_beam_gpu.py with beam_reference.tau) and lets at most 5 % of a test's utterances fall below.  On its seeds: 84
    utterances per case (a bias of 8 and one of about 2 000 phrases), 1 008 in all, none fragile; smallest margin 1.9e-6, largest
    tau below 1e-9."""
    tot = frag = 0
    mm, tm = math.inf, 0.0
    for size in B.SIZES:
        lm, cb, df, sets = B.case_inputs(vocab, form, size)
        assert cb.n_states > (1000 if size > 100 else 8)
        rules = B.WordRules(lm) if form.startswith("word") else None
        for W, nbest, xs in sets:
            for x in xs:
                r = B.search(x, W, nbest, vocab[1], df, lm, rules)
                t = BR.tau(x.shape[0], r.kmax)
                tot += 1
                frag += r.margin < t
                mm, tm = min(mm, r.margin), max(tm, t)
    print(f"V={vocab[0]} {form}: {tot} utterances, {frag} fragile, min margin {mm:.3g}, max tau {tm:.3g}")
    assert tot == 84 and frag == 0


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_value_errors():
    t = tok()
    ok = [((2, 3), 1.0)]
    for args, msg in [(([], 6, 0), "no phrase"), (([((), 1.0)], 6, 0), "empty spelling"), (([((2, 6), 1.0)], 6, 0), "leave"),
                      (([((2, -1), 1.0)], 6, 0), "leave"), (([((2, 0), 1.0)], 6, 0), "blank"), (([((2,), math.nan)], 6, 0), "boost"),
                      (([((2,), math.inf)], 6, 0), "boost"), (([((2,), -0.5)], 6, 0), "boost"), ((ok, 6, 0, None, -0.1), "partial"),
                      ((ok, 6, 0, None, 1.5), "partial"), ((ok, 6, 0, None, math.nan), "partial"), ((ok, 6, 0, None, 1.0, True), "delimiter"),
                      ((ok, 6, 0, 0), "delimiter"), ((ok, 6, 0, 6), "delimiter"), ((ok, 6, 6), "blank"), ((ok, 1, 0), "vocabulary")]:
        with pytest.raises(ValueError, match=msg):
            ContextBias(*args)
    with pytest.raises(ValueError, match="no phrase"):
        ContextBias.from_phrases([], t)
    with pytest.raises(ValueError, match="empty spelling"):
        ContextBias.from_phrases(["  "], t)
    with pytest.raises(ValueError, match="cannot spell"):
        ContextBias.from_phrases(["café society"], t)
    with pytest.raises(ValueError, match="boost"):
        ContextBias.from_ids([((2, 3), -1.0)], 6, 0)
    assert ContextBias.from_ids([(2, 3), ((3, 2), 0.5), [[2, 2], 0.25], np.array([3, 3])], 6, 0, boost=1.5).boosts == [1.5, 0.5, 0.25, 1.5]
    with pytest.raises(ValueError, match=f"more than {1 << 20}"):          # one phrase of 2^20 labels: 2^20 + 1 states
        ContextBias.from_ids([np.ones(1 << 20, np.int64)], 2, 0)
    with pytest.raises(ValueError, match="2\\^31"):                        # 2^19 states of 4096 labels
        ContextBias.from_ids([np.ones(1 << 19, np.int64)], 4096, 0)
    cb = ContextBias.from_ids([(2, 3)], 6, 0, delimiter=1)
    cb.next[1, 2] = 99
    with pytest.raises(ValueError, match="out of range"):
        cb.validate()


def test_search_argument_errors():
    """what beam_search checks on the host before it touches the device"""
    import torch
    from wav2vec2.longform import decode_long
    cb = ContextBias.from_ids([(2, 3)], 6, 0, delimiter=1)
    _check_args(6, 4, 2, 0, None, cb)
    with pytest.raises(ValueError, match="vocabulary"):
        _check_args(8, 4, 2, 0, None, cb)
    with pytest.raises(ValueError, match="blank"):
        _check_args(6, 4, 2, 2, None, cb)
    with pytest.raises(ValueError, match="blank"):
        _check_args(6, 4, 2, 5, None, cb)                                # (not the blank the bias was built with)
    with pytest.raises(ValueError, match="ContextBias"):
        _check_args(6, 4, 2, 0, None, [(2, 3)])
    wlm = WR.random_model(np.random.default_rng(1), 6, 0, 4, 5, 2)
    with pytest.raises(ValueError, match="delimiter"):
        _check_args(6, 4, 2, 0, wlm, cb)
    _check_args(6, 4, 2, 0, wlm, ContextBias.from_ids([(2, 3)], 6, 0, delimiter=4))
    _check_args(6, 4, 2, 0, wlm, ContextBias.from_ids([(2, 3)], 6, 0))
    with pytest.raises(ValueError, match="greedy"):
        decode_long(torch.zeros((5, 6)), beam_width=None, bias=cb)
