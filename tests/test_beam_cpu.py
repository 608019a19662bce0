"""CTC prefix beam search without a GPU: the fp64 reference (tests/beam_reference.py) against a brute-force enumeration of all V^T
frame paths, with and without language models; the textbook case where the greedy transcript is not the most probable one; the
index tie rule; CharNgramLM's counting, smoothing and argument checks; Hypothesis -> text."""

import math
import os

import numpy as np
import pytest

import beam_reference as BR
from wav2vec2.decoding import CharNgramLM, Hypothesis
from wav2vec2.processor import Wav2Vec2Processor

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")


def random_lm(rng, V, order):
    return np.log(rng.dirichlet(np.ones(V), V ** (order - 1))).astype(np.float32)


# ---- 1. the reference equals brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_reference_equals_brute_force(seed, order):
    rng = np.random.default_rng(100 * order + seed)
    T, V = int(rng.integers(1, 7)), int(rng.integers(2, 5))
    blank = int(rng.integers(0, V))
    x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
    lm = random_lm(rng, V, order) if order else None
    alpha, beta = (0.7, -0.3) if order else (0.0, 0.0)
    if seed % 3 == 2 and order:
        beta = 0.4                                           # an insertion bonus: totals may exceed 0
    got = BR.search(x, 100000, 100000, blank, lm, max(order, 1), alpha, beta)
    want = BR.brute_force(x, blank, lm, max(order, 1), alpha, beta)
    assert not got.bad and got.margin >= 0
    assert len(got.hyps) == len(want)
    exact = {k: (s, t) for k, s, t in want}
    for k, s, t in got.hyps:                                 # every transcript, with its exact score and total
        assert abs(s - exact[k][0]) <= 1e-12 and abs(t - exact[k][1]) <= 1e-12, (k, s, t, exact[k])
    totals = [t for _, _, t in got.hyps]
    assert all(a >= b for a, b in zip(totals, totals[1:]))
    # the same ranking as the enumeration wherever the enumeration's neighbours are apart by more than the rounding
    for i, (k, s, t) in enumerate(want):
        near = (i > 0 and want[i - 1][2] - t <= 1e-12) or (i + 1 < len(want) and t - want[i + 1][2] <= 1e-12)
        if not near:
            assert got.hyps[i][0] == k, (i, k, got.hyps[i])


def test_reference_pruned_score_is_a_lower_bound():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((6, 4)) * 1.5).astype(np.float32)
    exact = {k: s for k, s, _ in BR.brute_force(x)}
    for W in (1, 2, 3, 5):
        for k, s, t in BR.search(x, W, W).hyps:
            assert s <= exact[k] + 1e-12 and s == t


# ---- 2. greedy is not the most probable transcript ------------------------------------------------------------------------------
def greedy_case():
    """two frames, P(blank) = 0.4, P(a) = 0.35, P(b) = 0.25: the argmax path is blank-blank (0.16, the empty transcript), but "a"
    summed over its three paths (a a, a _, _ a) has 0.1225 + 2 * 0.14 = 0.4025"""
    return np.log(np.array([[0.4, 0.35, 0.25]] * 2)).astype(np.float32)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_reference_beats_greedy(W):
    x = greedy_case()
    assert x.argmax(1).tolist() == [0, 0]
    r = BR.search(x, W, 1)
    assert r.hyps[0][0] == (1,)
    assert abs(math.exp(r.hyps[0][1]) - 0.4025) < 1e-6


def test_reference_width_one_returns_the_empty_transcript():
    r = BR.search(greedy_case(), 1, 1)                       # the label is pruned after the first frame
    assert r.hyps[0][0] == () and abs(math.exp(r.hyps[0][1]) - 0.16) < 1e-6


def test_reference_index_tie_rule_and_bad_rows():
    x = np.zeros((3, 4), np.float32)                         # every column equal: hypotheses that swap letters have equal keys
    r = BR.search(x, 1000, 1000)
    assert r.margin == 0.0
    one = [k for k, _, _ in r.hyps if len(k) == 1]
    assert one == [(1,), (2,), (3,)]                         # equal keys in ascending candidate index
    two = [k for k, _, _ in r.hyps if len(k) == 2 and k[0] != k[1]]
    assert two == sorted(two)
    y = np.zeros((3, 4), np.float32)
    y[1, 2] = np.nan
    assert BR.search(y, 4, 2).bad and BR.search(y, 4, 2).hyps == []
    y[1, 2] = np.inf
    assert BR.search(y, 4, 2).bad
    y[1, 2] = -np.inf                                        # legal: that label cannot be emitted at frame 1
    r = BR.search(y, 1000, 1000)
    exact = {k: s for k, s, _ in BR.brute_force(y)}
    assert not r.bad and all(abs(s - exact[k]) <= 1e-12 for k, s, _ in r.hyps)
    assert len(r.hyps) == sum(1 for s in exact.values() if s > -math.inf)


# ---- 3. CharNgramLM -------------------------------------------------------------------------------------------------------------
def test_lm_add_k_on_a_hand_counted_example():
    V, blank = 4, 0
    lm = CharNgramLM.from_ids([[1, 2, 1, 2], [1, 3]], V, blank, order=2, add_k=0.5)
    assert lm.table.shape == (4, 4) and lm.order == 2 and lm.alpha == 1.0 and lm.beta == 0.0
    p = np.exp(lm.table.astype(np.float64))
    # history = blank (begin of sentence): 1 twice; history 1: 2 twice, 3 once; history 2: 1 once; history 3: nothing
    np.testing.assert_allclose(p[0, 1:], np.array([2.5, 0.5, 0.5]) / 3.5, rtol=1e-6)
    np.testing.assert_allclose(p[1, 1:], np.array([0.5, 2.5, 1.5]) / 4.5, rtol=1e-6)
    np.testing.assert_allclose(p[2, 1:], np.array([1.5, 0.5, 0.5]) / 2.5, rtol=1e-6)
    np.testing.assert_allclose(p[3, 1:], np.full(3, 1 / 3), rtol=1e-6)
    np.testing.assert_allclose(p[:, 1:].sum(1), 1.0, rtol=1e-6)          # each row sums to 1 over the labels


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_lm_rows_sum_to_one_and_blank_filled_history(order):
    rng = np.random.default_rng(order)
    V, blank = 6, 5
    seqs = [rng.integers(0, 5, size=int(rng.integers(0, 12))).tolist() for _ in range(20)]
    lm = CharNgramLM.from_ids(seqs, V, blank, order, add_k=1.0, alpha=0.5, beta=0.1)
    assert lm.table.shape == (V ** (order - 1), V) and np.isfinite(lm.table).all()
    p = np.exp(lm.table.astype(np.float64))
    np.testing.assert_allclose(np.delete(p, blank, axis=1).sum(1), 1.0, rtol=1e-5)
    # the first label of every sequence is counted in the all-blank row, the row the reference's ctx gives an empty prefix
    start = BR.lm_context((), V, blank, order)
    first = np.bincount([s[0] for s in seqs if s], minlength=V).astype(np.float64)
    if order > 1:
        want = (first + 1.0) / (first.sum() + 1.0 * (V - 1))
        np.testing.assert_allclose(p[start], want, rtol=1e-5)
        s = next(s for s in seqs if len(s) >= order)
        assert BR.lm_context(tuple(s[:order - 1]), V, blank, order) == sum(c * V ** (order - 2 - k) for k, c in enumerate(s[:order - 1]))


def test_lm_rejects_bad_input():
    good = np.zeros((16, 4), np.float32)
    CharNgramLM(good, 3)
    for table, order in [(np.zeros((4, 4), np.float32), 3), (np.zeros((16, 4), np.float32), 2), (np.zeros(4, np.float32), 1),
                         (good, 0), (good, 5), (np.zeros((1, 65), np.float32), 1)]:
        with pytest.raises(ValueError):
            CharNgramLM(table, order)
    for bad in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[3, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            CharNgramLM(t, 3)
    with pytest.raises(ValueError, match="finite"):
        CharNgramLM(good, 3, alpha=np.inf)
    with pytest.raises(ValueError):
        CharNgramLM.from_ids([[1, 0]], 4, 0, 2)              # the blank inside a sequence
    with pytest.raises(ValueError):
        CharNgramLM.from_ids([[1, 4]], 4, 0, 2)
    with pytest.raises(ValueError):
        CharNgramLM.from_ids([[1]], 4, 0, 2, add_k=0.0)
    with pytest.raises(ValueError):
        CharNgramLM.from_ids([[1]], 4, 4, 2)


def test_lm_from_text_and_hypothesis_text():
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    lm = CharNgramLM.from_text(["the cat", "the hat"], tok, order=2, add_k=0.1)
    assert lm.table.shape == (32, 32)
    v = tok.get_vocab()
    p = np.exp(lm.table.astype(np.float64))
    assert abs(p[v["T"], v["H"]] - (2 + 0.1) / (2 + 0.1 * 31)) < 1e-6          # T is followed by H twice (the final T of CAT / HAT by nothing)
    assert abs(p[v["<pad>"], v["T"]] - (2 + 0.1) / (2 + 0.1 * 31)) < 1e-6      # both texts start with T
    h = Hypothesis(tuple(tok("hello  world")), -1.0, -2.0)
    assert h.text(tok) == "HELLO  WORLD".strip()
    assert Hypothesis((v["L"], v["L"], v["|"]), 0.0, 0.0).text(tok) == "LL"     # no CTC collapse: these are labels, not frames
    assert Hypothesis((), 0.0, 0.0).text(tok) == ""


def test_argument_checks_need_no_device():
    from wav2vec2.decoding import _check_args
    lm8 = CharNgramLM(np.zeros((1, 8), np.float32), 1)
    lm4 = CharNgramLM(np.zeros((1, 4), np.float32), 1)
    _check_args(8, 16, 1, 0, None)
    _check_args(8, 64, 64, 7, lm8)
    for args in [(8, 0, 1, 0, None), (8, 65, 1, 0, None), (8, 4, 5, 0, None), (8, 4, 0, 0, None), (8, 4, 1, 8, None),
                 (8, 4, 1, -1, None), (65, 4, 1, 0, None), (8, 4, 1, 0, lm4), (8, 4, 1, 0, "arpa")]:
        with pytest.raises(ValueError):
            _check_args(*args)
