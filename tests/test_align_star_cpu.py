"""The star (wildcard) label of the CTC forced alignment without a GPU: the fp64 reference
(tests/align_star_reference.py) against align_reference.viterbi -- bit-equal without a star, and the same decisions as a run on
logits with the star's column appended --, the planted-gap experiment behind the default star_score, and the host code of
wav2vec2.alignment: word_spans with star_id, split_at_pauses with star_text, the transcript building of Wav2Vec2ForCTC.align and
the ValueErrors."""

import numpy as np
import pytest

import align_reference as AR
import align_star_reference as SR
from wav2vec2 import alignment as A
from wav2vec2.alignment import TokenSpan, WordSpan, split_at_pauses, star_transcript, word_spans


def rand_labels(rng, U, V, blank, rep=0.2):
    out = []
    for _ in range(U):
        if out and rng.random() < rep:
            out.append(out[-1])
        else:
            out.append(int(rng.choice([v for v in range(V) if v != blank])))
    return out


def same_bits(a, b):
    for u, v in zip(a[:3], b[:3]):
        assert u.dtype == v.dtype
        np.testing.assert_array_equal(u.view(np.int32), v.view(np.int32))
    assert np.float64(a[3]).tobytes() == np.float64(b[3]).tobytes() or (np.isnan(a[3]) and np.isnan(b[3]))


# ---- 1. without a star: align_reference's bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_star_free_labels_give_the_star_free_reference_bits(seed):
    rng = np.random.default_rng(seed)
    V, blank = (6, 2) if seed % 2 else (32, 0)
    U = int(rng.integers(0, 30))
    labels = rand_labels(rng, U, V, blank)
    T = U + AR.repeats(labels) + int(rng.integers(0, 20)) - (seed == 3) + (U == 0)
    x = rng.integers(-2, 3, size=(max(T, 1), V)).astype(np.float32) if seed % 3 == 0 else \
        rng.standard_normal((max(T, 1), V)).astype(np.float32) * 3
    if seed == 5:
        x[3 % x.shape[0], 1] = np.nan
    if seed == 7 and U:
        labels[U // 2] = blank                         # a bad label: the NaN utterance from both
    same_bits(SR.viterbi(x, labels, blank, -0.5), AR.viterbi(x, labels, blank))


# ---- 2. the star is one more column ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_star_equals_an_appended_column(seed):
    rng = np.random.default_rng(100 + seed)
    V, blank = (5, 1) if seed % 2 else (32, 0)
    U = int(rng.integers(1, 25))
    labels = rand_labels(rng, U, V, blank)
    for k in sorted(set(int(k) for k in rng.integers(0, U, size=1 + U // 6))):
        if (k == 0 or labels[k - 1] != V) and (k == U - 1 or labels[k + 1] != V):
            labels[k] = V
    if seed == 0:
        labels = [V]
    T = len(labels) + AR.repeats(labels) + int(rng.integers(0, 25))
    x = (rng.integers(-24, 25, size=(T, V)) / 8.0).astype(np.float32)       # multiples of 1/8: m_t - 0.5 is exact in fp32
    m = SR.frame_max(x)
    aug = np.concatenate([x, (m + np.float32(-0.5))[:, None]], axis=1).astype(np.float32)
    assert (aug[:, V].astype(np.float64) == SR.star_emission(x, -0.5)).all()
    tok, li, fl, sc = SR.viterbi(x, labels, blank, -0.5)
    rtok, rli, _, _ = AR.viterbi(aug, labels, blank)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(li, rli)
    assert (tok == V).any() and ((tok == V) == np.isin(li, np.flatnonzero(np.asarray(labels) == V))).all()
    # frame_logp of a star frame: the frame's maximum plus star_score, normalised by the lse of the V real columns
    star = tok == V
    np.testing.assert_array_equal(fl[star], (m[star].astype(np.float64) - 0.5 - AR.lse(x)[star]).astype(np.float32))


def test_frame_max_ignores_nan_like_fmax():
    x = np.array([[1.0, np.nan, 3.0], [np.nan, np.nan, np.nan], [-np.inf, -2.0, np.nan]], np.float32)
    np.testing.assert_array_equal(SR.frame_max(x), np.array([3.0, -np.inf, -2.0], np.float32))


# ---- 3. the planted-gap experiment behind the default star_score -------------------------------------------------------------
def planted_case(rng, V=32, blank=0):
    """runs A, X, C of labels on a planted frame path: each label held 1-3 frames, 0-2 blank frames between labels (one more
    before a repeated label); N(0, 1) logits with +6 on the path."""
    runs = [[int(v) for v in rng.integers(1, V, size=int(rng.integers(lo, hi + 1)))] for lo, hi in ((3, 11), (3, 19), (3, 11))]
    labels = runs[0] + runs[1] + runs[2]
    path = []
    for k, l in enumerate(labels):
        if k:
            path += [blank] * (int(rng.integers(0, 3)) + (l == labels[k - 1]))
        path += [l] * int(rng.integers(1, 4))
    x = rng.standard_normal((len(path), V)).astype(np.float32)
    x[np.arange(len(path)), path] += 6.0
    return x, runs


def planted_recovered(star_score, n=200):
    rng = np.random.default_rng(0)
    ok = 0
    for _ in range(n):
        x, (a, gap, c) = planted_case(rng)
        V = x.shape[1]
        _, full, _, _ = AR.viterbi(x, a + gap + c, 0)
        _, li, _, _ = SR.viterbi(x, a + [V] + c, 0, star_score)
        want = np.where(full < len(a), full, np.where(full >= len(a) + len(gap), full - len(gap) + 1, -2))
        got = np.where(li == len(a), -2, li)
        keep = (want >= 0) | (got >= 0)                 # the frames of A's and C's labels, in either alignment
        ok += bool((want[keep] == got[keep]).all())
    return ok


def test_planted_gaps_are_recovered_at_the_default_star_score():
    assert A.DEFAULT_STAR_SCORE == -0.5
    assert planted_recovered(-0.5) == 200


def test_a_star_that_ties_with_correct_labels_recovers_fewer():
    assert planted_recovered(0.0) < 200


# ---- 4. host code ------------------------------------------------------------------------------------------------------------
def test_word_spans_with_a_star():
    V, d = 32, 4
    spans = [TokenSpan(V, 0, 5, 0.5), TokenSpan(7, 5, 7, 0.9), TokenSpan(8, 7, 8, 0.6), TokenSpan(V, 9, 12, 0.25), TokenSpan(9, 12, 13, 1.0),
             TokenSpan(d, 13, 14, 1.0), TokenSpan(10, 14, 16, 0.5), TokenSpan(V, 16, 20, 0.125)]
    words = word_spans(spans, d, 0.02, star_id=V)
    assert [w.text for w in words] == ["*", (7, 8), "*", (9,), (10,), "*"]
    assert words[0] == WordSpan("*", 0.0, 5 * 0.02, 0.5) and words[2] == WordSpan("*", 9 * 0.02, 12 * 0.02, 0.25)
    assert words[1].start_s == 5 * 0.02 and words[1].end_s == 8 * 0.02 and words[1].score == pytest.approx((0.9 * 2 + 0.6) / 3)
    assert [w.text for w in word_spans(spans, d, 0.02, star_id=V, star_text="<gap>")][0] == "<gap>"
    # without star_id the call is the one it was: the star's id is a token like any other
    assert [w.text for w in word_spans(spans, d, 0.02)] == [(V, 7, 8, V, 9), (10, V)]


def test_split_at_pauses_cuts_at_star_words():
    w = lambda t, a, b: WordSpan(t, a, b, 0.5)
    words = [w("*", 0.0, 1.0), w("A", 1.0, 1.2), w("B", 1.25, 1.4), w("*", 1.4, 1.5), w("C", 1.5, 1.7), w("D", 2.5, 2.8), w("*", 2.8, 3.0)]
    segs = split_at_pauses(words, min_pause_s=0.3, star_text="*")
    assert [s.text for s in segs] == ["A B", "C", "D"]
    assert all(x.text != "*" for s in segs for x in s.words)
    assert (segs[0].start_s, segs[0].end_s) == (1.0, 1.4)
    assert split_at_pauses([w("*", 0.0, 1.0)], star_text="*") == []
    # without star_text a star word is a word
    assert [s.text for s in split_at_pauses(words, min_pause_s=0.3)] == ["* A B * C", "D *"]


def test_transcript_building():
    tok = lambda s: [{"|": 4}.get(c, ord(c)) for c in s.upper().replace(" ", "|")]
    V = 32
    hello = tok("HELLO WORLD")
    assert 4 in hello
    assert star_transcript("* HELLO WORLD *", V, tok, "*") == [V] + hello + [V]
    assert star_transcript("HELLO * WORLD", V, tok, "*") == tok("HELLO") + [V] + tok("WORLD")        # no delimiter beside the star
    assert star_transcript("HELLO WORLD", V, tok, "*") == hello == star_transcript("HELLO WORLD", V, tok)
    assert star_transcript("HELLO WORLD", V, tok, None, free_ends=True) == [V] + hello + [V]
    assert star_transcript("* HELLO WORLD", V, tok, "*", free_ends=True) == [V] + hello + [V]       # no second star at an end
    assert star_transcript([5, V, 6], V) == [5, V, 6] and star_transcript([5, 6], V, free_ends=True) == [V, 5, 6, V]
    assert star_transcript("", V, tok, "*", free_ends=True) == [V] and star_transcript("*", V, tok, "*", free_ends=True) == [V]
    assert star_transcript("* *", V, tok, "*") == [V, V]            # (forced_align refuses it)
    with pytest.raises(ValueError, match="tokenizer"):
        star_transcript("HELLO", V, None, "*")


def test_value_errors_on_the_host():
    V = 32
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 32\)"):
        A._check_labels([[3, V]], [10], V, 0)                       # V without star_score
    assert A._check_labels([[3, V, 5]], [10], V, 0, star=True)[0].tolist() == [3, V, 5]
    with pytest.raises(ValueError, match="two stars next to each other"):
        A._check_labels([[3, V, V, 5]], [10], V, 0, star=True)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 32\]"):
        A._check_labels([[V + 1]], [10], V, 0, star=True)
    with pytest.raises(ValueError, match="is the blank"):
        A._check_labels([[V, 0]], [10], V, 0, star=True)
    with pytest.raises(ValueError, match="cannot hold"):
        A._check_labels([[V, 3, 3]], [3], V, 0, star=True)          # the star needs a frame of its own
    for bad in (0.25, float("nan")):
        with pytest.raises(ValueError, match="star_score"):
            A.forced_align(None, None, star_score=bad)
        with pytest.raises(ValueError, match="star_score"):
            A.forced_align_long(None, None, star_score=bad)
    assert A.star_id(np.zeros((3, 7, V))) == V and A.star_id([np.zeros((7, V))]) == V
