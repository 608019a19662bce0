"""CTC forced alignment without a GPU: the fp64 reference Viterbi (tests/align_reference.py) against a brute-force enumeration of
every valid path, and the span helpers of wav2vec2.alignment on hand-built paths."""

import itertools

import numpy as np
import pytest

import align_reference as AR
from wav2vec2.alignment import Alignment, TokenSpan, WordSpan, token_spans, word_spans


def brute_force(x, labels, blank):
    """best (end score, states) over every valid state sequence; ties broken as the definition does: end state S-2 before S-1,
    then, from the last frame down, staying before advancing by one before skipping."""
    x = np.asarray(x, np.float32).astype(np.float64)
    T = x.shape[0]
    U = len(labels)
    S = 2 * U + 1
    ext = [blank if s % 2 == 0 else labels[s // 2] for s in range(S)]
    best = None
    for moves in itertools.product((0, 1, 2), repeat=T - 1):
        for s0 in ((0, 1) if U else (0,)):
            states = [s0]
            ok = True
            for mv in moves:
                s = states[-1] + mv
                if s >= S or (mv == 2 and (ext[s] == blank or ext[s] == ext[s - 2])):
                    ok = False
                    break
                states.append(s)
            if not ok or states[-1] < S - 2 or (U == 0 and states[-1] != 0):
                continue
            acc = x[0, ext[states[0]]]
            for t in range(1, T):
                acc = acc + x[t, ext[states[t]]]
            key = (-acc, 0 if (U and states[-1] == S - 2) else 1, tuple(reversed(moves)))
            if best is None or key < best[0]:
                best = (key, acc, states)
    return best[1], np.array(best[2])


@pytest.mark.parametrize("seed", range(40))
def test_reference_is_the_brute_force_optimum_with_its_tie_rule(seed):
    rng = np.random.default_rng(seed)
    V, blank = 4, int(rng.integers(0, 4))
    U = int(rng.integers(0, 4))
    others = [v for v in range(V) if v != blank]
    labels = [int(rng.choice(others)) for _ in range(U)]
    T = int(rng.integers(max(1, U + AR.repeats(labels)), 8))
    # small integers: many exact ties between paths
    x = rng.integers(-2, 3, size=(T, V)).astype(np.float32) if seed % 2 else rng.standard_normal((T, V)).astype(np.float32)
    tok, li, fl, score, states = AR.viterbi(x, labels, blank, return_states=True)
    acc, bstates = brute_force(x, labels, blank)
    np.testing.assert_array_equal(states, bstates)
    assert score == acc - AR.lse(x).sum()
    ext = np.array([blank if s % 2 == 0 else labels[s // 2] for s in range(2 * U + 1)])
    np.testing.assert_array_equal(tok, ext[bstates])
    np.testing.assert_array_equal(li, np.where(bstates % 2 == 1, bstates // 2, -1))


def test_reference_bad_and_infeasible():
    x = np.zeros((3, 5), np.float32)
    tok, li, fl, sc = AR.viterbi(x, [1, 1, 1], 0)           # needs 3 + 2 frames
    assert sc == -np.inf and (tok == -1).all() and (li == -1).all() and np.isnan(fl).all()
    assert np.isnan(AR.viterbi(x, [0], 0)[3]) and np.isnan(AR.viterbi(x, [5], 0)[3])
    tok, li, fl, sc = AR.viterbi(x, [2, 2], 0)              # T = U + R: the only path 2 _ 2
    np.testing.assert_array_equal(tok, [2, 0, 2])
    np.testing.assert_array_equal(li, [0, -1, 1])


def alignment_from_states(states, labels, blank, logp=None):
    states = np.asarray(states)
    ext = np.array([blank if s % 2 == 0 else labels[s // 2] for s in range(2 * len(labels) + 1)])
    li = np.where(states % 2 == 1, states // 2, -1).astype(np.int32)
    fl = np.log(np.full(states.size, 0.5, np.float32)) if logp is None else np.asarray(logp, np.float32)
    return Alignment(ext[states].astype(np.int32), li, fl, 0.0)


def test_token_spans_repeated_letters():
    # labels "E E" (5 5) must be separated by a blank: states 1 1 2 3 4
    al = alignment_from_states([1, 1, 2, 3, 4], [5, 5], 0, np.log([0.5, 0.25, 1.0, 1.0, 1.0]))
    spans = token_spans(al)
    assert [(s.token, s.start, s.end) for s in spans] == [(5, 0, 2), (5, 3, 4)]
    assert spans[0].score == pytest.approx(0.375) and spans[1].score == pytest.approx(1.0)


def test_word_spans_delimiters_and_seconds():
    d = 4
    # "| A B | | C |": leading, doubled and trailing delimiters; blanks between some tokens
    labels = [d, 7, 24, d, d, 19, d]
    states = [0, 1, 3, 3, 4, 5, 7, 8, 9, 11, 12, 13, 14]
    al = alignment_from_states(states, labels, 0)
    spans = token_spans(al)
    assert [s.token for s in spans] == labels
    words = word_spans(spans, d, 0.02, vocab={7: "A", 24: "B", 19: "C"})
    assert [w.text for w in words] == ["AB", "C"]
    a, b = words
    assert (a.start_s, a.end_s) == pytest.approx((0.02 * 2, 0.02 * 6))
    assert (b.start_s, b.end_s) == pytest.approx((0.02 * 9, 0.02 * 10))
    assert a.score == pytest.approx(0.5) and isinstance(a, WordSpan)
    assert [w.text for w in word_spans(spans, d, 0.02)] == [(7, 24), (19,)]


def test_word_score_is_mean_over_token_frames():
    spans = [TokenSpan(7, 0, 3, 0.9), TokenSpan(8, 5, 6, 0.3), TokenSpan(4, 6, 7, 1.0)]
    (w,) = word_spans(spans, 4, 0.5)
    assert w.score == pytest.approx((0.9 * 3 + 0.3) / 4) and (w.start_s, w.end_s) == (0.0, 3.0)


def test_empty_transcript_and_no_path():
    al = alignment_from_states([0, 0, 0], [], 0)
    assert token_spans(al) == [] and word_spans([], 4, 0.02) == []
    none = Alignment(np.full(4, -1, np.int32), np.full(4, -1, np.int32), np.full(4, np.nan, np.float32), float("-inf"))
    assert token_spans(none) == []
