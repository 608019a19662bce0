"""wav2vec2.metrics without a device: the reference DP (tests/edit_reference.py) against a brute-force enumeration of all
alignments, the ErrorRate totals, the word and character splitting, and the arithmetic of oracle_wer and mbr_select with the
device call replaced by the reference."""

import os

import numpy as np
import pytest

import edit_reference as ER
import helpers as H
from wav2vec2 import metrics as M


def ref_pairs(sequences, pairs):
    """edit_distance_pairs computed by the reference"""
    seqs = [list(s) for s in sequences]
    out = []
    for h, r in pairs:
        c, s, d, i = ER.edit_counts(seqs[h], seqs[r])
        out.append(M.EditCounts(c, len(seqs[r]) - s - d, s, d, i, len(seqs[r])))
    return out


@pytest.fixture
def host_distance(monkeypatch):
    calls = []

    def fake(sequences, pairs):
        pairs = list(pairs)
        calls.append(len(pairs))
        return ref_pairs(sequences, pairs)

    monkeypatch.setattr(M, "edit_distance_pairs", fake)
    return calls


def test_reference_equals_brute_force():
    """distance = the fewest errors of any alignment; among those alignments the fewest substitutions go with the most hits, and
    that alignment's (S, D, I) is unique"""
    rng = np.random.default_rng(0)
    n = 0
    for _ in range(400):
        a = rng.integers(0, 3, rng.integers(0, 7)).tolist()
        b = rng.integers(0, 3, rng.integers(0, 7)).tolist()
        al = ER.all_alignments(a, b)
        dist = min(s + d + i for _, s, d, i in al)
        best = [x for x in al if x[1] + x[2] + x[3] == dist]
        fewest = min(x[1] for x in best)
        pick = {x for x in best if x[1] == fewest}
        assert len(pick) == 1, (a, b, pick)
        h, s, d, i = next(iter(pick))
        assert h == max(x[0] for x in best)
        assert ER.edit_counts(a, b) == (dist, s, d, i), (a, b)
        assert h == len(b) - s - d and len(a) == h + s + i
        n += 1
    assert n == 400
    assert ER.edit_counts("ab", "ba") == (2, 0, 1, 1)
    assert ER.edit_counts([], [1, 2, 3]) == (3, 0, 3, 0) and ER.edit_counts([1, 2], []) == (2, 0, 0, 2)
    assert ER.edit_counts([], []) == (0, 0, 0, 0)


def test_error_rate_totals():
    counts = [M.EditCounts(3, 4, 1, 1, 1, 6), M.EditCounts(0, 5, 0, 0, 0, 5), M.EditCounts(2, 0, 0, 0, 2, 0)]
    e = M.ErrorRate.from_counts(counts)
    assert (e.errors, e.ref_len, e.hits, e.substitutions, e.deletions, e.insertions) == (5, 11, 9, 1, 1, 3)
    assert e.rate == 5 / 11 and e.per_utterance == counts
    # the corpus rate, not the mean of the utterances' rates
    assert e.rate != np.mean([3 / 6, 0.0])
    with pytest.raises(ValueError):
        M.ErrorRate.from_counts([M.EditCounts(2, 0, 0, 0, 2, 0)])
    with pytest.raises(ValueError):
        M.ErrorRate.from_counts([])


def test_word_and_character_splitting(host_distance):
    assert M.split_words("  the  quick\tbrown \n fox ") == ["the", "quick", "brown", "fox"]
    assert M.split_chars("  a  b\tc ") == [ord(c) for c in "a b c"]
    assert M.split_chars("") == [] and M.split_words("   ") == []

    class T:
        text = "hello  world"
    assert M.split_words(T()) == ["hello", "world"]
    with pytest.raises(TypeError):
        M.split_words(3)
    w = M.wer(["the cat  sat", T(), ""], ["the cat sat down", "hello there world", "a"])
    assert [c.distance for c in w.per_utterance] == [1, 1, 1] and w.ref_len == 8 and w.rate == 3 / 8
    assert w.deletions == 3 and w.hits == 5
    # no normalisation: case and punctuation count
    assert M.wer(["Hello, World"], ["hello world"]).errors == 2
    c = M.cer(["a  bc"], [" a b c "])
    assert (c.errors, c.ref_len, c.deletions) == (1, 5, 1)
    assert host_distance == [3, 1, 1]                    # one call per corpus


def test_python_value_errors(host_distance):
    with pytest.raises(ValueError):
        M.wer(["a"], ["a", "b"])
    with pytest.raises(ValueError):
        M.cer(["a", "b"], ["a"])
    with pytest.raises(ValueError):
        M.wer([""], [""])                                # no reference token (found after the distances)
    with pytest.raises(ValueError):
        M.oracle_wer([["a"]], ["a", "b"])
    with pytest.raises(ValueError):
        M.mbr_select([[((1, 2), 0.0)]], unit="word")     # no tokenizer to split words with
    with pytest.raises(ValueError):
        M.mbr_select([[((1, 2), 0.0)]], unit="phone")
    with pytest.raises(ValueError):
        M.mbr_select([[((1, 2), float("nan")), ((1,), 0.0)]], unit="char")
    assert host_distance == [1]


def test_limits_raise_before_any_launch(monkeypatch):
    from wav2vec2 import _native as N
    monkeypatch.setattr(N, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    assert M.edit_distance([], []) == [] and M.edit_distance_pairs([[1, 2]], []) == []
    long = np.zeros(N.EDIT_MAX_LEN + 1, np.int32)
    with pytest.raises(ValueError, match="65535"):
        M.edit_distance([long], [[1]])
    with pytest.raises(ValueError):
        M.edit_distance_pairs([[1], [2]], [(0, 2)])
    with pytest.raises(ValueError):
        M.edit_distance([[1]], [[1], [2]])
    with pytest.raises(ValueError):
        M.edit_distance([[2 ** 31]], [[1]])


def test_oracle_wer_arithmetic(host_distance):
    nbest = [["a b c", "a x c d", "a b c d"],            # errors 1, 1, 0 -> index 2
             ["x y", "p q", "p"],                        # errors 2, 0 (tie with nothing), 1 -> index 1
             ["m n", "n m", "m"],                        # reference "m o": 1, 2, 1 -> tie, lowest index 0
             []]                                         # no hypothesis: the empty string, 2 deletions
    refs = ["a b c d", "p q", "m o", "u v"]
    e, chosen = M.oracle_wer(nbest, refs)
    assert chosen == [2, 1, 0, -1]
    assert [c.distance for c in e.per_utterance] == [0, 0, 1, 2]
    assert (e.errors, e.ref_len) == (3, 10) and e.rate == 0.3
    assert host_distance == [10]                         # all hypotheses of all utterances in one call

    class Tr:
        texts = ["p", "p q"]
    e2, chosen2 = M.oracle_wer([Tr()], ["p q"])
    assert chosen2 == [1] and e2.errors == 0


def test_mbr_select_arithmetic(host_distance):
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))
    delim = tok.get_vocab()["|"]
    rng = np.random.default_rng(1)
    lists = []
    for K in (1, 2, 5, 8):
        base = rng.integers(5, 12, 14).tolist()
        hyps = []
        for _ in range(K):
            ids = [int(rng.integers(5, 12)) if rng.random() < 0.2 else x for x in base]
            ids = [delim if rng.random() < 0.25 else x for x in ids]
            hyps.append((tuple(ids), float(rng.normal(-20, 2))))
        lists.append(hyps)

    def words(ids):
        out, cur = [], []
        for x in list(ids) + [delim]:
            if x == delim:
                if cur:
                    out.append(tuple(cur))
                cur = []
            else:
                cur.append(x)
        return out

    for unit, tokens in (("word", words), ("char", list)):
        del host_distance[:]
        idx, risks = M.mbr_select(lists, tok, unit=unit, scale=0.5)
        want_idx, want_risks = ER.mbr_reference(lists, tokens, 0.5)
        assert idx == want_idx
        for r, w in zip(risks, want_risks):
            np.testing.assert_allclose(r, w, rtol=1e-13, atol=0)
        assert host_distance == [0 + 1 + 10 + 28]        # K (K - 1) / 2 pairs per utterance, one call
    # Hypothesis objects rank by `total`; a single hypothesis and an empty list need no distance
    from wav2vec2.decoding import Hypothesis
    del host_distance[:]
    idx, risks = M.mbr_select([[Hypothesis((5, 6), -1.0, -3.0)], []], unit="char")
    assert idx == [0, -1] and risks[0].tolist() == [0.0] and risks[1].size == 0
    # ties go to the lowest index: three hypotheses at equal distances and equal probability
    idx, risks = M.mbr_select([[((1, 2), 0.0), ((1, 3), 0.0), ((1, 4), 0.0)]], unit="char")
    assert idx == [0] and risks[0].tolist() == [2 / 3] * 3
    # the probability mass decides: the outlier never wins, and a sharper softmax moves the choice to the top score
    hyps = [((1, 2, 3, 4), 0.0), ((1, 2, 3), -0.1), ((1, 2, 3), -0.2), ((9, 9, 9, 9, 9, 9), -0.05)]
    assert M.mbr_select([hyps], unit="char", scale=1.0)[0] == [1]
    assert M.mbr_select([hyps], unit="char", scale=100.0)[0] == [0]
