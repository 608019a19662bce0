"""Host side of the CTC phrase search: the fp64 reference (tests/spot_reference.py) against brute force over all
begins and frame strings, the properties of the hit pass, the chunk rule on the input the GPU test uses, and the host logic of
wav2vec2.spotting with the kernel call stubbed by the reference (phrase_labels, thresholds, pairs, chunk plan and ownership,
times, every ValueError).  No GPU."""

import itertools
import os

import numpy as np
import pytest

import spot_reference as SR

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_equals_brute_force():
    rng = np.random.default_rng(1)
    checked = ties = 0
    for T, V, ints in [(1, 2, False), (4, 2, True), (6, 2, False), (5, 3, False), (6, 3, True), (6, 3, False)]:
        x = rng.integers(-2, 3, (T, V)).astype(np.float32) if ints else (rng.standard_normal((T, V)) * 3).astype(np.float32)
        for blank in (0, V - 1):
            pool = [v for v in range(V) if v != blank]
            for U in (1, 2, 3):
                for lab in itertools.product(pool, repeat=U):
                    z, c = SR.trace(x, lab, blank)
                    bf = SR.brute_force(x, lab, blank)
                    for t in range(T):
                        best, begins = bf[t]
                        assert z[t] == best, (T, V, blank, lab, t, z[t], best)        # the same additions in the same order: exact
                        if best == -np.inf:
                            assert c[t] == -1
                            continue
                        assert int(c[t]) in begins, (T, V, blank, lab, t, c[t], begins)
                        assert SR.path_score(x, lab, blank, int(c[t]), t) == z[t]      # the best path over [c_t, t] attains z_t
                        checked += 1
                        ties += len(begins) > 1
    assert checked > 300 and ties > 20


def test_reference_ties_keep_the_earlier_begin():
    # the first label is the argmax over a run of frames: the hit begins at the run's first frame
    x = np.zeros((8, 3), np.float32)
    x[:, 0] = 1.0                                           # blank leads ...
    x[2:6, 1] = 2.0                                         # ... except on frames 2 .. 5, where label 1 does
    x[6, 2] = 2.0
    z, c = SR.trace(x, [1, 2], 0)
    assert z[6] == 0.0 and c[6] == 2
    z, c = SR.trace(x, [1], 0)
    assert list(c[2:6]) == [2, 2, 2, 2] and (z[2:6] == 0.0).all()
    assert (z[6], c[6]) == (-2.0, 2)                        # stay (0.0) ties with the fresh start: the path goes on
    assert (z[7], c[7]) == (-1.0, 7)                        # ... and restarts once it has fallen below it


def test_reference_conventions():
    x = np.zeros((6, 5), np.float32)
    for bad in ([0], [5], [-1], [1, 0, 2]):
        assert SR.trace(x, bad, 0) is None
    y = x.copy()
    y[2, 4] = np.nan
    assert SR.trace(y, [1], 0) is None
    y[2, 4] = np.inf
    assert SR.trace(y, [1], 0) is None
    y[2, :] = -np.inf
    assert SR.trace(y, [1], 0) is None
    y = x.copy()
    y[:, 4] = -np.inf                                       # legal: label 4 can never be emitted
    z, _ = SR.trace(y, [4], 0)
    assert (z == -np.inf).all() and SR.spot(y, [4], 0)[0] == 0
    z, _ = SR.trace(x[:2], [1, 2, 3], 0)                    # fewer frames than labels: no hit
    assert (z == -np.inf).all()
    n, s, b, e, _, _ = SR.spot(y, [0], 0, max_hits=3)
    assert n == -1 and np.isnan(s).all() and (b == -1).all() and (e == -1).all()


def test_reference_edge_rule():
    blank, delim, A, B = 0, 1, 2, 3
    path = [A, B, delim, 0, 0, 0, delim, A, B, delim, 0, 0, 0, delim, A, B]
    x = SR.planted(np.random.default_rng(3), len(path), 5, blank, dict(enumerate(path)))
    lab = [delim, A, B, delim]
    on = SR.hit_pass(*SR.trace(x, lab, blank, delim), -1.0)
    off = SR.hit_pass(*SR.trace(x, lab, blank, -1), -1.0)
    assert on == [(0.0, 0, 2), (0.0, 6, 9), (0.0, 13, 15)] and off == [(0.0, 6, 9)]
    # a recording that is just the word
    x = SR.planted(np.random.default_rng(4), 4, 5, blank, {0: A, 1: A, 2: B, 3: B})
    assert SR.hit_pass(*SR.trace(x, lab, blank, delim), -1.0) == [(0.0, 0, 3)]
    assert SR.hit_pass(*SR.trace(x, lab, blank, -1), -1.0) == []
    # U < 3: the rule is off
    za, ca = SR.trace(x, [delim, delim], blank, delim)
    zb, cb = SR.trace(x, [delim, delim], blank, -1)
    assert np.array_equal(za, zb) and np.array_equal(ca, cb)


# ---- the hit pass ---------------------------------------------------------------------------------------------------------------
def test_hit_pass_properties():
    rng = np.random.default_rng(5)
    total = 0
    for case in range(40):
        T, V = int(rng.integers(5, 120)), 4
        x = rng.integers(-2, 3, (T, V)).astype(np.float32) if case % 2 else rng.standard_normal((T, V)).astype(np.float32)
        lab = rng.integers(1, V, int(rng.integers(1, 5)))
        z, c = SR.trace(x, lab, 0)
        for thr in (-np.inf, -6.0, -2.0, -0.5, 0.0, np.inf):
            hits = SR.hit_pass(z, c, thr)
            total += len(hits)
            for s, b, e in hits:
                assert s >= thr and s > -np.inf and 0 <= b <= e < T and z[e] == s and c[e] == b
            for u, v in zip(hits, hits[1:]):
                assert u[2] < v[1]                           # time order, pairwise non-overlapping
            n, s, b, e, _, _ = SR.spot(x, lab, 0, -1, thr, max_hits=2)
            assert n == len(hits) and [(s[i], b[i], e[i]) for i in range(min(n, 2))] == hits[:2]
            assert np.isnan(s[min(n, 2):]).all() and (b[min(n, 2):] == -1).all()
    assert total > 200


# ---- the chunk rule: the input of the GPU test ------------------------------------------------------------------------------------
CHUNK_PHRASE = [1, 2, 2, 3]
CHUNK_FRAMES = [1, 1, 1, 2, 2, 0, 2, 2, 3, 3, 3]            # 11 frames that spell it


def chunk_input(seed, T=1500, V=8, every=97):
    path = {t: 0 for t in range(T)}
    starts = list(range(0, T - len(CHUNK_FRAMES), every))
    for s in starts:
        for k, v in enumerate(CHUNK_FRAMES):
            path[s + k] = v
    return SR.planted(np.random.default_rng(seed), T, V, 0, path), starts


def test_chunk_plan_and_rule():
    assert SR.chunk_plan(100, 256, 64) == [(0, 100)]
    assert SR.chunk_plan(256, 256, 64) == [(0, 256)]
    assert SR.chunk_plan(257, 256, 64) == [(0, 256), (192, 65)]
    assert SR.chunk_plan(1500, 256, 64) == [(192 * k, min(256, 1500 - 192 * k)) for k in range(8)]
    for T, C, Ov in [(1000, 100, 1), (1000, 100, 99), (77, 10, 3)]:
        plan = SR.chunk_plan(T, C, Ov)
        assert plan[0][0] == 0 and plan[-1][0] + plan[-1][1] == T and all(f >= 1 for _, f in plan)
        assert all(b[0] - a[0] == C - Ov for a, b in zip(plan, plan[1:])) and all(f == C for _, f in plan[:-1])
    for seed in range(10):
        x, starts = chunk_input(seed)
        whole = SR.hit_pass(*SR.trace(x, CHUNK_PHRASE, 0), -1.0)
        assert len(starts) == 16 and whole == [(0.0, s, s + 8) for s in starts]      # the first frame of the last label ends the hit: ties keep it
        assert SR.chunked(x, CHUNK_PHRASE, 0, -1.0, 256, 64) == whole


# ---- host logic, the kernel stubbed by the reference ------------------------------------------------------------------------------
class FakeBase:
    """what _logits_base returns, on the host"""

    def __init__(self, a):
        self.a, self.shape, self.device = a, a.shape, "cpu"

    def __getitem__(self, k):
        return FakeBase(self.a[k])


@pytest.fixture
def stubbed(monkeypatch):
    from wav2vec2 import decoding as D
    from wav2vec2 import spotting as S
    calls = []

    def logits_base(logits, frame_lengths):
        parts = [np.asarray(p, np.float32) for p in logits]
        return FakeBase(np.concatenate(parts)), list(np.cumsum([0] + [len(p) for p in parts[:-1]])), [len(p) for p in parts]

    def spot(base, row0, frames, utt, labs, blank, delim, thr, max_hits, trace):
        calls.append(dict(row0=list(row0), frames=list(frames), utt=list(utt), labs=[list(l) for l in labs], delim=delim, thr=list(thr),
                          max_hits=max_hits, trace=trace))
        out = [SR.spot(base.a[row0[u]:row0[u] + frames[u]], l, blank, delim, t, max_hits) for u, l, t in zip(utt, labs, thr)]
        return (np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), np.stack([o[3] for o in out]),
                np.asarray([o[0] for o in out], np.int32), [(o[4], o[5]) if trace else None for o in out])

    def ctc_score(views, labels, blank=0, frame_lengths=None, utterance=None):
        calls.append(dict(score=[(v.shape[0], list(l)) for v, l in zip(views, labels)]))
        return np.asarray([-2.0 * v.shape[0] for v in views])

    monkeypatch.setattr(S, "_logits_base", logits_base)
    monkeypatch.setattr(S, "_spot", spot)
    monkeypatch.setattr(D, "ctc_score", ctc_score)
    return S, calls


def test_phrase_labels():
    from wav2vec2.processor import Wav2Vec2Processor
    from wav2vec2.spotting import phrase_labels
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    v = tok.get_vocab()
    d = v["|"]
    assert phrase_labels("cat", tok) == [d, v["C"], v["A"], v["T"], d]
    assert phrase_labels(" the cat ", tok) == [d, v["T"], v["H"], v["E"], d, v["C"], v["A"], v["T"], d]
    assert phrase_labels("cat", tok, whole_words=False) == [v["C"], v["A"], v["T"]]
    assert phrase_labels("", tok) == [] and phrase_labels(" ", tok) == []


def test_find_phrases_pairs_thresholds_and_hits(stubbed):
    S, calls = stubbed
    rng = np.random.default_rng(7)
    blank, V = 0, 6
    quiet = {t: blank for t in range(40)}                  # the blank leads wherever nothing is planted
    xs = [SR.planted(rng, 40, V, blank, {**quiet, 5: 1, 6: 2, 7: 3, 20: 1, 21: 2, 22: 3}),
          SR.planted(rng, 25, V, blank, {**{t: blank for t in range(25)}, 10: 4, 11: 4, 12: 5})]
    phrases = [[1, 2, 3], [4, 5]]
    hits = S.find_phrases(xs, phrases, blank=blank)
    assert len(calls) == 1 and calls[0]["utt"] == [0, 0, 1, 1] and calls[0]["labs"] == [[1, 2, 3], [4, 5], [1, 2, 3], [4, 5]]
    assert calls[0]["thr"] == [-3.0, -2.0, -3.0, -2.0] and calls[0]["delim"] == -1 and calls[0]["max_hits"] == 64 and not calls[0]["trace"]
    assert calls[0]["row0"] == [0, 40] and calls[0]["frames"] == [40, 25]
    assert [[(h.phrase, h.begin, h.end, h.score, h.logp) for h in hs] for hs in hits] == \
        [[(0, 5, 7, 0.0, None), (0, 20, 22, 0.0, None)], [], [], [(1, 10, 12, 0.0, None)]]
    # thresholds: margin_per_label, one min_score, one per phrase
    S.find_phrases(xs, phrases, margin_per_label=0.5)
    assert calls[-1]["thr"] == [-1.5, -1.0, -1.5, -1.0]
    S.find_phrases(xs, phrases, min_score=-7)
    assert calls[-1]["thr"] == [-7.0] * 4
    S.find_phrases(xs, phrases, min_score=[-1, -np.inf], delimiter_id=3, max_hits=5)
    assert calls[-1]["thr"] == [-1.0, -np.inf, -1.0, -np.inf] and calls[-1]["delim"] == 3 and calls[-1]["max_hits"] == 5
    # explicit pairs
    got = S.find_phrases(xs, [[4, 5], [1, 2, 3], [4, 5]], utterance=[1, 0, 0])
    assert calls[-1]["utt"] == [1, 0, 0] and [[(h.phrase, h.begin, h.end) for h in hs] for hs in got] == [[(0, 10, 12)], [(1, 5, 7), (1, 20, 22)], []]
    # trace
    got, traces = S.find_phrases(xs, phrases, trace=True)
    assert calls[-1]["trace"] and len(traces) == 4 and traces[3][0].shape == (25,) and traces[3][0][12] == 0.0 and traces[3][1][12] == 10
    # exact: ONE scoring call over every hit, on views of the logits
    n0 = len(calls)
    got = S.find_phrases(xs, phrases, exact=True)
    assert len(calls) == n0 + 2 and calls[-1]["score"] == [(3, [1, 2, 3]), (3, [1, 2, 3]), (3, [4, 5])]
    assert [h.logp for hs in got for h in hs] == [-2.0, -2.0, -2.0]
    n0 = len(calls)
    assert S.find_phrases(xs, [[5, 5, 5, 5]], exact=True) == [[], []] and len(calls) == n0 + 1      # no hit: no scoring call
    # a bad recording: None for its pairs
    bad = xs[1].copy()
    bad[3, 2] = np.nan
    got = S.find_phrases([xs[0], bad], phrases)
    assert got[2] is None and got[3] is None and len(got[0]) == 2


def test_find_phrases_chunks(stubbed):
    S, calls = stubbed
    x, starts = chunk_input(3)
    y, _ = chunk_input(4, T=300)
    got = S.find_phrases([x, y], [CHUNK_PHRASE, [5]], min_score=-1.0, chunk_frames=256, overlap_frames=64, delimiter_id=7)
    call = calls[-1]
    plan = SR.chunk_plan(1500, 256, 64) + [(1500 + s, f) for s, f in SR.chunk_plan(300, 256, 64)]
    assert call["row0"] == [s for s, _ in plan] and call["frames"] == [f for _, f in plan] and call["delim"] == -1
    assert call["utt"] == list(range(8)) * 2 + [8, 9] * 2 and call["labs"] == [CHUNK_PHRASE] * 8 + [[5]] * 8 + [CHUNK_PHRASE] * 2 + [[5]] * 2
    assert [(h.score, h.begin, h.end) for h in got[0]] == SR.chunked(x, CHUNK_PHRASE, 0, -1.0, 256, 64) == [(0.0, s, s + 8) for s in starts]
    assert [(h.score, h.begin, h.end) for h in got[2]] == SR.chunked(y, CHUNK_PHRASE, 0, -1.0, 256, 64) and len(got[2]) == 3
    assert got[1] == SR.chunked(x, [5], 0, -1.0, 256, 64) == []
    # ownership: a hit that ends inside a later piece's first `overlap` frames belongs to the piece before
    z = SR.planted(np.random.default_rng(9), 400, 8, 0, {**{t: 0 for t in range(400)}, 200: 1, 201: 2, 202: 3})
    got = S.find_phrases([z], [[1, 2, 3]], min_score=-1.0, chunk_frames=256, overlap_frames=64)
    assert [(h.begin, h.end) for h in got[0]] == [(200, 202)]             # found by both pieces (local end 10 < 64 in the second), kept once
    for kw in (dict(chunk_frames=256), dict(overlap_frames=64), dict(chunk_frames=64, overlap_frames=64), dict(chunk_frames=64, overlap_frames=0),
               dict(chunk_frames=256, overlap_frames=64, trace=True)):
        with pytest.raises(ValueError):
            S.find_phrases([z], [[1, 2, 3]], **kw)


def test_find_phrases_value_errors(stubbed):
    S, calls = stubbed
    xs = [np.zeros((9, 6), np.float32)]
    for phrases, kw, msg in [([[1], []], {}, "phrase 1 is empty"), ([[1], [6]], {}, "phrase 1"), ([[-1]], {}, "phrase 0"), ([[1, 0]], {}, "blank"),
                             ([[1, 5]], dict(blank=5), "blank"), ([[1] * 257], {}, "phrase 0: 257 labels"), ([], {}, "no phrase"),
                             ([[1]], dict(blank=6), "blank"), ([[1]], dict(delimiter_id=0), "delimiter"), ([[1]], dict(delimiter_id=6), "delimiter"),
                             ([[1]], dict(max_hits=0), "max_hits"), ([[1], [2]], dict(utterance=[0]), "utterance"),
                             ([[1]], dict(utterance=[1]), "utterance"), ([[1]], dict(utterance=[-1]), "utterance"),
                             ([[1], [2]], dict(min_score=[-1.0]), "min_score"), ([[1]], dict(min_score=float("nan")), "NaN")]:
        with pytest.raises(ValueError, match=msg):
            S.find_phrases(xs, phrases, **kw)
    assert not calls                                         # refused before the kernel
    assert S.find_phrases(xs, [[1] * 256]) == [[]]           # the limit itself is accepted


def test_spans_and_search_logits(stubbed):
    S, calls = stubbed
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    v = tok.get_vocab()
    V, blank, d = max(v.values()) + 1, v["<pad>"], v["|"]
    rng = np.random.default_rng(11)
    path = {t: blank for t in range(60)}
    for t, ch in zip(range(10, 15), "|HI|A"):
        path[t] = v[ch]
    for t, ch in zip(range(30, 34), "|HI|"):
        path[t] = v[ch]
    path[57], path[58], path[59] = d, v["H"], v["I"]                 # the recording ends with the word: found through the edge rule
    x = SR.planted(rng, 60, V, blank, path)
    spf = 0.02
    got = S.search_logits([x, x[:40]], ["hi", (v["A"],)], tok, blank, spf, min_score=-1.0)
    assert calls[-1]["delim"] == d and calls[-1]["labs"][0] == [d, v["H"], v["I"], d] and calls[-1]["labs"][1] == [v["A"]]
    assert got[0] == [S.PhraseSpan("hi", 10 * spf, 14 * spf, 0.0, None), S.PhraseSpan((v["A"],), 14 * spf, 15 * spf, 0.0, None),
                      S.PhraseSpan("hi", 30 * spf, 34 * spf, 0.0, None), S.PhraseSpan("hi", 57 * spf, 60 * spf, 0.0, None)]
    assert [s.text for s in got[1]] == ["hi", (v["A"],), "hi"]
    assert S.search_logits([x], "hi", tok, blank, spf, min_score=-1.0, whole_words=False)[0][0].start_s == 11 * spf
    assert S.search_logits([x], ["hi"], tok, blank, spf, min_score=-1.0, exact=True)[0][0].logp == -2.0
    with pytest.raises(ValueError, match="tokenizer"):
        S.search_logits([x], ["hi"], None, blank, spf)
    with pytest.raises(ValueError):
        S.search_logits([x], ["hi"], tok, blank, spf, utterance=[0])
