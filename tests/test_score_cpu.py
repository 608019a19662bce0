"""Host side of the exact CTC scoring: the fp64 reference against brute force and torch's double ctc_loss, and the
host functions of wav2vec2.decoding that work on the scores (hypothesis_posteriors, word_confidence, rescore's bookkeeping with a
stubbed scorer).  No GPU."""

import itertools
import math

import numpy as np
import pytest

import score_reference as SR


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_equals_brute_force():
    rng = np.random.default_rng(1)
    for T, V in [(1, 2), (3, 3), (5, 4), (6, 4), (6, 3)]:
        x = (rng.standard_normal((T, V)) * 3).astype(np.float32)
        for blank in (0, V - 1):
            labs = [l for U in range(0, 4) for l in itertools.product([v for v in range(V) if v != blank], repeat=U)]
            total = 0.0
            for lab in labs:
                got, ref = SR.ctc_logp(x, lab, blank), SR.brute_force(x, lab, blank)
                if ref == -math.inf:
                    assert got == -math.inf and T < len(lab) + SR.repeats(lab)
                else:
                    assert abs(got - ref) <= SR.tau(T, ref), (T, V, lab, got, ref)
                    total += math.exp(ref)
            if T <= 3:                                       # every transcript of up to 3 labels: the probabilities sum to 1
                assert abs(total - 1.0) < 1e-12


def test_reference_equals_torch_ctc_loss():
    import torch
    rng = np.random.default_rng(2)
    worst = 0.0
    for case in range(24):
        T = int(rng.integers(1, 200))
        V = (5, 32, 64)[case % 3]
        scale = (1.0, 4.0, 12.0)[(case // 3) % 3]
        x = (rng.standard_normal((T, V)) * scale).astype(np.float32)
        U = int(rng.integers(0, max(1, T // 2) + 1))
        lab = rng.integers(1, V, U)
        if U > 2 and case % 2:
            lab[1] = lab[0]                                  # a repeated neighbour
        if T < U + SR.repeats(lab):
            continue
        lp = torch.log_softmax(torch.from_numpy(x).double(), dim=1)[:, None, :]
        ref = -float(torch.nn.functional.ctc_loss(lp, torch.from_numpy(lab.astype(np.int64))[None], torch.tensor([T]), torch.tensor([U]),
                                                  blank=0, reduction="sum", zero_infinity=False))
        got = SR.ctc_logp(x, lab, 0)
        worst = max(worst, abs(got - ref) / SR.tau(T, ref))
        assert abs(got - ref) <= SR.tau(T, ref), (case, T, V, U, got, ref)
    print(f"largest |reference - torch| / tau = {worst:.4f}")


def test_reference_conventions():
    x = np.zeros((6, 5), np.float32)
    assert SR.ctc_logp(x, [1, 1, 2, 2, 3], 0) == -math.inf           # needs 7 frames
    assert math.isfinite(SR.ctc_logp(np.zeros((7, 5), np.float32), [1, 1, 2, 2, 3], 0))
    assert math.isnan(SR.ctc_logp(x, [0], 0)) and math.isnan(SR.ctc_logp(x, [5], 0)) and math.isnan(SR.ctc_logp(x, [-1], 0))
    y = x.copy()
    y[2, 4] = np.nan
    assert math.isnan(SR.ctc_logp(y, [1], 0))
    y[2, 4] = np.inf
    assert math.isnan(SR.ctc_logp(y, [1], 0))
    y[:, 4] = -np.inf
    assert math.isfinite(SR.ctc_logp(y, [1], 0)) and SR.ctc_logp(y, [4], 0) == -math.inf
    # the range: 40 frames whose blank leads by 2000; a probability form that flushes exp(-2000) would give -inf
    z = np.zeros((40, 5), np.float32)
    z[:, 0] = 2000.0
    assert abs(SR.ctc_logp(z, [1, 2], 0) - (-3993.34)) < 0.01


# ---- posteriors ---------------------------------------------------------------------------------------------------------------
def test_hypothesis_posteriors():
    from wav2vec2.decoding import hypothesis_posteriors
    p = hypothesis_posteriors([-3.0, -4.0, -10.0])
    assert p.dtype == np.float64 and abs(p.sum() - 1.0) < 1e-15 and p[0] > p[1] > p[2]
    assert abs(p[0] / p[1] - math.e) < 1e-12
    q = hypothesis_posteriors([-10000.0, -10001.0, -10000.5])           # exp(-1e4) underflows; the max is subtracted first
    assert np.isfinite(q).all() and abs(q.sum() - 1.0) < 1e-15 and abs(q[0] / q[1] - math.e) < 1e-9
    np.testing.assert_array_equal(hypothesis_posteriors([-5.0, -7.0, -100.0, -1e4], scale=0.0), np.full(4, 0.25))
    half = hypothesis_posteriors([-3.0, -4.0], scale=0.5)
    assert abs(half[0] / half[1] - math.exp(0.5)) < 1e-12
    assert hypothesis_posteriors([]).size == 0
    np.testing.assert_array_equal(hypothesis_posteriors([-7.5]), [1.0])


# ---- word confidence ------------------------------------------------------------------------------------------------------------
def test_word_confidence():
    from wav2vec2.decoding import word_confidence
    best = [("the", 0, 10), ("cat", 12, 20)]
    post = [0.5, 0.2, 0.2, 0.1]
    lists = [best,
             [("the", 5, 15), ("cat", 16, 30)],              # both overlap exactly half: 2 * 5 >= 10, 2 * 4 >= 8
             [("the", 6, 16), ("cat", 17, 30)],              # one frame less: 2 * 4 < 10, 2 * 3 < 8
             [("teh", 0, 10), ("cat", 12, 20)]]              # a different text; the same word at the same place
    got = word_confidence(lists, post)
    assert got == [0.5 + 0.2, 0.5 + 0.2 + 0.1]
    # a repeated neighbouring word does not support its twin: "the the" against a hypothesis that holds only the second
    got = word_confidence([[("the", 0, 10), ("the", 10, 20)], [("the", 10, 20)]], [0.6, 0.4])
    assert got == [0.6, 1.0]
    # a single hypothesis
    assert word_confidence([best], [1.0]) == [1.0, 1.0]
    # no words, no hypotheses
    assert word_confidence([[], [("a", 0, 1)]], [0.5, 0.5]) == [] and word_confidence([], []) == []
    with pytest.raises(ValueError):
        word_confidence([best], [0.5, 0.5])
    # bounds: every value in [posterior_0, 1]
    rng = np.random.default_rng(5)
    for _ in range(20):
        lists = [[(str(rng.integers(0, 3)), int(s), int(s + rng.integers(1, 6))) for s in np.sort(rng.integers(0, 40, 4))] for _ in range(5)]
        p = rng.dirichlet(np.ones(5))
        for c in word_confidence(lists, p):
            assert p[0] - 1e-12 <= c <= 1.0 + 1e-12


# ---- rescore's bookkeeping, the scorer stubbed ------------------------------------------------------------------------------------
def test_rescore_ordering_and_lm_part(monkeypatch):
    from wav2vec2 import decoding as D
    H = D.Hypothesis
    exact = {(1, 2): -4.0, (1,): -3.0, (2, 2): -3.5, (3,): -1.0, (): -2.0, (4,): -2.0}
    calls = []

    def stub(logits, labels, blank=0, frame_lengths=None, utterance=None):
        calls.append((logits, [tuple(l) for l in labels], blank, frame_lengths, list(utterance)))
        return np.array([exact[tuple(l)] for l in labels], np.float64)

    monkeypatch.setattr(D, "ctc_score", stub)
    lists = [[H((1, 2), -5.0, -4.0), H((1,), -5.5, -5.5), H((2, 2), -6.0, -5.75)],     # LM parts +1, 0, +0.25
             [],                                                                         # a constrained lexicon's empty list
             [H((3,), float("nan"), float("nan"))],                                      # the greedy path
             [H((), -2.5, -2.5), H((4,), -2.75, -2.75)]]                                 # equal exact totals: the old order stays
    out = D.rescore("LOGITS", lists, blank=7, frame_lengths=[9, 9, 9, 9])
    assert len(calls) == 1                                                                # one call for everything
    assert calls[0] == ("LOGITS", [(1, 2), (1,), (2, 2), (3,), (), (4,)], 7, [9, 9, 9, 9], [0, 0, 0, 2, 3, 3])
    assert out[0] == [H((1, 2), -4.0, -3.0), H((1,), -3.0, -3.0), H((2, 2), -3.5, -3.25)]
    assert out[1] == []
    assert out[2] == [H((3,), -1.0, -1.0)]
    assert out[3] == [H((), -2.0, -2.0), H((4,), -2.0, -2.0)]
    # the order changes where the exact totals say so
    out = D.rescore("LOGITS", [[H((1, 2), -1.0, -1.0), H((1,), -2.0, -2.0)]])
    assert [h.ids for h in out[0]] == [(1,), (1, 2)]
    # nothing to score: no call
    assert D.rescore("LOGITS", [[], []]) == [[], []] and len(calls) == 2
