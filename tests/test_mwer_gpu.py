"""MWER training on the GPU (wav2vec2.losses.expected_risk / MWERLoss): expected_risk against the composition of the
fp64 numpy references, descent on fixed lists, MWERLoss against expected_risk on its own lists, and two Trainer steps.

Gradient tolerance: score_grad_reference.bar with expected_risk's own coefficients (see tests/test_score_grad_gpu.py)."""

import types

import numpy as np
import pytest

import helpers as H
import score_grad_reference as GR
import score_reference as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


LISTS = [[(1, 2, 3), (1, 2), (1, 3, 3), ()], [(4, 5), (4,), (5, 4, 1)], [(2,), (2, 2)]]
RISKS = [[0.0, 1.0, 1.0, 3.0], [1.0, 0.0, 2.0], [0.0, 1.0]]
REFS = [(1, 2, 3), (4,), (2,)]


def composition(x, lists, risks, scale, prior, refs, weight):
    """(L, G, slack) per utterance from the numpy references: the definition of expected_risk"""
    out = []
    for i, (hyps, r) in enumerate(zip(lists, risks)):
        lp = np.asarray([SR.ctc_logp(x[i], h, 0) for h in hyps])
        z = scale * lp + np.asarray(prior[i])
        P = np.exp(z - z.max())
        P /= P.sum()
        L = float((P * np.asarray(r)).sum())
        c = list(scale * P * (np.asarray(r) - L))
        pairs = [list(h) for h in hyps]
        if refs is not None:
            pairs.append(list(refs[i]))
            c.append(-weight)
        logp, G, slack = GR.score_grad(x[i], pairs, c, 0)
        if refs is not None:
            L -= weight * logp[-1]
        out.append((L, G, slack))
    return out


@pytest.mark.parametrize("scale,with_prior,weight", [(1.0, False, 0.0), (0.7, True, 0.3)])
def test_expected_risk_against_the_composition(torch_mod, scale, with_prior, weight):
    from wav2vec2.losses import expected_risk
    rng = np.random.default_rng(31)
    B, T, V = 3, 40, 6
    x = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    prior = [[float(v) for v in rng.standard_normal(len(h))] for h in LISTS] if with_prior else None
    refs = REFS if weight else None
    L, grad = expected_risk(dev(torch_mod, x), LISTS, RISKS, posterior_scale=scale, prior=prior, ctc=refs, ctc_weight=weight)
    assert L.dtype == np.float64 and tuple(grad.shape) == x.shape and grad.dtype == torch_mod.float32
    grad = grad.cpu().numpy().astype(np.float64)
    want = composition(x, LISTS, RISKS, scale, prior or [[0.0] * len(h) for h in LISTS], refs, weight)
    worst = 0.0
    for i, (Li, G, slack) in enumerate(want):
        assert abs(L[i] - Li) <= 1e-12 * abs(Li), (i, L[i], Li)
        ratio = np.abs(grad[i] - G) / GR.bar(G, slack)
        assert ratio.max() <= 1.0, (i, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    assert np.abs(grad).max() > 1e-3
    print(f"expected_risk (scale {scale}, prior {with_prior}, ctc {weight}): largest |error| / bar = {worst:.4f}")


def test_descent_on_fixed_lists(torch_mod):
    from wav2vec2.losses import expected_risk
    rng = np.random.default_rng(32)
    x = dev(torch_mod, (rng.standard_normal((3, 40, 6)) * 2).astype(np.float32))
    totals = []
    for _ in range(6):
        L, grad = expected_risk(x, LISTS, RISKS)
        totals.append(float(L.sum()))
        x = x - 0.5 * grad
    print("sum_i L_i over five steps of size 0.5:", " ".join(f"{t:.5f}" for t in totals))
    assert all(b < a for a, b in zip(totals, totals[1:])), totals


def test_mwer_loss_against_expected_risk(torch_mod):
    torch = torch_mod
    from wav2vec2.losses import MWERLoss, expected_risk
    rng = np.random.default_rng(33)
    B, T, V, delim = 3, 30, 8, 4
    cfg = types.SimpleNamespace(kernal_sizes=[], strides=[], pad_id=0, vocab_size=V)
    x = dev(torch, (rng.standard_normal((B, T, V)) * 2).astype(np.float32))
    labels = np.asarray([[1, 2, 4, 3, 5, 0, 0], [6, 4, 4, 7, 1, 2, 0], [3, 0, 0, 0, 0, 0, 0]], np.int32)
    refs = [(1, 2, 4, 3, 5), (6, 4, 4, 7, 1, 2), (3,)]
    loss = MWERLoss(cfg, (B, T), division_factor=2, beam_width=8, nbest=4, delimiter_id=delim, ctc_weight=0.05)
    per, grad, total = loss.per_sample(labels, x, with_grad=True, with_total=True)
    assert tuple(per.shape) == (B,) and per.dtype == torch.float32 and tuple(grad.shape) == (B, T, V) and total.dim() == 0
    for hyps, ref, risks, post in zip(loss.last_lists, refs, loss.last_risks, loss.last_posteriors):
        assert hyps.count(ref) == 1 and len(set(hyps)) == len(hyps) and 4 <= len(hyps) <= 5       # the reference exactly once
        assert risks[hyps.index(ref)] == 0.0 and all(r >= 0 and r == int(r) for r in risks)
        assert abs(post.sum() - 1.0) < 1e-12
    L, want = expected_risk(x, loss.last_lists, loss.last_risks, ctc=refs, ctc_weight=0.05)
    assert torch.equal(grad, want / 2.0)
    np.testing.assert_array_equal(per.cpu().numpy(), L.astype(np.float32))
    assert abs(float(total) - L.sum() / 2.0) <= 1e-6 * abs(L.sum())
    assert float(loss(labels, x)) == float(total)
    # word risks: the second reference is the words (6,), (7, 1, 2); a hypothesis that differs inside one word costs one error
    from wav2vec2.losses import split_at
    assert split_at(refs[1], delim) == [(6,), (7, 1, 2)]
    # one hypothesis and no reference: P = 1, risk - L = 0, so the risk term has no gradient at all
    alone = MWERLoss(cfg, (B, T), beam_width=8, nbest=1, delimiter_id=delim, include_reference=False, ctc_weight=0.0)
    per1, grad1 = alone.per_sample(labels, x, with_grad=True)
    assert all(len(h) == 1 for h in alone.last_lists) and bool((grad1 == 0).all())
    np.testing.assert_array_equal(per1.cpu().numpy(), np.asarray([r[0] for r in alone.last_risks], np.float32))
    # unit="char" counts ids
    chars = MWERLoss(cfg, (B, T), beam_width=4, nbest=2, unit="char", ctc_weight=0.0)
    chars.per_sample(labels, x)
    from wav2vec2.metrics import edit_distance
    flat = [(h, ref) for hyps, ref in zip(chars.last_lists, refs) for h in hyps]
    counts = edit_distance([list(h) for h, _ in flat], [list(r) for _, r in flat])
    assert [c.distance for c in counts] == [int(r) for risks in chars.last_risks for r in risks]
    # per-call frame lengths
    short = loss.per_sample(labels, x, frame_lengths=[30, 20, 10])
    assert bool(torch.isfinite(short).all())


def test_trainer_runs_on_mwer_loss(torch_mod):
    import wav2vec2
    g = H.golden("tiny_base")
    x, labels = g["wave"], g["labels"]

    def run():
        cfg = H.case_config("tiny_base")
        m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(2, 4000))
        m.set_weights(H.case_weights("tiny_base"))
        m.freeze_feature_extractor()
        loss = wav2vec2.MWERLoss(cfg, x.shape, division_factor=2, beam_width=4, nbest=3, delimiter_id=4)
        tr = wav2vec2.Trainer(m, loss, learning_rate=1e-3, dropout=0.1, apply_spec_augment=False, seed=5)
        totals = [float(tr.step(x, labels)) for _ in range(2)]
        return totals, m.get_weights(), loss

    totals, w1, loss = run()
    assert all(np.isfinite(t) for t in totals), totals
    assert all(len(h) >= 1 for h in loss.last_lists)
    totals2, w2, _ = run()
    assert totals == totals2
    w0 = H.case_weights("tiny_base")
    assert any(not np.array_equal(w1[n], w0[n]) for n in w1 if n in w0)          # the steps moved something
    for n in w1:
        assert np.array_equal(w1[n], w2[n]), n
