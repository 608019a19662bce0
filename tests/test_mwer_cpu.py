"""The host side of MWER training (wav2vec2.losses.expected_risk / MWERLoss) without a GPU: the coefficients of
expected_risk against torch fp64 autograd with the native calls replaced by the numpy reference, list building, and argument
errors."""

import types

import numpy as np
import pytest

import score_grad_reference as GR
import score_reference as SR

torch = pytest.importorskip("torch")


@pytest.fixture
def stubbed(monkeypatch):
    """wav2vec2.decoding.ctc_score / ctc_score_grad computed by the numpy references on lists of (T_i, V) CPU tensors"""
    from wav2vec2 import decoding as D
    calls = dict(score=0, grad=0)

    def ctc_score(logits, labels, blank=0, frame_lengths=None, utterance=None):
        calls["score"] += 1
        return np.asarray([SR.ctc_logp(logits[i].numpy(), lab, blank) for i, lab in zip(utterance, labels)])

    def ctc_score_grad(logits, labels, coef, blank=0, frame_lengths=None, utterance=None, max_workspace_bytes=0):
        calls["grad"] += 1
        logp, grads = np.empty(len(labels)), []
        for i, x in enumerate(logits):
            mine = [j for j, u in enumerate(utterance) if u == i]
            lp, G, _ = GR.score_grad(x.numpy(), [labels[j] for j in mine], [coef[j] for j in mine], blank)
            logp[mine] = lp
            grads.append(torch.from_numpy(G))
        return logp, grads

    monkeypatch.setattr(D, "ctc_score", ctc_score)
    monkeypatch.setattr(D, "ctc_score_grad", ctc_score_grad)
    return calls


def autograd_risk(xs, lists, risks, scale, prior, refs, weight, blank):
    """L_i and d sum_i L_i / d x in fp64: sum_j softmax(scale * logp + prior)_j risk_j - weight * logp_ref"""
    Ls, grads = [], []
    for i, x in enumerate(xs):
        xt = torch.tensor(x.astype(np.float64), requires_grad=True)
        lp = torch.log_softmax(xt, dim=1)
        T = xt.shape[0]

        def logp(lab):
            return -torch.nn.functional.ctc_loss(lp[:, None, :], torch.tensor(list(lab), dtype=torch.long).reshape(1, -1), torch.tensor([T]),
                                                 torch.tensor([len(lab)]), blank=blank, reduction="sum")
        z = torch.stack([scale * logp(h) + p for h, p in zip(lists[i], prior[i])])
        L = (torch.softmax(z, dim=0) * torch.tensor(risks[i], dtype=torch.float64)).sum()
        if refs is not None:
            L = L - weight * logp(refs[i])
        L.backward()
        Ls.append(float(L.detach()))
        grads.append(xt.grad.numpy())
    return np.asarray(Ls), grads


@pytest.mark.parametrize("scale,with_prior,weight", [(1.0, False, 0.0), (0.6, True, 0.0), (1.0, True, 0.25), (0.0, False, 0.01)])
def test_expected_risk_against_autograd(stubbed, scale, with_prior, weight):
    from wav2vec2.losses import expected_risk
    rng = np.random.default_rng(3)
    xs = [(rng.standard_normal((T, 6)) * 2).astype(np.float32) for T in (9, 12, 7)]
    lists = [[(1, 2), (1,), (2, 2, 3), ()], [(4, 5, 1), (4, 1)], [(3,)]]
    risks = [[0.0, 1.0, 2.0, 2.0], [1.0, 0.0], [3.0]]
    prior = [[float(v) for v in rng.standard_normal(len(h))] for h in lists] if with_prior else None
    refs = [(1, 2), (4, 1), (5, 5)] if weight or scale == 0.0 else None
    L, grad = expected_risk([torch.from_numpy(x) for x in xs], lists, risks, blank=0, posterior_scale=scale, prior=prior, ctc=refs,
                            ctc_weight=weight)
    want_L, want = autograd_risk(xs, lists, risks, scale, prior or [[0.0] * len(h) for h in lists], refs, weight, 0)
    assert stubbed == dict(score=1, grad=1)
    assert L.dtype == np.float64
    np.testing.assert_allclose(L, want_L, rtol=1e-12, atol=1e-13)
    worst = max(float(np.abs(g.numpy() - w).max()) for g, w in zip(grad, want))
    print(f"scale {scale}, prior {with_prior}, ctc weight {weight}: largest gradient difference {worst:.3e}")
    assert worst <= 1e-12
    if not weight:
        assert (grad[2].numpy() == 0).all()                    # a list of one: P = 1 and risk - L = 0 exactly


def test_infeasible_hypothesis_is_left_out(stubbed):
    from wav2vec2.losses import expected_risk
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((4, 5)) * 2).astype(np.float32)
    lists, risks = [[(1, 2), (1, 1, 2, 2), (3,)]], [[1.0, 0.0, 2.0]]            # the second needs 6 frames
    L, grad = expected_risk([torch.from_numpy(x)], lists, risks)
    L2, grad2 = expected_risk([torch.from_numpy(x)], [[(1, 2), (3,)]], [[1.0, 2.0]])
    assert L[0] == L2[0]
    np.testing.assert_array_equal(grad[0].numpy(), grad2[0].numpy())


def test_expected_risk_refusals(stubbed):
    from wav2vec2.losses import expected_risk
    x = [torch.zeros((5, 4))]
    with pytest.raises(ValueError, match="twice"):
        expected_risk(x, [[(1, 2), (1, 2)]], [[0.0, 1.0]])
    with pytest.raises(ValueError, match="risks"):
        expected_risk(x, [[(1, 2), (1,)]], [[0.0]])
    with pytest.raises(ValueError, match="non-negative"):
        expected_risk(x, [[(1, 2), (1,)]], [[0.0, -1.0]])
    with pytest.raises(ValueError, match="priors"):
        expected_risk(x, [[(1, 2), (1,)]], [[0.0, 1.0]], prior=[[0.0]])
    with pytest.raises(ValueError, match="references"):
        expected_risk(x, [[(1, 2)]], [[0.0]], ctc=[(1,), (2,)], ctc_weight=0.1)
    with pytest.raises(ValueError, match="posterior_scale"):
        expected_risk(x, [[(1, 2)]], [[0.0]], posterior_scale=-1.0)
    with pytest.raises(ValueError, match="ctc_weight"):
        expected_risk(x, [[(1, 2)]], [[0.0]], ctc_weight=float("nan"))
    with pytest.raises(ValueError, match="2 lists for 1 utterances"):
        expected_risk(x, [[(1, 2)], [(1,)]], [[0.0], [1.0]])
    with pytest.raises(ValueError, match="nothing"):
        expected_risk(x, [[]], [[]])
    assert stubbed == dict(score=0, grad=0)


def test_list_building():
    from wav2vec2.decoding import Hypothesis
    from wav2vec2.losses import build_lists, split_at, token_pool
    hyps = [[Hypothesis((1, 2), -1.0, -1.5), Hypothesis((1,), -2.0, -2.25), Hypothesis((1, 2), -3.0, -3.0)],
            [Hypothesis((3, 4, 3), -1.0, -1.0), Hypothesis((3,), float("nan"), float("nan"))],
            []]
    refs = [(1,), (3, 3), ()]
    lists, priors = build_lists(hyps, refs, include_reference=True, with_prior=True)
    assert lists == [[(1, 2), (1,)], [(3, 4, 3), (3,), (3, 3)], [()]]          # deduplicated; present once; appended; the empty reference
    assert priors == [[-0.5, -0.25], [0.0, 0.0, 0.0], [0.0]]                   # total - score; NaN (a greedy path) counts as 0
    lists2, priors2 = build_lists(hyps, refs, include_reference=False)
    assert lists2 == [[(1, 2), (1,)], [(3, 4, 3), (3,)], []] and priors2 == [[0.0, 0.0], [0.0, 0.0], []]
    # words: split at the delimiter, empty runs dropped, one interning table for the call
    assert split_at((4, 1, 2, 4, 4, 3, 4), 4) == [(1, 2), (3,)] and split_at((), 4) == [] and split_at((4, 4), 4) == []
    pool, pairs = token_pool([[(1, 2, 4, 3), (3, 4, 1, 2)], [(1, 2)]], [(1, 2, 4, 3), (3,)], "word", 4)
    assert [p.tolist() for p in pool] == [[0, 1], [0, 1], [1, 0], [1], [0]]
    assert pairs == [(1, 0), (2, 0), (4, 3)]
    assert all(p.dtype == np.int32 for p in pool)
    pool, pairs = token_pool([[(1, 2, 4, 3)]], [(1, 2)], "char", None)
    assert [p.tolist() for p in pool] == [[1, 2], [1, 2, 4, 3]] and pairs == [(1, 0)]


def test_mwer_loss_argument_errors():
    from wav2vec2.losses import CTCLoss, MWERLoss
    cfg = types.SimpleNamespace(kernal_sizes=[10, 3], strides=[5, 2], pad_id=0, vocab_size=32)
    ok = MWERLoss(cfg, (2, 4000), delimiter_id=4)
    assert ok.beam_width == 8 and ok.nbest == 4 and ok.unit == "word" and ok.ctc_weight == 0.01 and ok.include_reference
    assert ok._ctc._get_logit_length(4000) == CTCLoss(cfg, (2, 4000))._get_logit_length(4000)
    assert MWERLoss(cfg, (2, 4000), unit="char").delimiter_id is None
    for kw in [dict(), dict(delimiter_id=0), dict(delimiter_id=32), dict(delimiter_id=4, unit="token"), dict(delimiter_id=4, nbest=0),
               dict(delimiter_id=4, beam_width=2, nbest=3), dict(delimiter_id=4, ctc_weight=-0.1), dict(delimiter_id=4, posterior_scale=-1),
               dict(delimiter_id=4, division_factor=0), dict(delimiter_id=4, beam_width=0)]:
        with pytest.raises(ValueError):
            MWERLoss(cfg, (2, 4000), **kw)
