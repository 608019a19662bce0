"""The fp64 numpy reference of w2v2_ctc_score_grad (tests/score_grad_reference.py) against torch's fp64 autograd through
torch.nn.functional.ctc_loss on the CPU, and the definition's own conventions where autograd is no reference (-inf logits, too few
frames).  No GPU."""

import math

import numpy as np
import pytest

import score_grad_reference as GR
import score_reference as SR

torch = pytest.importorskip("torch")


def autograd(x, pairs, coef, blank):
    """(logp per pair, d sum_j c_j logp_j / d x) in fp64 through torch's CTC loss"""
    xt = torch.tensor(np.asarray(x, np.float32).astype(np.float64), requires_grad=True)
    lp = torch.log_softmax(xt, dim=1)
    T = xt.shape[0]
    total, logps = 0.0, []
    for lab, c in zip(pairs, coef):
        nll = torch.nn.functional.ctc_loss(lp[:, None, :], torch.tensor([list(lab)], dtype=torch.long).reshape(1, -1), torch.tensor([T]),
                                           torch.tensor([len(lab)]), blank=blank, reduction="sum", zero_infinity=False)
        logps.append(-float(nll.detach()))
        total = total + float(c) * (-nll)
    total.backward()
    return np.asarray(logps), xt.grad.numpy()


def problems():
    """about 60 seeded problems, T <= 14, V <= 6: U = 0, T = 1, repeated labels, T = U + R, several pairs with both signs"""
    rng = np.random.default_rng(2024)
    out = []
    for k in range(60):
        V = int(rng.integers(2, 7))
        blank = int(rng.integers(0, V)) if k % 3 else 0
        pool = [v for v in range(V) if v != blank]
        T = 1 if k % 10 == 0 else int(rng.integers(1, 15))
        m = 1 + k % 4
        pairs = []
        for j in range(m):
            if k % 6 == 1 and j == 0:
                lab = []                                        # U = 0
            elif k % 6 == 2 and j == 0:                         # T = U + R exactly: the problem takes its T from this pair
                lab = [int(v) for v in rng.choice(pool, int(rng.integers(1, 7)))]
                for i in range(1, len(lab)):
                    if rng.random() < 0.5:
                        lab[i] = lab[i - 1]
                T = len(lab) + SR.repeats(lab)
            else:
                U = int(rng.integers(0, max(1, T // 2) + 1))
                lab = [int(v) for v in rng.choice(pool, U)]
                for i in range(1, U):
                    if rng.random() < 0.35:
                        lab[i] = lab[i - 1]
                while len(lab) + SR.repeats(lab) > T:
                    lab.pop()
            pairs.append(lab)
        coef = rng.standard_normal(m) * 2
        if m > 1:
            coef[0], coef[1] = abs(coef[0]), -abs(coef[1])
        x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
        out.append((x, pairs, coef, blank))
    return out


def test_reference_against_autograd():
    worst, seen = 0.0, dict(u0=0, t1=0, rep=0, tight=0, multi=0)
    for x, pairs, coef, blank in problems():
        logp, G, _ = GR.score_grad(x, pairs, coef, blank)
        want_lp, want = autograd(x, pairs, coef, blank)
        assert np.isfinite(want_lp).all()
        np.testing.assert_allclose(logp, want_lp, rtol=0, atol=1e-12)
        worst = max(worst, float(np.abs(G - want).max()))
        seen["u0"] += any(len(p) == 0 for p in pairs)
        seen["t1"] += x.shape[0] == 1
        seen["rep"] += any(SR.repeats(p) for p in pairs)
        seen["tight"] += any(len(p) and len(p) + SR.repeats(p) == x.shape[0] for p in pairs)
        seen["multi"] += len(pairs) > 1 and (np.asarray(coef) > 0).any() and (np.asarray(coef) < 0).any()
    print(f"numpy reference against torch fp64 autograd: largest difference {worst:.3e}; cases {seen}")
    assert worst <= 1e-12
    assert all(v >= 3 for v in seen.values()), seen


def test_logp_is_the_scorers():
    for x, pairs, coef, blank in problems()[:20]:
        logp, _, _ = GR.score_grad(x, pairs, coef, blank)
        for lp, lab in zip(logp, pairs):
            assert lp == SR.ctc_logp(x, lab, blank)


def test_unused_minus_inf_column():
    rng = np.random.default_rng(5)
    T, V = 9, 6
    x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
    x[:, 4] = -np.inf                                           # no label uses column 4
    pairs, coef = [[1, 2, 2], [3], []], [0.7, -1.3, 0.4]
    logp, G, _ = GR.score_grad(x, pairs, coef, 0)
    assert np.isfinite(logp).all() and np.isfinite(G).all()
    assert (G[:, 4] == 0).all()
    keep = [0, 1, 2, 3, 5]
    logp2, G2, _ = GR.score_grad(x[:, keep], pairs, coef, 0)
    np.testing.assert_allclose(logp, logp2, rtol=0, atol=1e-13)
    np.testing.assert_allclose(G[:, keep], G2, rtol=0, atol=1e-13)
    _, want = autograd(x[:, keep], pairs, coef, 0)
    np.testing.assert_allclose(G2, want, rtol=0, atol=1e-12)


def test_used_minus_inf_column_and_one_frame_short():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((6, 5)) * 2).astype(np.float32)
    lab = [1, 1, 2, 2, 3]                                       # U + R = 7: one frame less than feasible
    logp, G, slack = GR.score_grad(x, [lab], [1.5], 0)
    assert logp[0] == -math.inf and (G == 0).all() and slack == 0.0
    # beside a feasible pair it adds nothing
    logp2, G2, _ = GR.score_grad(x, [lab, [1, 2]], [1.5, -0.5], 0)
    _, only, _ = GR.score_grad(x, [[1, 2]], [-0.5], 0)
    assert logp2[0] == -math.inf and math.isfinite(logp2[1])
    np.testing.assert_array_equal(G2, only)
    # seven frames: feasible, and autograd agrees
    x7 = (rng.standard_normal((7, 5)) * 2).astype(np.float32)
    logp7, G7, _ = GR.score_grad(x7, [lab], [1.5], 0)
    _, want = autograd(x7, [lab], [1.5], 0)
    assert math.isfinite(logp7[0])
    np.testing.assert_allclose(G7, want, rtol=0, atol=1e-12)
    # a -inf column that the labels use: no path, no contribution
    x7[:, 2] = -np.inf
    logp8, G8, _ = GR.score_grad(x7, [lab], [1.5], 0)
    assert logp8[0] == -math.inf and (G8 == 0).all()
    # bad label and non-finite utterance: NaN and nothing
    assert math.isnan(GR.score_grad(x, [[0]], [1.0], 0)[0][0]) and math.isnan(GR.score_grad(x, [[5]], [1.0], 0)[0][0])
    xn = x.copy()
    xn[2, 1] = np.nan
    lpn, Gn, _ = GR.score_grad(xn, [[1]], [1.0], 0)
    assert math.isnan(lpn[0]) and (Gn == 0).all()


def test_gamma_sums_to_one_per_frame():
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((12, 6)) * 3).astype(np.float32)
    _, Gam = GR.occupancy(x, [1, 1, 4, 2], 0)
    np.testing.assert_allclose(Gam.sum(axis=1), 1.0, rtol=0, atol=1e-13)
