"""The fp64 numpy reference of w2v2_ctc_score_star / w2v2_ctc_score_grad_star (tests/score_star_reference.py) against
a brute-force sum over all frame paths, the star-free references, the aligner's reference and central finite differences, and the
host code of the star in wav2vec2.decoding, wav2vec2.losses and the C ABI table.  No GPU."""

import math

import numpy as np
import pytest

import align_star_reference as AS
import score_grad_reference as GR
import score_reference as SR
import score_star_reference as XR

STAR_SCORES = (0.0, -0.25, -0.5, -2.0)


def star_case(rng, k, Tmax=13, stars=True):
    """(x, labels, blank, star_score): V in 3..8, T <= Tmax, labels that fit their frames, stars planted at random (never two in
    a row)"""
    V = int(rng.integers(3, 9))
    blank = int(rng.integers(0, V)) if k % 3 else 0
    pool = [v for v in range(V) if v != blank]
    T = int(rng.integers(1, Tmax + 1))
    U = int(rng.integers(0, max(1, T // 2) + 1))
    lab = [int(v) for v in rng.choice(pool, U)]
    for i in range(1, U):
        if rng.random() < 0.3:
            lab[i] = lab[i - 1]
    if stars:
        for i in range(U):
            if rng.random() < 0.35 and (i == 0 or lab[i - 1] != V):
                lab[i] = V
        if U == 0 and T >= 1 and k % 2:
            lab = [V]
    while len(lab) + SR.repeats(lab) > T:
        lab.pop()
    x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
    return x, lab, blank, STAR_SCORES[k % 4]


def test_reference_against_brute_force():
    rng = np.random.default_rng(11)
    worst, with_star, above_zero = 0.0, 0, 0
    for k in range(60):
        V = int(rng.integers(2, 4))
        blank = int(rng.integers(0, V))
        pool = [v for v in range(V) if v != blank] + [V]
        T = int(rng.integers(1, 7))
        lab = []
        for _ in range(int(rng.integers(0, T + 1))):
            c = int(rng.choice(pool))
            if c == V and lab and lab[-1] == V:
                continue
            lab.append(c)
        x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
        ss = STAR_SCORES[k % 4]
        want = XR.brute_force(x, lab, blank, ss)
        got = XR.ctc_logp(x, lab, blank, ss)
        if T < len(lab) + SR.repeats(lab):
            assert got == -math.inf and want == -math.inf
            continue
        assert math.isfinite(want)
        worst = max(worst, abs(got - want))
        with_star += V in lab
        above_zero += got > 0
    assert worst < 1e-12, worst
    assert with_star >= 20 and above_zero >= 1              # a star's score is no log-probability


def test_star_free_labels_give_the_star_free_references():
    rng = np.random.default_rng(12)
    for k in range(80):
        x, lab, blank, ss = star_case(rng, k, stars=False)
        logp, Gam = XR.occupancy(x, lab, blank, ss)
        assert logp == SR.ctc_logp(x, lab, blank)
        logp2, Gam2 = GR.occupancy(x, lab, blank)
        assert logp == logp2 and np.array_equal(Gam, Gam2)
        a, b = XR.score_grad(x, [lab, lab[:1]], [1.5, -0.5], blank, ss), GR.score_grad(x, [lab, lab[:1]], [1.5, -0.5], blank)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_score_is_never_below_the_aligners():
    rng = np.random.default_rng(13)
    seen, single = 0, 0
    for k in range(120):
        x, lab, blank, ss = star_case(rng, k)
        logp = XR.ctc_logp(x, lab, blank, ss)
        score = AS.viterbi(x, lab, blank, ss)[3]
        assert math.isfinite(logp) and math.isfinite(score)
        if not lab or x.shape[0] == len(lab) + SR.repeats(lab):
            # U = 0 or T = U + R: ONE path, and the two references add its terms in different orders (sum_t (x_t - lse_t) against
            # sum_t x_t - sum_t lse_t): the same number up to rounding, so neither >= nor <= can be asked of the last bit
            assert abs(logp - score) <= SR.tau(x.shape[0], score), (k, logp, score)
            single += 1
        else:
            assert logp >= score, (k, logp, score)
        seen += x.shape[1] in lab
    assert seen >= 40 and 0 < single < 40


def finite_difference(x, lab, blank, ss, h=1e-6):
    """central differences of logp in fp64, with the star's emission and the top token held as the definition states them: the
    logits are perturbed in fp64, so the reference is evaluated on an fp64 copy of its own formulae"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    T, V = x64.shape

    def logp(z):
        m = z.max(axis=1, keepdims=True)
        ls = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]
        lp = np.concatenate([z, m + np.float64(np.float32(ss))], axis=1) - ls[:, None]
        U = len(lab)
        S = 2 * U + 1
        ext = np.full(S, blank, np.int64)
        ext[1::2] = lab
        alpha = np.full(S, -np.inf)
        alpha[0] = lp[0, blank]
        if U:
            alpha[1] = lp[0, lab[0]]
        for t in range(1, T):
            new = np.full(S, -np.inf)
            for s in range(S):
                c = [alpha[s]]
                if s >= 1:
                    c.append(alpha[s - 1])
                if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                    c.append(alpha[s - 2])
                new[s] = SR._lse_stack([np.array([v]) for v in c])[0] + lp[t, ext[s]]
            alpha = new
        return alpha[0] if U == 0 else SR._lse_stack([alpha[S - 1:S], alpha[S - 2:S - 1]])[0]

    G = np.zeros((T, V))
    for t in range(T):
        for v in range(V):
            zp, zm = x64.copy(), x64.copy()
            zp[t, v] += h
            zm[t, v] -= h
            G[t, v] = (logp(zp) - logp(zm)) / (2 * h)
    return G


def test_gradient_against_finite_differences():
    rng = np.random.default_rng(14)              # a seed for which at most 5 % of the cases have a near-tie of the frame maximum
    cases, skipped, worst, with_star = 0, 0, 0.0, 0
    for k in range(100):
        x, lab, blank, ss = star_case(rng, k, Tmax=8)
        cases += 1
        top2 = np.sort(x.astype(np.float64), axis=1)[:, -2:]
        if (top2[:, 1] - top2[:, 0] < 1e-3).any():
            skipped += 1                         # the maximum's derivative jumps at a tie: no finite difference there
            continue
        logp, Gam = XR.occupancy(x, lab, blank, ss)
        assert math.isfinite(logp)
        _, G, _ = XR.score_grad(x, [lab], [1.0], blank, ss)
        assert np.abs(G.sum(axis=1)).max() < 1e-12           # every row of G sums to 0
        assert np.abs(Gam.sum(axis=1) - 1.0).max() < 1e-12   # sum_s gamma_t(s) = 1
        fd = finite_difference(x, lab, blank, ss)
        worst = max(worst, float(np.abs(G - fd).max()))
        with_star += x.shape[1] in lab
    assert skipped <= 0.05 * cases, (skipped, cases)
    assert with_star >= 30
    assert worst <= 1e-6, worst


def test_conventions():
    x = np.random.default_rng(15).standard_normal((5, 4)).astype(np.float32)
    V = 4
    assert math.isnan(XR.ctc_logp(x, [V + 1], 0)) and math.isnan(XR.ctc_logp(x, [0], 0)) and math.isnan(XR.ctc_logp(x, [-1], 0))
    assert XR.ctc_logp(x[:4], [V, 1, 1, V], 0) == -math.inf                # T = 4 < U + R = 5: the star counts as a label
    assert math.isfinite(XR.ctc_logp(x, [V, 1, 1, V], 0))                  # T = U + R exactly
    assert math.isfinite(XR.ctc_logp(x, [V, 1, V], 0))
    assert math.isfinite(XR.ctc_logp(x[:1], [V], 0, -0.5))                 # a lone star on one frame
    xn = x.copy()
    xn[2, 1] = np.nan
    assert math.isnan(XR.ctc_logp(xn, [V], 0))
    # exact ties of the frame maximum: the star's occupancy lands on the lowest index
    xt = (np.round(x * 8) / 8).astype(np.float32)
    xt[1, 3] = xt[1, 2] = xt[1].max() + 0.125
    assert XR.top_token(xt)[1] == 2
    _, Gam = XR.occupancy(xt, [V], 0, 0.0)
    assert Gam[1, 2] > 0 and Gam[1, 3] == 0.0


def test_host_label_checks():
    from wav2vec2 import decoding as D
    V = 32
    with pytest.raises(ValueError, match=r"pair 0: labels must lie in \[0, 32\)"):
        D._check_score_labels([[3, V]], V, 0)                              # V without star_score
    assert D._check_score_labels([[3, V, 5], []], V, 0, star=True)[0].tolist() == [3, V, 5]
    with pytest.raises(ValueError, match="pair 1: two stars next to each other"):
        D._check_score_labels([[3], [3, V, V, 5]], V, 0, star=True)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 32\] \(32 is the star\)"):
        D._check_score_labels([[V + 1]], V, 0, star=True)
    with pytest.raises(ValueError, match="is the blank"):
        D._check_score_labels([[V, 0]], V, 0, star=True)
    with pytest.raises(ValueError, match="at most 8191"):
        D._check_score_labels([[V, 1] * 4096], V, 0, star=True)
    for bad in (0.25, float("nan")):
        with pytest.raises(ValueError, match="star_score"):
            D.ctc_score(None, None, star_score=bad)
        with pytest.raises(ValueError, match="star_score"):
            D.ctc_score_grad(None, None, None, star_score=bad)


class Tok:
    """a tokenizer with get_vocab(): A..Z from 5, "|" = 4, "<pad>" = 0; 31 entries, so the star is 31"""
    vocab = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, **{chr(65 + i): 5 + i for i in range(26)}}

    def get_vocab(self):
        return dict(self.vocab)

    def __call__(self, text):
        return [self.vocab[c] for c in text.upper().replace(" ", "|")]


def test_star_labels():
    from wav2vec2.losses import star_labels
    tok = Tok()
    V = len(tok.vocab)
    rows = star_labels(["* HELLO WORLD", "HI * YOU", "NO"], tok)
    assert rows.dtype == np.int32 and rows.shape == (3, 1 + len("HELLO WORLD"))
    assert rows[0].tolist() == [V] + tok("HELLO WORLD")
    assert rows[1].tolist() == tok("HI") + [V] + tok("YOU") + [0] * (rows.shape[1] - 6)
    assert rows[2].tolist() == tok("NO") + [0] * (rows.shape[1] - 2)
    ends = star_labels(["HI", "* HI"], tok, free_ends=True)
    assert ends.tolist() == [[V] + tok("HI") + [V]] * 2
    assert star_labels(["A # B"], tok, star="#").tolist() == [tok("A") + [V] + tok("B")]
    assert star_labels([[5, 40, 6]], None, vocab_size=40, pad_id=0).tolist() == [[5, 40, 6]]
    assert star_labels([""], tok).tolist() == [[0]]
    with pytest.raises(ValueError, match="two stars next to each other"):
        star_labels(["A * * B"], tok)
    with pytest.raises(ValueError, match="list of transcripts"):
        star_labels("A * B", tok)
    with pytest.raises(ValueError, match="vocab_size"):
        star_labels([[5, 6]], None)


def test_star_ctc_loss_arguments():
    from types import SimpleNamespace
    from wav2vec2.losses import StarCTCLoss
    cfg = SimpleNamespace(kernal_sizes=[10, 3], strides=[5, 2], pad_id=0)
    loss = StarCTCLoss(cfg, (1, 400), division_factor=2)
    assert loss.star_score == -0.5 and loss.pad_id == 0 and loss.division_factor == 2
    assert StarCTCLoss(cfg, (1, 400), star_score=0).star_score == 0.0
    for bad in (0.5, float("nan")):
        with pytest.raises(ValueError, match="star_score"):
            StarCTCLoss(cfg, (1, 400), star_score=bad)
    with pytest.raises(ValueError, match="division_factor"):
        StarCTCLoss(cfg, (1, 400), division_factor=0)


def test_c_abi_table_and_header_name_the_star_entry_points():
    import os
    from wav2vec2 import _native as N
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "w2v2.h")).read()
    for name, extra in (("w2v2_ctc_score_star", "w2v2_ctc_score"), ("w2v2_ctc_score_grad_star", "w2v2_ctc_score_grad")):
        assert name + "(" in header
        res, args = N.PROTOTYPES[name]
        res0, args0 = N.PROTOTYPES[extra]
        assert res is res0 and len(args) == len(args0) + 1 and args[:11] == args0[:11] and args[12:] == args0[11:]
        import ctypes
        assert args[11] is ctypes.c_float                                  # star_score after blank
    assert "w2v2_ctc_score_grad_star_workspace(" in header
    assert N.PROTOTYPES["w2v2_ctc_score_grad_star_workspace"] == N.PROTOTYPES["w2v2_ctc_score_grad_workspace"]
