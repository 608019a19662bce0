"""Exact CTC scoring with a star and its gradient on the GPU (w2v2_ctc_score_star, w2v2_ctc_score_grad_star,
wav2vec2.decoding.ctc_score / ctc_score_grad with ``star_score``, wav2vec2.losses.StarCTCLoss, model.score(star=...))
against the fp64 numpy reference (tests/score_star_reference.py): every thread layout with stars at the edges of a thread's pairs,
the edges of the recursion, exact ties of the frame maximum, -inf and NaN logits, the bits of the star-free entry points,
determinism, workspace groups, the aligner's score as a lower bound, refusals, and the loss and model entry points.

Tolerances (derived, not measured): logp within score_reference.tau, the gradient within score_grad_reference.bar.  The star adds one
fp64 add of two fp32 values, xs_t = (double)m_t + (double)star_score, which the reference performs identically, so neither bound
gets an extra term."""

import math
import os
import types

import numpy as np
import pytest

import align_star_reference as AS
import helpers as H
import score_grad_reference as GR
import score_reference as SR
import score_star_reference as XR

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits64(a):
    return np.asarray(a, np.float64).view(np.int64)


def bits32(t):
    return t.cpu().numpy().view(np.int32)


def check_logp(got, ref, T, what=""):
    """one logp against the reference: exact for -inf / NaN, score_reference.tau otherwise; returns |error| / tau"""
    if math.isnan(ref):
        assert math.isnan(got), (what, got, ref)
        return 0.0
    if ref == -math.inf:
        assert got == -math.inf, (what, got, ref)
        return 0.0
    r = abs(got - ref) / SR.tau(T, ref)
    print(f"{what}: logp {got!r} reference {ref!r} |error| / tau = {r:.4f}")
    assert r <= 1.0, (what, got, ref, r)
    return r


def check_grad(got, x, pairs, coef, blank, star_score, what=""):
    """one utterance's rows against the reference; returns (largest |error| / bar, the reference's logp)"""
    logp, G, slack = XR.score_grad(x, pairs, coef, blank, star_score)
    got = np.asarray(got, np.float64)
    assert got.shape == G.shape, (what, got.shape, G.shape)
    assert np.isfinite(got).all(), what
    if slack == 0.0:
        assert (got == 0).all(), (what, "no pair contributes: zeros")
        return 0.0, logp
    ratio = np.abs(got - G) / GR.bar(G, slack)
    print(f"{what}: gradient largest |error| / bar = {float(ratio.max()):.4f}")
    assert ratio.max() <= 1.0, (what, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return float(ratio.max()), logp


def random_labels(rng, U, V, blank, repeat_p=0.3):
    pool = [v for v in range(V) if v != blank]
    lab = rng.choice(pool, U) if U else np.zeros(0, np.int64)
    for k in range(1, U):
        if rng.random() < repeat_p:
            lab[k] = lab[k - 1]
    return lab.astype(np.int64)


def pairs_per_thread(U):
    return 1 if U + 1 <= 256 else 2 if U + 1 <= 512 else 4 if U + 1 <= 1024 else 8


# ---- 1. every thread layout, stars at the edges of a thread's pairs ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_cases():
    """per (U, V): logits, the star labels, the star-free labels they were planted in; T = U + R + 3"""
    out = {}
    for U in (255, 256, 511, 512, 1023, 1024, 2049):
        for V in (32, 400):
            rng = np.random.default_rng(1000 * V + U)
            P = pairs_per_thread(U)
            plain = random_labels(rng, U, V, 0, 0.15)
            lab = plain.copy()
            between = 20 * P + 2
            lab[between - 1] = lab[between + 1]                  # a star between equal labels
            for k in (0, 5 * P, 8 * P - 1, between, U - 1):      # label 0, a thread's first and last pair, label U - 1
                lab[k] = V
            assert not ((lab[1:] == V) & (lab[:-1] == V)).any()
            T = U + SR.repeats(lab) + 3
            x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
            out[U, V] = (x, lab, plain)
    return out


@pytest.mark.parametrize("V", [32, 400])
@pytest.mark.parametrize("U", [255, 256, 511, 512, 1023, 1024, 2049])
def test_thread_layouts(torch_mod, layout_cases, U, V):
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    x, lab, plain = layout_cases[U, V]
    T = x.shape[0]
    ss = -0.5
    part = dev(torch_mod, x)
    # utterance 0 carries the star pair, utterance 1 (the same rows) the star-free pair: one call mixes both
    coef = [0.7, -1.3]
    logp, grad = ctc_score_grad([part, part.clone()], [lab, plain], coef, star_score=ss)
    np.testing.assert_array_equal(bits64(logp), bits64(ctc_score([part, part], [lab, plain], star_score=ss)))
    e, ref_lp = check_grad(grad[0].cpu().numpy(), x, [lab], coef[:1], 0, ss, f"U = {U}, V = {V}")
    check_logp(float(logp[0]), float(ref_lp[0]), T, f"U = {U}, V = {V}")
    # the star-free pair of the mixed call carries the bits of the star-free entry points
    lp0, g0 = ctc_score_grad([part], [plain], coef[1:])
    np.testing.assert_array_equal(bits64(logp[1:]), bits64(lp0))
    np.testing.assert_array_equal(bits64(logp[1:]), bits64(ctc_score([part], [plain])))
    np.testing.assert_array_equal(bits32(grad[1]), bits32(g0[0]))
    # T = U + R exactly, and one frame less (infeasible)
    R = SR.repeats(lab)
    lp2 = ctc_score([part[:U + R], part[:U + R - 1]], [lab, lab], star_score=ss)
    check_logp(float(lp2[0]), XR.ctc_logp(x[:U + R], lab, 0, ss), U + R, f"U = {U}, V = {V}, T = U + R")
    assert math.isfinite(lp2[0]) and lp2[1] == -math.inf
    lp3, g3 = ctc_score_grad([part[:U + R - 1]], [lab], [1.0], star_score=ss)
    assert lp3[0] == -math.inf and (g3[0].cpu().numpy() == 0).all()


# ---- 2. the edges of the recursion ---------------------------------------------------------------------------------------------------------
def test_edges(torch_mod):
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    rng = np.random.default_rng(11)
    V = 5
    S = V                                                     # the star
    cases = [(1, [S]), (1, []), (2, [S]), (9, [S]), (3, [S, 1, S]), (2, [S, 1, S]), (7, [1, 1, S, 2, 2]), (6, [1, 1, S, 2, 2]),
             (5, [1, S, 1, S, 1]), (4, [1, S, 1, S, 1]), (6, [2, S, 2]), (1, [S, 2]), (8, [3, 4, S])]
    xs = [(rng.standard_normal((T, V)) * 2).astype(np.float32) for T, _ in cases]
    coef = rng.standard_normal(len(cases)) * 1.5
    worst = 0.0
    for blank, ss in ((0, -0.5), (4, 0.0), (0, -2.0)):
        labs = [[l if l == S else ((l % 4) + 1 if blank == 0 else l % 4) for l in lab] for _, lab in cases]
        parts = [dev(torch_mod, x) for x in xs]
        logp, grad = ctc_score_grad(parts, labs, coef, blank=blank, star_score=ss)
        assert logp.dtype == np.float64 and logp.shape == (len(cases),) and len(grad) == len(cases)
        np.testing.assert_array_equal(bits64(logp), bits64(ctc_score(parts, labs, blank=blank, star_score=ss)))
        for k, (g, x, lab) in enumerate(zip(grad, xs, labs)):
            assert g.dtype == torch_mod.float32 and tuple(g.shape) == x.shape
            e, ref_lp = check_grad(g.cpu().numpy(), x, [lab], [coef[k]], blank, ss, (cases[k], blank, ss))
            check_logp(float(logp[k]), float(ref_lp[0]), x.shape[0], (cases[k], blank, ss))
            worst = max(worst, e)
        assert math.isfinite(logp[0])                                                   # a lone star at T = 1
        assert math.isfinite(logp[4]) and logp[5] == -math.inf                          # T = U + R, and one frame less
        assert math.isfinite(logp[6]) and logp[7] == -math.inf and (grad[7].cpu().numpy() == 0).all()
        assert math.isfinite(logp[8]) and logp[9] == -math.inf and logp[11] == -math.inf
    print(f"edges: largest |error| / bar = {worst:.4f}")


# ---- 3. exact ties of the frame maximum: the gradient lands on the lowest index -----------------------------------------------------------
def test_ties_land_on_the_lowest_index(torch_mod):
    from wav2vec2.decoding import ctc_score_grad
    rng = np.random.default_rng(31)
    T, V = 24, 70                                                # columns beyond one wave's 64 lanes
    x = (np.round(rng.standard_normal((T, V)) * 8) / 8).astype(np.float32)
    lows, highs = [], []
    for t in range(T):
        lo, hi = sorted(int(v) for v in rng.choice(np.arange(10, V), 2, replace=False))
        if t % 3 == 0:
            lo, hi = lo % 6 + 58, 64 + hi % 6                    # the tie straddles the lanes' second round
        x[t, lo] = x[t, hi] = x[t].max() + 0.125
        lows.append(lo)
        highs.append(hi)
    assert (XR.top_token(x) == np.asarray(lows)).all()
    lab = [1, V, 2, V, 3]                                        # labels below column 10: the tied columns belong to no label
    for ss in (0.0, -0.5):
        logp, grad = ctc_score_grad([dev(torch_mod, x)], [lab], [1.0], star_score=ss)
        g = grad[0].cpu().numpy()
        e, ref_lp = check_grad(g, x, [lab], [1.0], 0, ss, f"ties, star_score {ss}")
        check_logp(float(logp[0]), float(ref_lp[0]), T, f"ties, star_score {ss}")
        _, Gam = XR.occupancy(x, lab, 0, ss)
        rows = np.arange(T)
        occ = Gam[rows, lows]                                    # the star's occupancy: no label emits these columns
        assert occ.max() > 0.5
        # the two tied columns have the same y: the star's whole occupancy separates them, on the lower index
        diff = g[rows, lows].astype(np.float64) - g[rows, highs].astype(np.float64)
        assert np.abs(diff - occ).max() <= 2.0 ** -22
        assert (g[rows, highs] <= 0).all() and (Gam[rows, highs] == 0).all()


# ---- 4. -inf and NaN logits -----------------------------------------------------------------------------------------------------------------
def test_nonfinite_logits(torch_mod):
    from wav2vec2.decoding import ctc_score_grad
    rng = np.random.default_rng(51)
    V = 8
    xs = [(rng.standard_normal((T, V)) * 2).astype(np.float32) for T in (40, 30, 30, 25)]
    xs[1][7, 5] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][:, 6] = -np.inf                                        # legal: label 6 can never be emitted; the star ignores the column
    xs[3][4, 3] = -np.inf
    utt = [0, 1, 1, 2, 3, 3, 3, 3]
    labs = [[1, V, 3], [1, V], [V], [V, 3], [1, V, 3], [1, 6, V], [V], [3, V, 3]]
    coef = np.asarray([0.5, 1.0, -1.0, 2.0, -0.7, 3.0, 0.9, -1.1])
    parts = [dev(torch_mod, x) for x in xs]
    logp, grad = ctc_score_grad(parts, labs, coef, utterance=utt, star_score=-0.5)
    worst = 0.0
    for i, x in enumerate(xs):
        mine = [j for j, u in enumerate(utt) if u == i]
        e, ref_lp = check_grad(grad[i].cpu().numpy(), x, [labs[j] for j in mine], coef[mine], 0, -0.5, f"utterance {i}")
        for j, r in zip(mine, ref_lp):
            check_logp(float(logp[j]), float(r), x.shape[0], f"pair {j}")
        worst = max(worst, e)
    assert np.isnan(logp[[1, 2, 3]]).all() and logp[5] == -math.inf and np.isfinite(logp[[0, 4, 6, 7]]).all()
    assert (grad[1].cpu().numpy() == 0).all() and (grad[2].cpu().numpy() == 0).all()
    assert (grad[3].cpu().numpy()[:, 6] == 0).all()              # y = 0 and no state there
    # the NaN utterances leave the good ones' bits unchanged
    lp2, g2 = ctc_score_grad([parts[0], parts[3]], [labs[j] for j in (0, 4, 5, 6, 7)], coef[[0, 4, 5, 6, 7]], utterance=[0, 1, 1, 1, 1],
                             star_score=-0.5)
    np.testing.assert_array_equal(bits64(lp2), bits64(logp[[0, 4, 5, 6, 7]]))
    for a, b in zip(g2, (grad[0], grad[3])):
        np.testing.assert_array_equal(bits32(a), bits32(b))
    print(f"non-finite logits: largest |error| / bar = {worst:.4f}")


# ---- 5. the star-free bits, determinism, workspace groups ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(21)
    Ts, V = [50, 7, 333, 128, 700, 90], 32
    xs = [(rng.standard_normal((T, V)) * 3).astype(np.float32) for T in Ts]
    utt = [0, 0, 1, 2, 2, 2, 3, 4, 4, 5, 0]
    labs = [random_labels(rng, int(rng.integers(0, Ts[i] // 2 + 1)), V, 0) for i in utt]
    labs[7] = random_labels(rng, 300, V, 0, 0.05)                # a pair of another thread layout in the same call
    starred = [l.copy() for l in labs]
    for j in (0, 3, 5, 7, 9):                                    # utterances 1 and 3 and pairs 1, 4, 10 stay star-free
        if starred[j].size == 0:
            starred[j] = np.asarray([V], np.int64)
        starred[j][::7] = V
    coef = rng.standard_normal(len(utt))
    return types.SimpleNamespace(Ts=Ts, V=V, xs=xs, utt=utt, labs=labs, starred=starred, coef=coef)


def test_star_free_bits_and_determinism(torch_mod, mixed):
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    m = mixed
    parts = [dev(torch_mod, x) for x in m.xs]
    # the star entry points on star-free labels: the bits of the star-free entry points
    logp0, grad0 = ctc_score_grad(parts, m.labs, m.coef, utterance=m.utt)
    logp1, grad1 = ctc_score_grad(parts, m.labs, m.coef, utterance=m.utt, star_score=-0.5)
    np.testing.assert_array_equal(bits64(logp1), bits64(logp0))
    np.testing.assert_array_equal(bits64(ctc_score(parts, m.labs, utterance=m.utt, star_score=-0.5)), bits64(logp0))
    np.testing.assert_array_equal(bits64(ctc_score(parts, m.labs, utterance=m.utt)), bits64(logp0))
    for a, b in zip(grad1, grad0):
        np.testing.assert_array_equal(bits32(a), bits32(b))
    # a call that mixes star and star-free pairs: the star-free pairs and the utterances without a star keep those bits
    logp2, grad2 = ctc_score_grad(parts, m.starred, m.coef, utterance=m.utt, star_score=-0.5)
    free = [j for j in range(len(m.utt)) if not (m.starred[j] == m.V).any()]
    assert 0 < len(free) < len(m.utt)
    np.testing.assert_array_equal(bits64(logp2[free]), bits64(logp0[free]))
    np.testing.assert_array_equal(bits64(ctc_score(parts, m.starred, utterance=m.utt, star_score=-0.5)), bits64(logp2))
    for i in (1, 3):
        np.testing.assert_array_equal(bits32(grad2[i]), bits32(grad0[i]))
    worst = 0.0
    for i, x in enumerate(m.xs):
        mine = [j for j, u in enumerate(m.utt) if u == i]
        e, ref_lp = check_grad(grad2[i].cpu().numpy(), x, [m.starred[j] for j in mine], m.coef[mine], 0, -0.5, f"mixed utterance {i}")
        for j, r in zip(mine, ref_lp):
            check_logp(float(logp2[j]), float(r), x.shape[0], f"mixed pair {j}")
        worst = max(worst, e)
    print(f"mixed call: largest |error| / bar = {worst:.4f}")
    # twice
    logp3, grad3 = ctc_score_grad(parts, m.starred, m.coef, utterance=m.utt, star_score=-0.5)
    np.testing.assert_array_equal(bits64(logp3), bits64(logp2))
    for a, b in zip(grad3, grad2):
        np.testing.assert_array_equal(bits32(a), bits32(b))
    # another star_score moves the star pairs only
    logp4 = ctc_score(parts, m.starred, utterance=m.utt, star_score=-1.0)
    np.testing.assert_array_equal(bits64(logp4[free]), bits64(logp0[free]))
    assert all(logp4[j] < logp2[j] for j in range(len(m.utt)) if j not in free)


def test_workspace_groups(torch_mod, mixed):
    from wav2vec2 import _native as N
    from wav2vec2.decoding import ctc_score_grad
    m = mixed
    lib = N.load()
    parts = [dev(torch_mod, x) for x in m.xs]
    logp, grad = ctc_score_grad(parts, m.starred, m.coef, utterance=m.utt, star_score=-0.5)
    nlab = np.asarray([len(l) for l in m.starred], np.int32)
    Ts_h, utt_h = np.asarray(m.Ts, np.int32), np.asarray(m.utt, np.int32)
    whole = lib.w2v2_ctc_score_grad_star_workspace(len(m.Ts), N.ptr(Ts_h), len(nlab), N.ptr(utt_h), N.ptr(nlab), m.V)
    plain = lib.w2v2_ctc_score_grad_workspace(len(m.Ts), N.ptr(Ts_h), len(nlab), N.ptr(utt_h), N.ptr(nlab), m.V)
    frames = int(Ts_h.sum())
    up = lambda b: (b + 255) & ~255
    assert whole == plain + up(8 * frames) + up(4 * frames)                      # the xs and a arrays
    alone = []
    for i in range(len(m.Ts)):
        mine = np.flatnonzero(utt_h == i)
        one, zero, nl = Ts_h[i:i + 1].copy(), np.zeros(len(mine), np.int32), np.ascontiguousarray(nlab[mine])
        alone.append(lib.w2v2_ctc_score_grad_star_workspace(1, N.ptr(one), len(mine), N.ptr(zero), N.ptr(nl), m.V))
    assert whole > max(alone) > 0
    for cap in (max(alone), max(alone) + min(alone) + 4096):                     # one utterance per group; some groups of two
        assert cap < whole
        lp2, g2 = ctc_score_grad(parts, m.starred, m.coef, utterance=m.utt, star_score=-0.5, max_workspace_bytes=cap)
        np.testing.assert_array_equal(bits64(lp2), bits64(logp))
        for a, b in zip(g2, grad):
            np.testing.assert_array_equal(bits32(a), bits32(b))
    worst = int(np.argmax(alone))
    with pytest.raises(MemoryError, match=f"utterance {worst} "):
        ctc_score_grad(parts, m.starred, m.coef, utterance=m.utt, star_score=-0.5, max_workspace_bytes=max(alone) - 1)


# ---- 6. never below the aligner's score ---------------------------------------------------------------------------------------------------
def test_score_is_never_below_the_aligners(torch_mod, layout_cases):
    from wav2vec2.alignment import forced_align
    from wav2vec2.decoding import ctc_score
    rng = np.random.default_rng(61)
    V = 32
    xs, labs = [], []
    for T in (1, 9, 40, 200, 333):
        x = (rng.standard_normal((T, V)) * 3).astype(np.float32)
        lab = random_labels(rng, min(T, int(rng.integers(1, T // 2 + 2))), V, 0, 0.1)
        lab[::5] = V
        xs.append(x)
        labs.append(lab)
    x, lab, _ = layout_cases[511, 32]
    xs.append(x)
    labs.append(lab)
    parts = [dev(torch_mod, x) for x in xs]
    for ss in (0.0, -0.5, -2.0):
        logp = ctc_score(parts, labs, star_score=ss)
        al = forced_align(parts, labs, star_score=ss)
        for k, (lp, a) in enumerate(zip(logp, al)):
            assert math.isfinite(lp) and math.isfinite(a.score)
            if len(labs[k]) == 0 or xs[k].shape[0] == len(labs[k]) + SR.repeats(labs[k]):      # one path: the same number, added in another order
                assert abs(lp - a.score) <= SR.tau(xs[k].shape[0], a.score), (k, ss, lp, a.score)
            else:
                assert lp >= a.score, (k, ss, lp, a.score)
            ref = AS.viterbi(xs[k], labs[k], 0, ss)[3]
            assert abs(a.score - ref) <= SR.tau(xs[k].shape[0], ref)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    lib = N.load()
    V = 8
    x = dev(torch, np.random.default_rng(71).standard_normal((2, 10, V)).astype(np.float32))
    for bad in (0.25, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="star_score"):
            ctc_score(x, [[1], [2]], star_score=bad)
        with pytest.raises(ValueError, match="star_score"):
            ctc_score_grad(x, [[1], [2]], [1.0, 1.0], star_score=bad)
    with pytest.raises(ValueError, match=r"pair 1: labels must lie in \[0, 8\)"):
        ctc_score(x, [[1], [2, V]])                              # the star's id without star_score
    with pytest.raises(ValueError, match=r"pair 1: labels must lie in \[0, 8\)"):
        ctc_score_grad(x, [[1], [2, V]], [1.0, 1.0])
    with pytest.raises(ValueError, match=r"pair 0: labels must lie in \[0, 8\] \(8 is the star\)"):
        ctc_score(x, [[V + 1], [2]], star_score=-0.5)
    with pytest.raises(ValueError, match="pair 1: two stars next to each other"):
        ctc_score_grad(x, [[1], [2, V, V]], [1.0, 1.0], star_score=-0.5)
    with pytest.raises(ValueError, match="is the blank"):
        ctc_score(x, [[V, 0], [2]], star_score=-0.5)
    assert np.isfinite(ctc_score(x, [[V], [2, V]], star_score=0)).all()          # 0 is a legal star_score

    # the C ABI: star_score NaN or > 0 is refused before any launch; labels on the device are checked by the kernel (NaN)
    base = x.reshape(20, V)
    lab = torch.tensor([1, V, 2, 0, V + 1, 3, V, V, -1, 1, 1], dtype=torch.int32, device="cuda")
    label0 = np.asarray([0, 3, 4, 6, 8, 9], np.int64)
    nlab = np.asarray([3, 1, 2, 2, 1, 2], np.int32)              # [1 V 2] [0: the blank] [V+1 3] [V V] [-1] [1 1]
    utt = np.asarray([0, 0, 1, 1, 0, 1], np.int32)
    row0, frames = np.asarray([0, 10], np.int64), np.asarray([10, 10], np.int32)
    coef = torch.ones(6, dtype=torch.float64, device="cuda")
    logp = torch.full((6,), -7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((20, V), -7.5, device="cuda")

    def score(ss, out):
        return lib.w2v2_ctc_score_star(N.ptr(base), V, 2, N.ptr(row0), N.ptr(frames), 6, N.ptr(utt), N.ptr(lab), N.ptr(label0),
                                       N.ptr(nlab), 0, ss, N.ptr(out), N.current_stream())

    def score_grad(ss, cap=0, V_=V, m=6):
        return lib.w2v2_ctc_score_grad_star(N.ptr(base), V_, 2, N.ptr(row0), N.ptr(frames), m, N.ptr(utt), N.ptr(lab), N.ptr(label0),
                                            N.ptr(nlab), 0, ss, N.ptr(coef), N.ptr(logp), N.ptr(grad), cap, N.current_stream())

    for ss in (0.25, float("nan"), float("inf")):
        assert score(ss, logp) == -1 and "star_score" in N.last_error()
        assert score_grad(ss) == -1 and "star_score" in N.last_error()
    assert score_grad(-0.5, cap=-1) == -1 and score_grad(-0.5, cap=64) == -1 and score_grad(-0.5, V_=1) == -1 and score_grad(-0.5, m=0) == -1
    assert lib.w2v2_ctc_score_star(None, V, 2, N.ptr(row0), N.ptr(frames), 6, N.ptr(utt), N.ptr(lab), N.ptr(label0), N.ptr(nlab), 0, -0.5,
                                   N.ptr(logp), N.current_stream()) == -1
    assert lib.w2v2_ctc_score_grad_star_workspace(0, N.ptr(frames), 6, N.ptr(utt), N.ptr(nlab), V) == -1
    torch.cuda.synchronize()
    assert (logp == -7.0).all() and (grad == -7.5).all()         # nothing launched, nothing written
    out = torch.full((6,), -7.0, dtype=torch.float64, device="cuda")
    assert score(-0.5, out) == 0 and score_grad(-0.5) == 0
    torch.cuda.synchronize()
    got, got2 = out.cpu().numpy(), logp.cpu().numpy()
    np.testing.assert_array_equal(bits64(got), bits64(got2))
    assert math.isfinite(got[0]) and np.isnan(got[[1, 2, 4]]).all() and math.isfinite(got[5])
    assert math.isfinite(got[3])                                 # two stars in a row are the host's refusal; the kernel counts a repeat
    assert torch.isfinite(grad).all()


# ---- 8. the loss and the model -----------------------------------------------------------------------------------------------------------
def test_star_ctc_loss(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import ctc_score_grad
    from wav2vec2.losses import CTCLoss, StarCTCLoss
    rng = np.random.default_rng(77)
    B, T, V, Umax = 4, 64, 32, 20
    x = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    labels = np.zeros((B, Umax), np.int64)
    plain = []
    for b in range(B):
        lab = random_labels(rng, int(rng.integers(3, Umax + 1)), V, 0)
        labels[b, :lab.size] = lab
        plain.append(lab)
    cfg = types.SimpleNamespace(kernal_sizes=[], strides=[], pad_id=0)
    xd = dev(torch, x)
    # star-free labels: the CTC loss, its gradient as DESIGN.md §23 states it, and ctc_score_grad's bits
    loss = StarCTCLoss(cfg, (B, T))
    nll, grad, total = loss.per_sample(labels, xd, with_grad=True, with_total=True)
    nll0, want = CTCLoss(cfg, (B, T)).per_sample(labels, xd, with_grad=True)
    lp0, g0 = ctc_score_grad(xd, plain, [-1.0] * B)
    np.testing.assert_array_equal(bits32(grad), bits32(g0))
    np.testing.assert_array_equal(nll.cpu().numpy(), (-lp0).astype(np.float32))
    diff = float((grad - want).abs().max())
    print(f"against w2v2_ctc_loss: largest gradient difference {diff:.3e}")
    assert float(want.abs().max()) > 0.1 and diff <= 2e-5
    assert float(total) == np.float32(-lp0.sum())
    # with stars: the hand-composed ctc_score_grad call, with the division and explicit frame lengths
    starred = labels.copy()
    starred[0, 0] = V
    starred[1, 2] = V
    starred[3, 1] = starred[3, 5] = V
    rows = [[int(v) for v in r if v != 0] for r in starred]
    lens = [64, 50, 33, 64]
    loss2 = StarCTCLoss(cfg, (B, T), division_factor=4, star_score=-0.25)
    nll2, grad2, total2 = loss2.per_sample(torch.as_tensor(starred), xd, with_grad=True, with_total=True, frame_lengths=lens)
    lp, g = ctc_score_grad(xd, rows, [-0.25] * B, frame_lengths=lens, star_score=-0.25)
    np.testing.assert_array_equal(bits32(grad2), bits32(g))
    np.testing.assert_array_equal(nll2.cpu().numpy(), (-lp).astype(np.float32))
    assert float(total2) == np.float32(-lp.sum() / 4.0) and float(loss2.last_total) == float(total2)
    assert (grad2[1, 50:] == 0).all() and (grad2[2, 33:] == 0).all()
    for b in range(B):
        check_grad(grad2[b, :lens[b]].cpu().numpy(), x[b, :lens[b]], [rows[b]], [-0.25], 0, -0.25, f"loss row {b}")
    only = loss2.per_sample(starred, xd, frame_lengths=lens)
    np.testing.assert_array_equal(only.cpu().numpy(), nll2.cpu().numpy())
    full = StarCTCLoss(cfg, (B, T), division_factor=4, star_score=-0.25)
    tot = float(full(starred, xd))
    ref = sum(-XR.ctc_logp(x[b], rows[b], 0, -0.25) for b in range(B)) / 4.0
    assert abs(tot - ref) <= 2.0 ** -22 * abs(ref)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 32\]"):
        loss2.per_sample(np.full((B, 3), V + 1), xd)


def test_trainer_step_on_star_ctc_loss(torch_mod):
    import wav2vec2
    g = H.golden("tiny_base")
    x, labels = g["wave"], np.asarray(g["labels"]).copy()
    cfg = H.case_config("tiny_base")
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(2, 4000))
    m.set_weights(H.case_weights("tiny_base"))
    m.freeze_feature_extractor()
    labels[0, 0] = cfg.vocab_size                                # a star at the head of the first transcript
    loss = wav2vec2.StarCTCLoss(cfg, x.shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss, learning_rate=1e-3, dropout=0.1, apply_spec_augment=False, seed=5)
    total = float(tr.step(x, labels))
    assert np.isfinite(total), total
    w0, w1 = H.case_weights("tiny_base"), m.get_weights()
    assert any(not np.array_equal(w1[n], w0[n]) for n in w1 if n in w0)          # the step moved something


def test_model_score_with_a_star(torch_mod):
    import wav2vec2
    from wav2vec2.alignment import star_transcript
    from wav2vec2.decoding import ctc_score
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    cfg = H.case_config("tiny_base")
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights("tiny_base"))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 24000)]
    logits = m.predict_packed(waves)
    V = cfg.vocab_size
    texts = ["* A", "HI * YOU", "THE CAT"]
    ids = [star_transcript(t, V, tok, "*") for t in texts]
    assert ids[0][0] == V and V in ids[1] and V not in ids[2]
    got = m.score(waves, texts, tok, star="*", star_score=-0.25)
    direct = ctc_score(logits, ids, blank=cfg.pad_id, star_score=-0.25)
    for (lp, per), d, l, lab in zip(got, direct, logits, ids):
        assert lp == d and per == d / int(l.shape[0])
        check_logp(lp, XR.ctc_logp(l.cpu().numpy(), lab, cfg.pad_id, -0.25), int(l.shape[0]), lab)
    assert m.score(waves, ids, star_score=-0.25) == got          # an id transcript that holds the star's id
    # free_ends, and the aligner's score below it
    ends = m.score(waves, texts, tok, star="*", free_ends=True)
    ids2 = [star_transcript(t, V, tok, "*", True) for t in texts]
    assert [v for v, _ in ends] == list(ctc_score(logits, ids2, blank=cfg.pad_id, star_score=-0.5))
    # without the star arguments nothing changes
    plain = m.score(waves, ["A", "HI", "THE CAT"], tok)
    assert [v for v, _ in plain] == list(ctc_score(logits, [list(tok(t)) for t in ("A", "HI", "THE CAT")], blank=cfg.pad_id))
    assert plain[2] == got[2]                                    # the star-free pair of the star call: the same bits
