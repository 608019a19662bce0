"""The gradient of weighted exact CTC log-probabilities on the GPU (w2v2_ctc_score_grad, wav2vec2.decoding.ctc_score_grad;
DESIGN.md §23) against the fp64 numpy reference (tests/score_grad_reference.py): the edges of the recursion, every thread layout, a
mixed call through the C ABI with shared rows, junk rows and a sentinel, workspace groups, the bits of the scorer, determinism and
isolation, the range of fp64 log space, -inf and NaN logits, the loss kernel's gradient, and the C ABI's refusals.

Tolerance (derived, not measured): |got - ref| <= 2^-23 |ref| + sum_j |c_j| * 4 * 16 T 2^-52 * max(1, |logp_j| + 40)
(score_grad_reference.bar); logp is compared as the score tests do (score_reference.tau; -inf and NaN exactly)."""

import math
import types

import numpy as np
import pytest

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


def check_logp(got, ref, T, what=""):
    """one logp against the reference: exact for -inf / NaN, score_reference.tau otherwise"""
    if math.isnan(ref):
        assert math.isnan(got), (what, got, ref)
    elif ref == -math.inf:
        assert got == -math.inf, (what, got, ref)
    else:
        assert abs(got - ref) <= SR.tau(T, ref), (what, got, ref, abs(got - ref) / SR.tau(T, ref))


def random_labels(rng, U, V, blank, repeat_p=0.3):
    pool = [v for v in range(V) if v != blank]
    lab = rng.choice(pool, U) if U else np.zeros(0, np.int64)
    for k in range(1, U):
        if rng.random() < repeat_p:
            lab[k] = lab[k - 1]
    return lab.astype(np.int64)


def check_grad(got, x, pairs, coef, blank, what=""):
    """one utterance's rows against the reference; returns the largest |error| / bar"""
    logp, G, slack = GR.score_grad(x, pairs, coef, blank)
    got = np.asarray(got, np.float64)
    assert got.shape == G.shape, (what, got.shape, G.shape)
    assert np.isfinite(got).all(), what
    if slack == 0.0:
        assert (got == 0).all(), (what, "no pair contributes: zeros")
        return 0.0, logp
    ratio = np.abs(got - G) / GR.bar(G, slack)
    assert ratio.max() <= 1.0, (what, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return float(ratio.max()), logp


def raw_grad(torch, base, V, row0, frames, utt, labs, coef, blank, cap=0, sentinel=-7.5, lead=5, expect_ok=True):
    """w2v2_ctc_score_grad through ctypes: (return code, logp, grad buffer prefilled with ``sentinel``)"""
    from wav2vec2 import _native as N
    flat = np.concatenate([np.full(lead, 10 ** 6, np.int32)] + [np.asarray(l, np.int32) for l in labs] + [np.zeros(1, np.int32)])
    label0 = (lead + np.cumsum([0] + [len(l) for l in labs[:-1]])).astype(np.int64)
    nlab = np.asarray([len(l) for l in labs], np.int32)
    lab_dev = torch.from_numpy(flat).cuda()
    coef_dev = torch.from_numpy(np.asarray(coef, np.float64)).cuda()
    logp = torch.full((len(labs),), -7.0, dtype=torch.float64, device="cuda")
    grad = torch.full(tuple(base.shape), sentinel, dtype=torch.float32, device="cuda")
    row0_h, frames_h, utt_h = np.asarray(row0, np.int64), np.asarray(frames, np.int32), np.asarray(utt, np.int32)
    rc = N.load().w2v2_ctc_score_grad(N.ptr(base), V, len(frames), N.ptr(row0_h), N.ptr(frames_h), len(labs), N.ptr(utt_h), N.ptr(lab_dev),
                                      N.ptr(label0), N.ptr(nlab), blank, N.ptr(coef_dev), N.ptr(logp), N.ptr(grad), cap, N.current_stream())
    if expect_ok:
        N.check(rc, "w2v2_ctc_score_grad")
    torch.cuda.synchronize()
    return rc, logp.cpu().numpy(), grad.cpu().numpy()


# ---- 1. the edges of the recursion, with gradients ----------------------------------------------------------------------------------
def test_edges(torch_mod):
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    rng = np.random.default_rng(11)
    cases = [(1, []), (9, []), (1, [3]), (2, [3]), (7, [1, 1, 2, 2, 3]), (6, [1, 1, 2, 2, 3]), (5, [1, 2, 3, 4, 1]), (4, [1, 2, 3, 4, 1]),
             (3, [2, 2]), (2, [2, 2]), (1, [1, 2])]
    xs = [(rng.standard_normal((T, 5)) * 2).astype(np.float32) for T, _ in cases]
    coef = rng.standard_normal(len(cases)) * 1.5
    worst = 0.0
    for blank in (0, 4):
        labs = [[(l % 4) + 1 if blank == 0 else l % 4 for l in lab] for _, lab in cases]
        parts = [dev(torch_mod, x) for x in xs]
        logp, grad = ctc_score_grad(parts, labs, coef, blank=blank)
        assert logp.dtype == np.float64 and logp.shape == (len(cases),) and len(grad) == len(cases)
        np.testing.assert_array_equal(logp, ctc_score(parts, labs, blank=blank))
        for k, (g, x, lab) in enumerate(zip(grad, xs, labs)):
            assert g.dtype == torch_mod.float32 and tuple(g.shape) == x.shape
            e, ref_lp = check_grad(g.cpu().numpy(), x, [lab], [coef[k]], blank, (cases[k], blank))
            check_logp(float(logp[k]), float(ref_lp[0]), x.shape[0], (cases[k], blank))
            worst = max(worst, e)
        assert math.isfinite(logp[4]) and logp[5] == -math.inf and (grad[5].cpu().numpy() == 0).all()      # T = U + R, and one frame less
    print(f"edges: largest |error| / bar = {worst:.4f}")


# ---- 2. every thread layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [255, 256, 511, 512, 1023, 1024, 2049])
def test_thread_layouts(torch_mod, U):
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    rng = np.random.default_rng(U)
    T, V = 2 * U + 3, 8
    x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
    lab = random_labels(rng, U, V, 0)
    short = lab[:U - 70]                                     # a second pair of the same utterance, in a smaller layout where one exists
    coef = [0.7, -1.3]
    part = dev(torch_mod, x)
    logp, grad = ctc_score_grad([part], [lab, short], coef, utterance=[0, 0])
    np.testing.assert_array_equal(logp.view(np.int64), ctc_score([part], [lab, short], utterance=[0, 0]).view(np.int64))     # (a) in every layout
    e, ref_lp = check_grad(grad[0].cpu().numpy(), x, [lab, short], coef, 0, U)
    check_logp(float(logp[0]), float(ref_lp[0]), T, U)
    check_logp(float(logp[1]), float(ref_lp[1]), T, (U, "short"))
    print(f"U = {U}: |error| / bar = {e:.4f}")


# ---- 3. a mixed call through the C ABI, and the same call in workspace groups -------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(torch_mod):
    rng = np.random.default_rng(101)
    V, blank, Ts = 32, 31, [3, 64, 129, 311]
    xs = [(rng.standard_normal((T, V)) * 4).astype(np.float32) for T in Ts]
    place = [2, 0, 3, 1]
    chunks, row0, at = [np.full((3, V), np.nan, np.float32)], [0] * 4, 3
    for i in place:
        row0[i] = at
        chunks += [xs[i], np.full((2, V), np.nan, np.float32)]
        at += Ts[i] + 2
    base = np.concatenate(chunks)
    pairs = [(0, random_labels(rng, 4 + k, V, blank)) for k in range(3)]         # utterance 0 (3 frames): no feasible pair
    for i in (1, 2, 3):
        for k in range(12):
            U = Ts[i] + 1 + k if k % 6 == 5 else int(rng.integers(0, Ts[i] // 2 + 1))      # some with too few frames
            pairs.append((i, random_labels(rng, U, V, blank)))
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    coef = rng.standard_normal(len(pairs))
    return types.SimpleNamespace(V=V, blank=blank, Ts=Ts, xs=xs, row0=row0, base=base, pairs=pairs, coef=coef,
                                 utt=[i for i, _ in pairs], labs=[l for _, l in pairs])


def test_mixed_call(torch_mod, mixed):
    m = mixed
    rc, logp, grad = raw_grad(torch_mod, dev(torch_mod, m.base), m.V, m.row0, m.Ts, m.utt, m.labs, m.coef, m.blank)
    inside = np.zeros(len(m.base), bool)
    worst, ninf = 0.0, 0
    for i, T in enumerate(m.Ts):
        inside[m.row0[i]:m.row0[i] + T] = True
        mine = [j for j, u in enumerate(m.utt) if u == i]
        e, ref_lp = check_grad(grad[m.row0[i]:m.row0[i] + T], m.xs[i], [m.labs[j] for j in mine], m.coef[mine], m.blank, i)
        for j, r in zip(mine, ref_lp):
            check_logp(float(logp[j]), float(r), T, j)
            ninf += r == -math.inf
        worst = max(worst, e)
    assert (grad[~inside] == -7.5).all()                                         # the junk rows keep the sentinel
    assert (grad[m.row0[0]:m.row0[0] + 3] == 0).all()                            # no feasible pair: zeros
    assert 3 < ninf < len(m.pairs) // 2
    print(f"mixed call: {len(m.pairs)} pairs, {ninf} infeasible, largest |error| / bar = {worst:.4f}")


def test_workspace_groups(torch_mod, mixed):
    from wav2vec2 import _native as N
    from wav2vec2.decoding import ctc_score_grad
    m = mixed
    lib = N.load()
    base = dev(torch_mod, m.base)
    _, logp, grad = raw_grad(torch_mod, base, m.V, m.row0, m.Ts, m.utt, m.labs, m.coef, m.blank)
    nlab = np.asarray([len(l) for l in m.labs], np.int32)
    Ts_h, utt_h = np.asarray(m.Ts, np.int32), np.asarray(m.utt, np.int32)
    whole = lib.w2v2_ctc_score_grad_workspace(4, N.ptr(Ts_h), len(m.labs), N.ptr(utt_h), N.ptr(nlab), m.V)
    alone = []
    for i in range(4):
        mine = np.flatnonzero(utt_h == i)
        one, zero, nl = Ts_h[i:i + 1].copy(), np.zeros(len(mine), np.int32), np.ascontiguousarray(nlab[mine])
        alone.append(lib.w2v2_ctc_score_grad_workspace(1, N.ptr(one), len(mine), N.ptr(zero), N.ptr(nl), m.V))
    assert whole > max(alone) > 0
    for cap in (max(alone), max(alone) + min(a for a in alone if a > 0) + 4096):           # one utterance per group; some groups of two
        assert cap < whole
        _, logp2, grad2 = raw_grad(torch_mod, base, m.V, m.row0, m.Ts, m.utt, m.labs, m.coef, m.blank, cap=cap)
        np.testing.assert_array_equal(logp2.view(np.int64), logp.view(np.int64))
        np.testing.assert_array_equal(grad2.view(np.int32), grad.view(np.int32))
    # a cap below one utterance's need: refused with nothing written, naming the utterance and the bytes
    rc, logp3, grad3 = raw_grad(torch_mod, base, m.V, m.row0, m.Ts, m.utt, m.labs, m.coef, m.blank, cap=max(alone) - 1, expect_ok=False)
    assert rc == -1 and (logp3 == -7.0).all() and (grad3 == -7.5).all()
    worst = int(np.argmax(alone))
    assert f"utterance {worst} " in N.last_error() and str(max(alone)) in N.last_error()
    parts = [dev(torch_mod, x) for x in m.xs]
    with pytest.raises(MemoryError, match=f"utterance {worst} "):
        ctc_score_grad(parts, m.labs, m.coef, blank=m.blank, utterance=m.utt, max_workspace_bytes=max(alone) - 1)
    lp4, g4 = ctc_score_grad(parts, m.labs, m.coef, blank=m.blank, utterance=m.utt, max_workspace_bytes=max(alone))
    np.testing.assert_array_equal(lp4.view(np.int64), logp.view(np.int64))
    for i, g in enumerate(g4):
        np.testing.assert_array_equal(g.cpu().numpy().view(np.int32), grad[m.row0[i]:m.row0[i] + m.Ts[i]].view(np.int32))


# ---- 4. the scorer's bits, determinism, isolation ---------------------------------------------------------------------------------------
def test_scorer_bits_determinism_isolation(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import ctc_score, ctc_score_grad
    rng = np.random.default_rng(21)
    Ts, V = [50, 7, 333, 128, 700, 90], 32
    xs = [(rng.standard_normal((T, V)) * 3).astype(np.float32) for T in Ts]
    utt = [0, 0, 1, 2, 2, 2, 3, 4, 4, 5, 0]
    labs = [random_labels(rng, int(rng.integers(0, Ts[i] // 2 + 1)), V, 0) for i in utt]
    labs[7] = random_labels(rng, 300, V, 0, 0.05)            # a pair of another thread layout in the same call
    coef = rng.standard_normal(len(utt))
    parts = [dev(torch, x) for x in xs]
    logp, grad = ctc_score_grad(parts, labs, coef, utterance=utt)
    grad = [g.cpu().numpy() for g in grad]
    assert np.isfinite(logp).all()
    # (a) the scorer's bits
    np.testing.assert_array_equal(logp.view(np.int64), ctc_score(parts, labs, utterance=utt).view(np.int64))
    # (b) twice
    logp2, grad2 = ctc_score_grad(parts, labs, coef, utterance=utt)
    np.testing.assert_array_equal(logp2.view(np.int64), logp.view(np.int64))
    for g, h in zip(grad, grad2):
        np.testing.assert_array_equal(h.cpu().numpy().view(np.int32), g.view(np.int32))
    # (c) each utterance alone, and in a padded buffer at another position with junk behind it and other neighbours
    for i in range(len(Ts)):
        mine = [j for j, u in enumerate(utt) if u == i]
        lp1, g1 = ctc_score_grad([parts[i]], [labs[j] for j in mine], coef[mine], utterance=[0] * len(mine))
        np.testing.assert_array_equal(lp1.view(np.int64), logp[mine].view(np.int64))
        np.testing.assert_array_equal(g1[0].cpu().numpy().view(np.int32), grad[i].view(np.int32))
    pad = rng.standard_normal((len(Ts), max(Ts), V)).astype(np.float32) * 50
    rev = list(range(len(Ts)))[::-1]
    for b, i in enumerate(rev):
        pad[b, :Ts[i]] = xs[i]
    keep = [j for j, u in enumerate(utt) if u != 3]           # utterance 3 loses its pair: zeros, the others unchanged
    lp3, g3 = ctc_score_grad(dev(torch, pad), [labs[j] for j in keep], coef[keep], frame_lengths=[Ts[i] for i in rev],
                             utterance=[rev.index(utt[j]) for j in keep])
    assert tuple(g3.shape) == pad.shape
    g3 = g3.cpu().numpy()
    np.testing.assert_array_equal(lp3.view(np.int64), logp[keep].view(np.int64))
    for b, i in enumerate(rev):
        assert (g3[b, Ts[i]:] == 0).all()
        if i == 3:
            assert (g3[b] == 0).all()
        else:
            np.testing.assert_array_equal(g3[b, :Ts[i]].view(np.int32), grad[i].view(np.int32))
    # a device coefficient tensor is the same call
    lp5, g5 = ctc_score_grad(parts, labs, dev(torch, coef), utterance=utt)
    np.testing.assert_array_equal(g5[4].cpu().numpy().view(np.int32), grad[4].view(np.int32))


# ---- 5. range, -inf and NaN logits ------------------------------------------------------------------------------------------------------
def test_range_and_nonfinite(torch_mod):
    from wav2vec2.decoding import ctc_score_grad
    z = np.zeros((40, 5), np.float32)
    z[:, 0] = 2000.0                                         # every label emission is e^-2000 (DESIGN.md §18's range case)
    logp, grad = ctc_score_grad([dev(torch_mod, z)], [[1, 2]], [-1.0])
    g = grad[0].cpu().numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 1e-3
    e, ref_lp = check_grad(g, z, [[1, 2]], [-1.0], 0, "range")
    check_logp(float(logp[0]), float(ref_lp[0]), 40)
    print(f"range case: |error| / bar = {e:.4f}")
    rng = np.random.default_rng(51)
    xs = [(rng.standard_normal((T, 8)) * 2).astype(np.float32) for T in (40, 30, 30, 25, 40)]
    xs[1][7, 5] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][:, 6] = -np.inf                                    # legal: label 6 can never be emitted
    xs[3][4, 3] = -np.inf
    utt = [0, 1, 1, 2, 3, 3, 3, 4, 2]
    labs = [[1, 2, 3], [1, 2], [], [3], [1, 2, 3], [1, 6, 2], [3, 3], [7, 7, 1], []]
    coef = np.asarray([0.5, 1.0, -1.0, 2.0, -0.7, 3.0, 0.9, -1.1, 0.3])
    parts = [dev(torch_mod, x) for x in xs]
    logp, grad = ctc_score_grad(parts, labs, coef, utterance=utt)
    worst = 0.0
    for i, x in enumerate(xs):
        mine = [j for j, u in enumerate(utt) if u == i]
        e, ref_lp = check_grad(grad[i].cpu().numpy(), x, [labs[j] for j in mine], coef[mine], 0, i)
        for j, r in zip(mine, ref_lp):
            check_logp(float(logp[j]), float(r), x.shape[0], j)
        worst = max(worst, e)
    assert np.isnan(logp[[1, 2, 3, 8]]).all() and logp[5] == -math.inf           # a used -inf column: -inf, a zero contribution
    assert (grad[1].cpu().numpy() == 0).all() and (grad[2].cpu().numpy() == 0).all()
    assert (grad[3].cpu().numpy()[:, 6] == 0).all()                             # y = 0 and no state there
    # the NaN utterances leave the good ones' bits unchanged
    lp2, g2 = ctc_score_grad([parts[0], parts[3], parts[4]], [labs[0], labs[4], labs[5], labs[6], labs[7]], coef[[0, 4, 5, 6, 7]],
                             utterance=[0, 1, 1, 1, 2])
    np.testing.assert_array_equal(lp2.view(np.int64), logp[[0, 4, 5, 6, 7]].view(np.int64))
    for a, b in zip(g2, (grad[0], grad[3], grad[4])):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    print(f"non-finite logits: largest |error| / bar = {worst:.4f}")


# ---- 6. against the loss kernel ---------------------------------------------------------------------------------------------------------
def test_against_ctc_loss_kernel(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import ctc_score_grad
    from wav2vec2.losses import CTCLoss
    rng = np.random.default_rng(77)
    B, T, V, Umax = 4, 64, 32, 20
    x = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    labels = np.zeros((B, Umax), np.int64)
    labs = []
    for b in range(B):
        lab = random_labels(rng, int(rng.integers(3, Umax + 1)), V, 0)
        labels[b, :lab.size] = lab
        labs.append(lab)
    cfg = types.SimpleNamespace(kernal_sizes=[], strides=[], pad_id=0)
    nll, want = CTCLoss(cfg, (B, T)).per_sample(labels, dev(torch, x), with_grad=True)
    logp, grad = ctc_score_grad(dev(torch, x), labs, [-1.0] * B)
    # that kernel's own test holds it to 1e-5 of fp64 and this one is far inside that: the bound is the sum of the two
    assert grad.data_ptr() != want.data_ptr() and float(want.abs().max()) > 0.1
    for b in range(B):                                       # and this kernel against its own reference on the same rows
        check_grad(grad[b].cpu().numpy(), x[b], [labs[b]], [-1.0], 0, b)
    diff = float((grad - want).abs().max())
    print(f"against w2v2_ctc_loss: largest gradient difference {diff:.3e}; nll difference {float(np.abs(-logp - nll.cpu().numpy()).max()):.3e}")
    assert diff <= 2e-5


# ---- 7. the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_abi_refusals(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    V = 8
    base = torch.zeros((20, V), device="cuda")
    lab = torch.ones(8, dtype=torch.int32, device="cuda")
    coef = torch.ones(2, dtype=torch.float64, device="cuda")
    logp = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((20, V), -7.5, device="cuda")
    good = dict(logits=base, V=V, n=2, row0=np.asarray([0, 10], np.int64), frames=np.asarray([10, 10], np.int32), m=2,
                utt=np.asarray([0, 1], np.int32), labels=lab, label0=np.asarray([0, 4], np.int64), nlab=np.asarray([4, 4], np.int32), blank=0,
                coef=coef, logp=logp, grad=grad, cap=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.w2v2_ctc_score_grad(N.ptr(a["logits"]), a["V"], a["n"], N.ptr(a["row0"]), N.ptr(a["frames"]), a["m"], N.ptr(a["utt"]),
                                       N.ptr(a["labels"]), N.ptr(a["label0"]), N.ptr(a["nlab"]), a["blank"], N.ptr(a["coef"]), N.ptr(a["logp"]),
                                       N.ptr(a["grad"]), a["cap"], N.current_stream())
    bad = [dict(logits=None), dict(coef=None), dict(logp=None), dict(grad=None), dict(labels=None), dict(n=0), dict(m=0), dict(V=1),
           dict(blank=V), dict(blank=-1), dict(frames=np.asarray([10, 0], np.int32)), dict(row0=np.asarray([0, -1], np.int64)),
           dict(utt=np.asarray([0, 2], np.int32)), dict(utt=np.asarray([-1, 1], np.int32)), dict(label0=np.asarray([0, -4], np.int64)),
           dict(nlab=np.asarray([4, -1], np.int32)), dict(nlab=np.asarray([4, 8192], np.int32)), dict(cap=-1), dict(cap=64)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert N.last_error()
    torch.cuda.synchronize()
    assert (logp == -7.0).all() and (grad == -7.5).all()                         # nothing launched, nothing written
    assert lib.w2v2_ctc_score_grad_workspace(0, N.ptr(good["frames"]), 2, N.ptr(good["utt"]), N.ptr(good["nlab"]), V) == -1
    long = np.asarray([4, 8192], np.int32)
    assert lib.w2v2_ctc_score_grad_workspace(2, N.ptr(good["frames"]), 2, N.ptr(good["utt"]), N.ptr(long), V) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(logp).all() and torch.isfinite(grad).all()
