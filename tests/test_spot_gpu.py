"""CTC phrase search on the GPU (w2v2_ctc_spot, wav2vec2.spotting) against the fp64 numpy reference
(tests/spot_reference.py).  No tolerance: the trace z is compared bitwise (as int64), c, the hits and the counts with ==.  The edges
of the recursion and of the prefetch ring, every lane layout, ties, the hit pass, the edge rule, bad inputs, a mixed call through
the C ABI with isolation, determinism and the argument checks, a long recording, exact=True, chunking, and the model's entry
points."""

import itertools
import os

import numpy as np
import pytest

import helpers as H
import score_reference as ScR
import spot_reference as SR

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")
NEG = -np.inf


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def raw_spot(torch, base, V, row0, frames, utt, labs, blank, delim, thr, max_hits, traced=None, lead=5):
    """w2v2_ctc_spot through the C ABI.  `traced`: the pairs that get a trace (None: all).  Returns host arrays: score, begin, end
    (m, max_hits), count (m), and per pair (z, c) or None."""
    from wav2vec2 import _native as N
    m = len(labs)
    flat = np.concatenate([np.full(lead, 10 ** 6, np.int32)] + [np.asarray(l, np.int32) for l in labs] + [np.zeros(1, np.int32)])
    label0 = (lead + np.cumsum([0] + [len(l) for l in labs[:-1]])).astype(np.int64)
    nlab = np.asarray([len(l) for l in labs], np.int32)
    lab_dev = torch.from_numpy(flat).cuda()
    score = torch.full((m, max_hits), -7.0, dtype=torch.float64, device="cuda")
    begin = torch.full((m, max_hits), -7, dtype=torch.int32, device="cuda")
    end = torch.full((m, max_hits), -7, dtype=torch.int32, device="cuda")
    count = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    traced = list(range(m)) if traced is None else list(traced)
    trace0 = np.full(m, -1, np.int64)
    at = 3
    for j in traced:
        trace0[j] = at
        at += frames[utt[j]] + 2                             # (gaps between the traces: nothing may be written there)
    tz = torch.full((at,), -7.0, dtype=torch.float64, device="cuda")
    tc = torch.full((at,), -7, dtype=torch.int32, device="cuda")
    thr = np.broadcast_to(np.asarray(thr, np.float64), (m,)).copy()
    row0_h, frames_h, utt_h = np.asarray(row0, np.int64), np.asarray(frames, np.int32), np.asarray(utt, np.int32)     # (alive over the call)
    N.check(N.load().w2v2_ctc_spot(N.ptr(base), V, len(frames), N.ptr(row0_h), N.ptr(frames_h), m,
                                   N.ptr(utt_h), N.ptr(lab_dev), N.ptr(label0), N.ptr(nlab), blank, delim, N.ptr(thr),
                                   max_hits, N.ptr(score), N.ptr(begin), N.ptr(end), N.ptr(count), N.ptr(tz), N.ptr(tc), N.ptr(trace0),
                                   N.current_stream()), "w2v2_ctc_spot")
    tz_h, tc_h = tz.cpu().numpy(), tc.cpu().numpy()
    traces = [None] * m
    used = np.zeros(at, bool)
    for j in traced:
        T = frames[utt[j]]
        traces[j] = (tz_h[trace0[j]:trace0[j] + T], tc_h[trace0[j]:trace0[j] + T])
        used[trace0[j]:trace0[j] + T] = True
    assert (tz_h[~used] == -7.0).all() and (tc_h[~used] == -7).all()
    return score.cpu().numpy(), begin.cpu().numpy(), end.cpu().numpy(), count.cpu().numpy(), traces


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def check_pair(out, j, x, lab, blank, delim, thr, max_hits, what=""):
    """pair j of a raw_spot result against the reference on recording x; returns the reference's count"""
    score, begin, end, count, traces = out
    n, s, b, e, z, c = SR.spot(x, lab, blank, delim, thr, max_hits)
    if traces[j] is not None:
        if n >= 0:
            assert same_bits(traces[j][0], z), (what, "z", np.flatnonzero(traces[j][0] != z)[:5])
        else:
            assert np.isnan(traces[j][0]).all(), (what, "z of a bad pair")
        assert np.array_equal(traces[j][1], c), (what, "c", np.flatnonzero(traces[j][1] != c)[:5])
    assert count[j] == n, (what, "count", count[j], n)
    k = max(0, min(n, max_hits))
    assert same_bits(score[j, :k], s[:k]) and np.isnan(score[j, k:]).all(), (what, "score", score[j], s)
    assert np.array_equal(begin[j], b) and np.array_equal(end[j], e), (what, "spans", begin[j], b, end[j], e)
    return n


def run_and_check(torch, xs, pairs, blank, delim=-1, thr=NEG, max_hits=8, V=None):
    """recordings xs back to back in one buffer, pairs [(recording, labels)]: one call, every pair against the reference"""
    V = V or xs[0].shape[1]
    base = dev(torch, np.concatenate(xs))
    row0 = list(np.cumsum([0] + [len(x) for x in xs[:-1]]))
    frames = [len(x) for x in xs]
    out = raw_spot(torch, base, V, row0, frames, [i for i, _ in pairs], [l for _, l in pairs], blank, delim, thr, max_hits)
    thr = np.broadcast_to(np.asarray(thr, np.float64), (len(pairs),))
    return out, [check_pair(out, j, xs[i], lab, blank, delim, thr[j], max_hits, (j, i, len(lab))) for j, (i, lab) in enumerate(pairs)]


def distinct_labels(rng, U, V, blank):
    """U labels, no two neighbours equal"""
    pool = [v for v in range(V) if v != blank]
    lab = [int(rng.choice(pool))]
    while len(lab) < U:
        v = int(rng.choice(pool))
        if v != lab[-1]:
            lab.append(v)
    return lab


# ---- 1. edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank_last", [False, True])
def test_edges(torch_mod, blank_last):
    rng = np.random.default_rng(11)
    V = 5
    blank = V - 1 if blank_last else 0
    rel = (lambda l: [v - 1 for v in l]) if blank_last else (lambda l: l)          # labels 1 .. 4 -> 0 .. 3 when the blank is last
    xs = [(rng.standard_normal((T, V)) * 2).astype(np.float32) for T in range(1, 41)]
    pairs = [(T - 1, rel([1, 2, 3])) for T in range(1, 41)]                         # every T in 1 .. 40 for U = 3: the ring's start and tail
    pairs += [(i, rel(l)) for i in (0, 1, 2, 8, 16, 17, 39) for l in ([2], [1, 2], [3, 3], [1, 1, 2, 2], [1, 2, 1, 2, 1], [4, 3, 2, 1, 2, 3, 4])]
    for thr in (NEG, -3.0):
        _, counts = run_and_check(torch_mod, xs, pairs, blank, thr=thr)
        assert counts[0] in (0, 1) and counts[1] == 0 and max(counts) >= 2          # T = 1; T = 2 < U: no hit
    # V = 2: the blank and one label
    x2 = [(rng.standard_normal((T, 2)) * 2).astype(np.float32) for T in (1, 7, 30)]
    b2 = 1 if blank_last else 0
    run_and_check(torch_mod, x2, [(i, [1 - b2] * U) for i in range(3) for U in (1, 2, 3)], b2, thr=-2.0)


# ---- 2. every lane layout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256])
def test_lane_layouts(torch_mod, U):
    rng = np.random.default_rng(U)
    T, V, blank = 3 * U + 5, 8, 0
    lab = distinct_labels(rng, U, V, blank)
    starts = [1, U + 3]
    path = {t: blank for t in range(T)}
    for s in starts:
        for k, v in enumerate(lab):
            path[s + k] = v
    x = SR.planted(rng, T, V, blank, path)
    short = lab[:max(1, U - 70)]                             # a second pair of the same recording, in a smaller layout where one exists
    out, counts = run_and_check(torch_mod, [x], [(0, lab), (0, short), (0, lab)], blank, thr=[-1.0, NEG, -1.0], max_hits=4)
    score, begin, end = out[0], out[1], out[2]
    assert counts[0] == 2 and list(begin[0, :2]) == starts and list(end[0, :2]) == [s + U - 1 for s in starts]
    assert (score[0, :2] == 0.0).all()                       # each occurrence IS the greedy path: exactly 0
    z = out[4][0][0]
    assert np.isfinite(z[U - 1:]).all()                      # the deepest state carries finite scores from the first frame that can
    assert same_bits(out[4][0][0], out[4][2][0]) and np.array_equal(out[4][0][1], out[4][2][1])


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------------
def test_ties(torch_mod):
    rng = np.random.default_rng(3)
    xs = [rng.integers(-2, 3, (200, V)).astype(np.float32) for V in (4, 4, 4)]
    pairs = [(0, [1, 2, 3, 1, 2]), (1, [1, 1, 2, 3, 3]), (2, [3, 2, 3, 2, 3]), (0, [2]), (1, [3, 1])]
    out, counts = run_and_check(torch_mod, xs, pairs, 0, thr=NEG, max_hits=64)
    z, c = out[4][0]
    fin = np.isfinite(z)
    assert len(np.unique(z[fin])) < fin.sum() // 4           # integers: the scores collide all the time
    # delim set on integer logits: the edge candidates tie with the regular ones
    run_and_check(torch_mod, xs, [(0, [1, 2, 3, 1]), (1, [1, 3, 2, 1]), (2, [1, 2, 1])], 0, delim=1, thr=NEG, max_hits=64)


# ---- 4. the hit pass on the device ----------------------------------------------------------------------------------------------------
def test_hit_pass(torch_mod):
    rng = np.random.default_rng(4)
    T, V, blank, lab = 120, 6, 0, [1, 2, 3]
    path = {t: blank for t in range(T)}
    starts = [4, 30, 31 + 20, 80, 110]
    for s in starts:
        for k, v in enumerate([1, 1, 2, 3, 3]):
            path[s + k] = v
    x = SR.planted(rng, T, V, blank, path)
    noisy = (rng.standard_normal((T, V))).astype(np.float32)
    pairs = [(0, lab), (1, lab), (1, [2]), (0, [3, 3])]
    for max_hits in (2, 64):
        for thr in (NEG, -4.0, -1.0, 0.0, np.inf):
            out, counts = run_and_check(torch_mod, [x, noisy], pairs, blank, thr=thr, max_hits=max_hits)
            if thr == -1.0:
                assert counts[0] == 5                        # the true count, whatever max_hits
                assert list(out[1][0, :2]) == starts[:2] and list(out[2][0, :2]) == [s + 3 for s in starts[:2]]
                if max_hits == 2:
                    assert out[0].shape == (4, 2) and not np.isnan(out[0][0]).any()
            if thr == NEG:
                assert counts[1] >= 3                        # candidates on every frame: overlapping ones compete
            if thr == np.inf:
                assert counts == [0, 0, 0, 0]


# ---- 5. the edge rule -----------------------------------------------------------------------------------------------------------------
def test_edge_rule(torch_mod):
    blank, delim, A, B = 0, 1, 2, 3
    path = [A, B, delim, 0, 0, 0, delim, A, B, delim, 0, 0, 0, delim, A, B]
    x = SR.planted(np.random.default_rng(3), len(path), 5, blank, dict(enumerate(path)))
    just = SR.planted(np.random.default_rng(4), 4, 5, blank, {0: A, 1: A, 2: B, 3: B})
    lab = [delim, A, B, delim]
    pairs = [(0, lab), (1, lab), (0, [delim, A, delim]), (0, [A, B]), (1, [delim, delim])]
    on, n_on = run_and_check(torch_mod, [x, just], pairs, blank, delim=delim, thr=-1.0)
    off, n_off = run_and_check(torch_mod, [x, just], pairs, blank, delim=-1, thr=-1.0)
    assert n_on[:2] == [3, 1] and n_off[:2] == [1, 0]
    assert list(on[1][0, :3]) == [0, 6, 13] and list(on[2][0, :3]) == [2, 9, 15]           # frame 0, the interior, frame T - 1
    assert (on[1][1, 0], on[2][1, 0]) == (0, 3)                                             # the recording that is just the word
    assert (off[0][0, 0], off[1][0, 0], off[2][0, 0]) == (on[0][0, 1], on[1][0, 1], on[2][0, 1]) == (0.0, 6, 9)     # interior: the same
    assert n_on[3] == n_off[3] == 3 and np.array_equal(on[1][3], off[1][3])                 # a phrase without the delimiter: the same


# ---- 6. bad inputs --------------------------------------------------------------------------------------------------------------------
def test_bad_inputs(torch_mod):
    rng = np.random.default_rng(6)
    V = 8
    xs = [(rng.standard_normal((T, V)) * 2).astype(np.float32) for T in (40, 30, 30, 25, 40, 33)]
    xs[1][7, 5] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][11, :] = -np.inf                                   # a frame of -inf only
    xs[4][:, 6] = -np.inf                                    # legal: label 6 can never be emitted
    xs[4][rng.random((40, V)) < 0.1] = -np.inf               # a sprinkling of -inf
    xs[4][:, 0] = np.maximum(xs[4][:, 0], -5.0)              # ... that leaves every frame a finite entry
    utt = [0, 1, 1, 2, 3, 4, 4, 4, 5, 0, 5, 0]
    labs = [[1, 2, 3], [1, 2], [4], [3], [1, 2, 3], [1, 6, 2], [3, 3], [1, 2], [7, 7, 1], [8], [0, 1], [2, -1, 3]]
    out, counts = run_and_check(torch_mod, xs, list(zip(utt, labs)), 0, thr=-6.0, max_hits=4)
    assert counts == [counts[0], -1, -1, -1, -1, counts[5], counts[6], counts[7], counts[8], -1, -1, -1]
    assert min(counts[0], counts[6], counts[7], counts[8]) >= 1 and counts[5] == 0
    # the neighbours of the bad pairs are what they are alone
    alone, _ = run_and_check(torch_mod, [xs[0], xs[4], xs[5]], [(0, labs[0]), (1, labs[6]), (2, labs[8])], 0, thr=-6.0, max_hits=4)
    for j, k in ((0, 0), (6, 1), (8, 2)):
        assert same_bits(out[4][j][0], alone[4][k][0]) and np.array_equal(out[1][j], alone[1][k]) and same_bits(out[0][j], alone[0][k])


# ---- 7. a mixed call through the C ABI --------------------------------------------------------------------------------------------------
def mixed_case():
    rng = np.random.default_rng(7)
    V, blank, delim = 16, 3, 5
    big = (rng.standard_normal((700, V)) * 2).astype(np.float32)
    big[rng.random(700) < 0.5, blank] += 3.0
    # 5 recordings at row offsets of one buffer; 1 and 2 overlap, 3 lies inside 0
    row0, frames = [10, 300, 350, 60, 560], [200, 150, 120, 41, 140]
    pool = [v for v in range(V) if v != blank]
    labs = []
    for U in (1, 2, 3, 5, 8, 13, 20, 40, 64, 65, 100, 130):
        lab = rng.choice(pool, U)
        for k in range(1, U):
            if rng.random() < 0.2:
                lab[k] = lab[k - 1]
        labs.append([int(v) for v in lab])
    labs[2][0] = labs[4][-1] = delim
    pairs = [(i, p) for i in range(5) for p in range(12) if (i + p) % 2 == 0 or p < 4]
    order = rng.permutation(len(pairs))
    pairs = [pairs[k] for k in order]
    thr = [(-2.0 * len(labs[p]), NEG, -4.0)[(i + p) % 3] for i, p in pairs]
    traced = [j for j in range(len(pairs)) if j % 3 != 1]
    return big, V, blank, delim, row0, frames, labs, pairs, thr, traced


def test_mixed_call_isolation_determinism(torch_mod):
    torch = torch_mod
    big, V, blank, delim, row0, frames, labs, pairs, thr, traced = mixed_case()
    base = dev(torch, big)
    utt, pl = [i for i, _ in pairs], [labs[p] for _, p in pairs]
    out = raw_spot(torch, base, V, row0, frames, utt, pl, blank, delim, thr, 6, traced)
    total = 0
    for j, (i, p) in enumerate(pairs):
        assert (out[4][j] is not None) == (j in traced)
        total += check_pair(out, j, big[row0[i]:row0[i] + frames[i]], labs[p], blank, delim, thr[j], 6, (j, i, p))
    assert total > 50
    again = raw_spot(torch, base, V, row0, frames, utt, pl, blank, delim, thr, 6, traced)                   # twice: the same bits
    for a, b in zip(out[:4], again[:4]):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    for j in traced:
        assert same_bits(out[4][j][0], again[4][j][0]) and np.array_equal(out[4][j][1], again[4][j][1])
    for j in range(0, len(pairs), 3):                                                                        # alone: the same bits
        i, p = pairs[j]
        one = raw_spot(torch, base, V, [row0[i]], [frames[i]], [0], [labs[p]], blank, delim, [thr[j]], 6)
        assert same_bits(one[0][0], out[0][j]) and np.array_equal(one[1][0], out[1][j]) and np.array_equal(one[2][0], out[2][j])
        assert one[3][0] == out[3][j]
        if j in traced:
            assert same_bits(one[4][0][0], out[4][j][0]) and np.array_equal(one[4][0][1], out[4][j][1])


def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    x = torch.zeros((4, 8), device="cuda")
    lab = torch.ones(600, dtype=torch.int32, device="cuda")
    hs = torch.full((2, 3), -7.0, dtype=torch.float64, device="cuda")
    hb = torch.full((2, 3), -7, dtype=torch.int32, device="cuda")
    he = torch.full((2, 3), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    tz = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    tc = torch.full((8,), -7, dtype=torch.int32, device="cuda")

    def call(logits=N.ptr(x), V=8, n=1, r0=(0,), frames=(4,), m=2, utt=(0, 0), labp=N.ptr(lab), l0=(0, 3), nl=(2, 1), blank=0, delim=-1,
             thr=(-1.0, -1.0), max_hits=3, hsp=N.ptr(hs), hbp=N.ptr(hb), hep=N.ptr(he), cntp=N.ptr(cnt), tzp=N.ptr(tz), tcp=N.ptr(tc),
             t0=(0, 4), uttp=True, framesp=True, thrp=True, t0p=True):
        r0, fr, ut = np.asarray(r0, np.int64), np.asarray(frames, np.int32), np.asarray(utt, np.int32)
        l0, nl, th, t0 = np.asarray(l0, np.int64), np.asarray(nl, np.int32), np.asarray(thr, np.float64), np.asarray(t0, np.int64)
        return lib.w2v2_ctc_spot(logits, V, n, N.ptr(r0), N.ptr(fr) if framesp else None, m, N.ptr(ut) if uttp else None, labp, N.ptr(l0),
                                 N.ptr(nl), blank, delim, N.ptr(th) if thrp else None, max_hits, hsp, hbp, hep, cntp, tzp, tcp,
                                 N.ptr(t0) if t0p else None, N.current_stream())

    def untouched():
        torch.cuda.synchronize()
        return all((t.cpu().numpy() == -7).all() for t in (hs, hb, he, cnt, tz, tc))

    for kw, msg in [(dict(logits=None), "null"), (dict(labp=None), "null"), (dict(hsp=None), "null"), (dict(hbp=None), "null"),
                    (dict(hep=None), "null"), (dict(cntp=None), "null"), (dict(uttp=False), "null"), (dict(framesp=False), "null"),
                    (dict(thrp=False), "null"), (dict(t0p=False), "null"), (dict(tzp=None), "trace"), (dict(tcp=None), "trace"),
                    (dict(m=0), "pairs"), (dict(n=0), "recordings"), (dict(max_hits=0), "max_hits"), (dict(V=1), "vocabulary"),
                    (dict(frames=(0,)), "frames"), (dict(frames=(-4,)), "frames"), (dict(r0=(-1,)), "negative"), (dict(l0=(0, -1)), "negative"),
                    (dict(t0=(0, -2)), "negative"), (dict(utt=(0, 1)), "recording"), (dict(utt=(-1, 0)), "recording"), (dict(nl=(0, 1)), "labels"),
                    (dict(nl=(257, 1)), "labels"), (dict(nl=(-1, 1)), "labels"), (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
                    (dict(delim=0), "delimiter"), (dict(delim=8), "delimiter"), (dict(delim=-2), "delimiter"),
                    (dict(thr=(-1.0, float("nan"))), "NaN")]:
        assert call(**kw) != 0, kw
        assert msg in N.last_error(), (kw, N.last_error())
    assert untouched()                                       # refused without a launch: nothing was written
    assert call(tzp=None, tcp=None, t0p=False) == 0          # no trace at all is legal
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() >= 0).all() and (tz.cpu().numpy() == -7.0).all()
    assert call(nl=(256, 1), delim=7, thr=(NEG, np.inf)) == 0                      # the limits themselves are accepted
    torch.cuda.synchronize()
    assert list(cnt.cpu().numpy()) == [0, 0] and np.isnan(hs.cpu().numpy()).all() and (hb.cpu().numpy() == -1).all()


# ---- 8. long --------------------------------------------------------------------------------------------------------------------------
def test_long_recording(torch_mod):
    rng = np.random.default_rng(8)
    T, V, blank, lab = 20000, 8, 0, [1, 2, 3, 4, 5]
    path = {t: blank for t in range(T)}
    for s in range(50, 1000, 90):                            # occurrences at the start, then thousands of frames without one
        for k, v in enumerate(lab):
            path[s + k] = v
    x = SR.planted(rng, T, V, blank, path, scale=3.0)
    out, counts = run_and_check(torch_mod, [x], [(0, lab), (0, lab)], blank, thr=[-4.0, NEG], max_hits=32)
    z, c = out[4][0]
    assert counts[0] >= 11 and np.isfinite(z[4:]).all()
    stale = np.diff(np.flatnonzero(np.diff(c[1000:]) != 0))
    assert stale.max() > 5                                   # paths that stay alive in the last state for frames on end
    assert z.min() < -10.0


# ---- 9. exact=True --------------------------------------------------------------------------------------------------------------------
def test_exact_logp(torch_mod):
    from wav2vec2.spotting import find_phrases
    rng = np.random.default_rng(9)
    V, blank = 8, 0
    phrases = [[1, 2, 3], [4, 4, 5], [6]]
    xs = []
    for T in (90, 140):
        path = {t: blank for t in range(T)}
        for s, p in zip(range(7, T - 12, 23), itertools.cycle(phrases)):
            k = s
            for a, v in enumerate(p):
                if a and p[a - 1] == v:
                    k += 1                                   # a blank frame between repeated labels
                path[k] = path[k + 1] = v
                k += 2
        xs.append(SR.planted(rng, T, V, blank, path, scale=4.0))
    parts = [dev(torch_mod, x) for x in xs]
    hits = find_phrases(parts, phrases, blank=blank, exact=True)
    plain = find_phrases(parts, phrases, blank=blank)
    n = 0
    for j, (hs, ps) in enumerate(zip(hits, plain)):
        x = xs[j // 3]
        assert [h[:4] for h in hs] == [h[:4] for h in ps] and all(p.logp is None for p in ps)
        for h in hs:
            frames = h.end - h.begin + 1
            ref = ScR.ctc_logp(x[h.begin:h.end + 1], phrases[h.phrase], blank)
            assert abs(h.logp * frames - ref) <= ScR.tau(frames, ref), (j, h, ref)
            n += 1
    assert n >= 8


# ---- 10. chunking ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_cases():
    from test_spot_cpu import CHUNK_PHRASE, chunk_input
    cases = [chunk_input(seed) for seed in range(10)]
    return CHUNK_PHRASE, [(x, starts, SR.chunked(x, CHUNK_PHRASE, 0, -1.0, 256, 64)) for x, starts in cases]


def test_chunking(torch_mod, chunk_cases):
    from wav2vec2.spotting import find_phrases
    phrase, cases = chunk_cases
    parts = [dev(torch_mod, x) for x, _, _ in cases]
    got = find_phrases(parts, [phrase], min_score=-1.0, chunk_frames=256, overlap_frames=64)
    whole = find_phrases(parts, [phrase], min_score=-1.0)
    for hs, ws, (x, starts, ref) in zip(got, whole, cases):
        assert [(h.score, h.begin, h.end) for h in hs] == ref                      # the reference's chunk rule, exactly
        assert hs == ws and len(hs) == 16 and [h.begin for h in hs] == starts       # ... and on this input the unchunked result


# ---- 11. the model's entry points -----------------------------------------------------------------------------------------------------
def test_model_search(torch_mod):
    import wav2vec2
    from wav2vec2.processor import Wav2Vec2Processor
    from wav2vec2.spotting import find_phrases, phrase_labels, phrase_spans
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    delim = tok.get_vocab()["|"]
    cfg = H.case_config("tiny_base")
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights("tiny_base"))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 24000)]
    phrases = ["a", "the cat", (5, 6)]
    labs = [phrase_labels("a", tok), phrase_labels("the cat", tok), [5, 6]]
    spf = 320 / 16000.0
    kw = dict(margin_per_label=3.0, max_hits=16)
    got = m.search(waves, phrases, tok, **kw)
    logits = m.predict_packed(waves)
    hits = find_phrases(logits, labs, blank=cfg.pad_id, delimiter_id=delim, **kw)
    assert len(got) == 3 and sum(len(g) for g in got) > 0
    for i, g in enumerate(got):
        assert g == phrase_spans(hits[3 * i:3 * i + 3], ["a", "the cat", (5, 6)], spf)
        assert all(a.start_s <= b.start_s for a, b in zip(g, g[1:]))
        for s in g:
            assert 0.0 <= s.start_s < s.end_s <= logits[i].shape[0] * spf + 1e-9 and s.score <= 0.0 and s.logp is None
    j, h = next((j, hs[0]) for j, hs in enumerate(hits) if hs)
    assert phrase_spans([[h]], {h.phrase: "x"}, spf) == [wav2vec2.spotting.PhraseSpan("x", h.begin * spf, (h.end + 1) * spf, h.score, None)]
    host = logits[j // 3].cpu().numpy()
    n, s, b, e, _, _ = SR.spot(host, labs[j % 3], cfg.pad_id, delim, -3.0 * len(labs[j % 3]), 16)
    assert n == len(hits[j]) and [(x.score, x.begin, x.end) for x in hits[j]] == [(s[i], b[i], e[i]) for i in range(n)]
    ex = m.search(waves, phrases, tok, exact=True, **kw)
    assert [[s[:4] for s in g] for g in ex] == [[s[:4] for s in g] for g in got] and all(s.logp <= 0.0 for g in ex for s in g)
    # sampling_rate= passes through
    w8 = [w[::2].copy() for w in waves]
    got8 = m.search(w8, phrases, tok, sampling_rate=8000, **kw)
    hits8 = find_phrases(m.predict_packed(w8, sampling_rate=8000), labs, blank=cfg.pad_id, delimiter_id=delim, **kw)
    assert [g for g in got8] == [phrase_spans(hits8[3 * i:3 * i + 3], phrases, spf) for i in range(3)]
    with pytest.raises(ValueError, match="tokenizer"):
        m.search(waves, phrases, **kw)
    # search_long on a recording of three windows
    rec = rng.standard_normal(14000).astype(np.float32)
    wkw = dict(window_s=6400 / 16000.0, margin_s=640 / 16000.0)
    long_logits = m.predict_long(rec, **wkw)
    assert long_logits.shape[0] == m.num_frames(14000)
    got = m.search_long(rec, phrases, tok, **wkw, **kw)
    ref = find_phrases([long_logits], labs, blank=cfg.pad_id, delimiter_id=delim, **kw)
    assert got == phrase_spans(ref, phrases, spf) and len(got) > 0
    both = m.search_long([rec, rec[:9000]], phrases, tok, **wkw, **kw)
    assert isinstance(both, list) and len(both) == 2 and both[0] == got
