"""Exact CTC scoring on the GPU (w2v2_ctc_score, wav2vec2.decoding.ctc_score / rescore) against the fp64 numpy
reference (tests/score_reference.py): the edges of the recursion, every thread layout, a mixed call through the C ABI with shared
rows and offsets, isolation and determinism, the range of fp64 log space, the beam search's lower bounds, the C ABI's argument
checks, and the model's entry points (transcribe with rescore / confidence, score).

Tolerance: tau = 16 T 2^-52 max(1, |reference|) (score_reference.tau); -inf and NaN results are compared exactly."""

import math
import os

import numpy as np
import pytest

import helpers as H
import score_reference as SR

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def check(got, ref, T, what=""):
    """one result against the reference: exact for -inf / NaN, tau otherwise; returns |error| / tau"""
    if math.isnan(ref):
        assert math.isnan(got), (what, got, ref)
        return 0.0
    if ref == -math.inf:
        assert got == -math.inf, (what, got, ref)
        return 0.0
    t = SR.tau(T, ref)
    assert abs(got - ref) <= t, (what, got, ref, abs(got - ref) / t)
    return abs(got - ref) / t


def random_labels(rng, U, V, blank, repeat_p=0.3):
    pool = [v for v in range(V) if v != blank]
    lab = rng.choice(pool, U) if U else np.zeros(0, np.int64)
    for k in range(1, U):
        if rng.random() < repeat_p:
            lab[k] = lab[k - 1]
    return lab.astype(np.int64)


# ---- 1. the edges of the recursion ------------------------------------------------------------------------------------------------
def test_edges(torch_mod):
    from wav2vec2.decoding import ctc_score
    rng = np.random.default_rng(11)
    cases = [(1, []), (9, []), (1, [3]), (2, [3]), (7, [1, 1, 2, 2, 3]), (6, [1, 1, 2, 2, 3]), (5, [1, 2, 3, 4, 1]), (4, [1, 2, 3, 4, 1]),
             (3, [2, 2]), (2, [2, 2]), (1, [1, 2])]
    xs = [(rng.standard_normal((T, 5)) * 2).astype(np.float32) for T, _ in cases]
    for blank in (0, 4):
        labs = [[(l % 4) + 1 if blank == 0 else l % 4 for l in lab] for _, lab in cases]
        got = ctc_score([dev(torch_mod, x) for x in xs], labs, blank=blank)
        assert got.dtype == np.float64 and got.shape == (len(cases),)
        for g, x, lab, (T, _) in zip(got, xs, labs, cases):
            check(float(g), SR.ctc_logp(x, lab, blank), T, (T, lab, blank))
    T7, T6 = cases[4][0], cases[5][0]
    assert T7 == 7 and T6 == 6 and math.isfinite(got[4]) and got[5] == -math.inf      # T = U + R exactly, and one frame less


# ---- 2. every thread layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [255, 256, 257, 511, 512, 1023, 1024, 2049])
def test_thread_layouts(torch_mod, U):
    from wav2vec2.decoding import ctc_score
    rng = np.random.default_rng(U)
    T, V = 2 * U + 3, 8
    x = (rng.standard_normal((T, V)) * 2).astype(np.float32)
    lab = random_labels(rng, U, V, 0)
    short = lab[:U - 70]                                     # a second pair of the same utterance in a smaller layout where one exists
    got = ctc_score([dev(torch_mod, x)], [lab, short, lab], utterance=[0, 0, 0])
    e = check(float(got[0]), SR.ctc_logp(x, lab, 0), T, U)
    check(float(got[1]), SR.ctc_logp(x, short, 0), T, (U, "short"))
    assert got[0] == got[2]
    print(f"U = {U}: |error| / tau = {e:.4f}")


# ---- 3. a mixed call through the C ABI: shared rows, scrambled pairs, non-zero offsets ----------------------------------------------
def raw_score(torch, base, V, row0, frames, utt, labs, blank, lead=5):
    from wav2vec2 import _native as N
    flat = np.concatenate([np.full(lead, 10 ** 6, np.int32)] + [np.asarray(l, np.int32) for l in labs] + [np.zeros(1, np.int32)])
    label0 = (lead + np.cumsum([0] + [len(l) for l in labs[:-1]])).astype(np.int64)
    nlab = np.asarray([len(l) for l in labs], np.int32)
    lab_dev = torch.from_numpy(flat).cuda()
    out = torch.full((len(labs),), -7.0, dtype=torch.float64, device="cuda")
    N.check(N.load().w2v2_ctc_score(N.ptr(base), V, len(frames), N.ptr(np.asarray(row0, np.int64)), N.ptr(np.asarray(frames, np.int32)),
                                    len(labs), N.ptr(np.asarray(utt, np.int32)), N.ptr(lab_dev), N.ptr(label0), N.ptr(nlab), blank,
                                    N.ptr(out), N.current_stream()), "w2v2_ctc_score")
    return out.cpu().numpy()


@pytest.mark.parametrize("V,scale,seed", [(5, 1.0, 0), (32, 4.0, 1), (64, 12.0, 2)])
def test_mixed_call(torch_mod, V, scale, seed):
    rng = np.random.default_rng(100 + seed)
    Ts = [[1, 2, 37, 400], [3, 64, 129, 311], [5, 65, 200, 399]][seed]
    blank = [0, V - 1, 7][seed]
    xs = [(rng.standard_normal((T, V)) * scale).astype(np.float32) for T in Ts]
    # the utterances in one buffer with junk rows before, between and behind them, in an order of their own
    place = [2, 0, 3, 1]
    chunks, row0, at = [rng.standard_normal((3, V)).astype(np.float32) * 99], [0] * 4, 3
    for i in place:
        row0[i] = at
        chunks += [xs[i], np.full((2, V), np.nan, np.float32)]
        at += Ts[i] + 2
    base = dev(torch_mod, np.concatenate(chunks))
    pairs = []
    for i, T in enumerate(Ts):
        for _ in range(17):
            U = int(rng.integers(0, T + 2)) if rng.random() < 0.3 else int(rng.integers(0, T // 2 + 2))
            pairs.append((i, random_labels(rng, U, V, blank)))
    order = rng.permutation(len(pairs))
    pairs = [pairs[k] for k in order]
    got = raw_score(torch_mod, base, V, row0, Ts, [i for i, _ in pairs], [l for _, l in pairs], blank)
    worst, ninf = 0.0, 0
    for g, (i, lab) in zip(got, pairs):
        ref = SR.ctc_logp(xs[i], lab, blank)
        ninf += ref == -math.inf
        worst = max(worst, check(float(g), ref, Ts[i], (i, lab.size)))
    print(f"V = {V}: {len(pairs)} pairs, {ninf} infeasible, largest |error| / tau = {worst:.4f}")
    assert 0 < ninf < len(pairs) // 2


# ---- 4. isolation and determinism ---------------------------------------------------------------------------------------------------
def test_isolation_forms_and_determinism(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import ctc_score
    rng = np.random.default_rng(21)
    Ts, V = [50, 7, 333, 128, 700, 90], 32
    xs = [(rng.standard_normal((T, V)) * 3).astype(np.float32) for T in Ts]
    utt = [0, 0, 1, 2, 2, 2, 3, 4, 4, 5, 0]
    labs = [random_labels(rng, int(rng.integers(0, Ts[i] // 2 + 1)), V, 0) for i in utt]
    labs[7] = random_labels(rng, 300, V, 0, 0.05)            # a pair of another thread layout in the same call
    parts = [dev(torch, x) for x in xs]
    ref = ctc_score(parts, labs, utterance=utt)
    assert np.isfinite(ref).all()
    np.testing.assert_array_equal(ctc_score(parts, labs, utterance=utt), ref)                        # twice
    perm = rng.permutation(len(utt))
    np.testing.assert_array_equal(ctc_score(parts, [labs[k] for k in perm], utterance=[utt[k] for k in perm]), ref[perm])
    np.testing.assert_array_equal(ctc_score(parts, labs + labs, utterance=utt + utt), np.concatenate((ref, ref)))    # repetition
    for k, (i, lab) in enumerate(zip(utt, labs)):                                                   # alone
        assert ctc_score([parts[i]], [lab])[0] == ref[k]
    # padded (B, Tmax, V) with junk behind each utterance
    pad = rng.standard_normal((len(Ts), max(Ts), V)).astype(np.float32) * 50
    for b, x in enumerate(xs):
        pad[b, :x.shape[0]] = x
    np.testing.assert_array_equal(ctc_score(dev(torch, pad), labs, frame_lengths=Ts, utterance=utt), ref)
    # views that are not row-contiguous take the one-concatenation path of _logits_base
    strided = [dev(torch, np.ascontiguousarray(x.T)).t() for x in xs]
    assert not strided[0].is_contiguous()
    np.testing.assert_array_equal(ctc_score(strided, labs, utterance=utt), ref)
    wide = [dev(torch, np.concatenate((x, x), axis=1))[:, :V] for x in xs]
    np.testing.assert_array_equal(ctc_score(wide, labs, utterance=utt), ref)
    # the default pairing: one label sequence per utterance
    one = ctc_score(parts, [labs[utt.index(i)] for i in range(len(Ts))])
    np.testing.assert_array_equal(one, [ref[utt.index(i)] for i in range(len(Ts))])


# ---- 5. range and non-finite logits ---------------------------------------------------------------------------------------------------
def test_range_and_nonfinite(torch_mod):
    from wav2vec2.decoding import ctc_score
    z = np.zeros((40, 5), np.float32)
    z[:, 0] = 2000.0                                         # every label emission is e^-2000: a probability form flushes it
    got = ctc_score([dev(torch_mod, z)], [[1, 2]])[0]
    ref = SR.ctc_logp(z, [1, 2], 0)
    assert abs(ref - (-3993.34)) < 0.01
    check(float(got), ref, 40)
    rng = np.random.default_rng(51)
    xs = [(rng.standard_normal((T, 8)) * 2).astype(np.float32) for T in (40, 30, 30, 25, 40)]
    xs[1][7, 5] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][:, 6] = -np.inf                                    # legal: label 6 can never be emitted
    xs[3][4, 3] = -np.inf
    utt = [0, 1, 1, 2, 3, 3, 3, 4, 2]
    labs = [[1, 2, 3], [1, 2], [], [3], [1, 2, 3], [1, 6, 2], [3, 3], [7, 7, 1], []]
    got = ctc_score([dev(torch_mod, x) for x in xs], labs, utterance=utt)
    for g, i, lab in zip(got, utt, labs):
        check(float(g), SR.ctc_logp(xs[i], lab, 0), xs[i].shape[0], (i, lab))
    assert np.isnan(got[[1, 2, 3, 8]]).all()                 # every pair of the NaN and the +inf utterance, their neighbours not
    assert np.isfinite(got[[0, 4, 6, 7]]).all() and got[5] == -math.inf
    clean = ctc_score([dev(torch_mod, xs[0]), dev(torch_mod, xs[4])], [labs[0], labs[7]])
    assert clean[0] == got[0] and clean[1] == got[7]


def test_python_raises_on_host_checkable_cases(torch_mod):
    from wav2vec2.decoding import ctc_score
    x = torch_mod.zeros((2, 5, 8), device="cuda")
    for labs, kw in [([[8], [1]], {}), ([[-1], [1]], {}), ([[0], [1]], {}), ([[3], [1]], dict(blank=3)), ([[1]], {}), ([[1], [1]], dict(blank=8)),
                     ([[1], [1], [1]], dict(utterance=[0, 1])), ([[1]], dict(utterance=[2])), ([[1]], dict(utterance=[-1])),
                     ([[1] * 8192, [1]], {}), ([], dict(utterance=[]))]:
        with pytest.raises(ValueError):
            ctc_score(x, labs, **kw)
    got = ctc_score(x, [[1, 2, 1, 2, 1, 2], [1, 1, 1]])      # too few frames is a result
    assert got[0] == -math.inf and math.isfinite(got[1])
    big = torch_mod.zeros((1, 8200, 4), device="cuda")
    lab = (np.arange(8191) % 3 + 1).tolist()                 # the most labels a pair may have: the one layout of 1024 threads
    check(float(ctc_score(big, [lab])[0]), SR.ctc_logp(np.zeros((8200, 4), np.float32), lab, 0), 8200)


# ---- 6. against the beam search ---------------------------------------------------------------------------------------------------
def test_rescore_against_the_beam(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import CharNgramLM, beam_search, rescore
    rng = np.random.default_rng(61)
    V = 16
    xs = []
    for T in (30, 77, 150, 12):
        x = rng.standard_normal((T, V)).astype(np.float32)
        tgt = np.repeat(rng.integers(0, V, T // 3 + 1), 3)[:T]
        tgt[rng.random(T) < 0.5] = 0
        x[np.arange(T), tgt] += rng.uniform(1, 5, T).astype(np.float32)
        xs.append(x)
    parts = [dev(torch, x) for x in xs]
    lm = CharNgramLM(np.log(rng.dirichlet(np.ones(V), V)).astype(np.float32), 2, alpha=0.7, beta=0.3)
    gaps = {}
    for W in (1, 4, 16, 64):
        for m in (None, lm):
            nbest = min(W, 8)
            hyps = beam_search(parts, beam_width=W, nbest=nbest, lm=m)
            out = rescore(parts, hyps)
            for i, (old, new) in enumerate(zip(hyps, out)):
                T = xs[i].shape[0]
                assert sorted(h.ids for h in old) == sorted(h.ids for h in new)
                by_ids = {h.ids: h for h in old}
                for h in new:
                    o = by_ids[h.ids]
                    check(h.score, SR.ctc_logp(xs[i], h.ids, 0), T, (W, i, h.ids))
                    assert h.score >= o.score - SR.tau(T, h.score)                       # the beam's score is a lower bound
                    assert abs((h.total - h.score) - (o.total - o.score)) <= 1e-9        # the LM part is kept
                    gaps[W] = max(gaps.get(W, 0.0), h.score - o.score)
                assert all(a.total >= b.total for a, b in zip(new, new[1:]))             # sorted by total
    print("largest exact - beam score by width:", {w: round(g, 4) for w, g in gaps.items()})
    # V = 5 and at most 4 frames: at most 57 prefixes are alive before the last frame (5, 17, 57 after 1, 2, 3 frames), so width 64 prunes nothing
    # that a surviving hypothesis' paths pass through, and the beam's scores ARE exact
    for T in (3, 4):
        x = (rng.standard_normal((T, 5)) * 2).astype(np.float32)
        hyps = beam_search([dev(torch, x)], beam_width=64, nbest=64)
        new = rescore([dev(torch, x)], hyps)[0]
        old = {h.ids: h for h in hyps[0]}
        assert len(new) >= 50
        for h in new:
            check(h.score, SR.ctc_logp(x, h.ids, 0), T, h.ids)
            assert abs(h.score - old[h.ids].score) <= SR.tau(T, h.score)
    # the greedy path's hypothesis (no beam score) gets score = total = exact
    from wav2vec2.decoding import Hypothesis
    g = rescore(parts[:1], [[Hypothesis((1, 2), float("nan"), float("nan"))]])[0][0]
    assert g.score == g.total
    check(g.score, SR.ctc_logp(xs[0], (1, 2), 0), 30)


def test_beam_is_exact_at_v5_t5_width64(torch_mod):
    """The beam's scores equal the exact ones within tau at V = 5, T = 5, width 64, where nothing is pruned.

    "Nothing is pruned" is a property of the logits, not of the shape: a beam entry with probability 0 (key -inf) is dropped, so
    the prefixes that count are those with a path of non-zero probability.  On logits whose four labels can all be emitted there
    are 5, 17, 57, 189 such prefixes after 1 .. 4 frames, width 64 prunes, and the beam's score is a strict lower bound
    (fp64 reference beam against the fp64 exact score on six seeded inputs: up to 0.115 below; on the MI355X 4.3e-3 on one).
    So the logits here make one label impossible (a -inf column, which is legal): with three labels a prefix of U labels and R
    repeated neighbours is alive after t frames iff U + R <= t, which gives 4, 10, 25, 61 prefixes after 1 .. 4 frames -- never
    more than 64.  Only the cut of the final list to 64 drops anything, and that drops whole hypotheses, not paths of those that
    stay.  The fp64 reference beam agrees with the fp64 exact score to 0.034 tau on eight such seeded inputs."""
    from wav2vec2.decoding import beam_search, rescore
    worst = 0.0
    for seed in range(4):
        rng = np.random.default_rng(62 + seed)
        x = (rng.standard_normal((5, 5)) * 2).astype(np.float32)
        x[:, 1 + seed] = -np.inf                            # label 1 + seed can never be emitted
        hyps = beam_search([dev(torch_mod, x)], beam_width=64, nbest=64)
        new = rescore([dev(torch_mod, x)], hyps)[0]
        old = {h.ids: h for h in hyps[0]}
        assert len(new) == 64 and all(1 + seed not in h.ids for h in new)
        for h in new:
            check(h.score, SR.ctc_logp(x, h.ids, 0), 5, h.ids)
            t = SR.tau(5, h.score)
            worst = max(worst, abs(h.score - old[h.ids].score) / t)
            assert abs(h.score - old[h.ids].score) <= t, (seed, h.ids, h.score, old[h.ids].score)
    print(f"V = 5, T = 5, width 64, one impossible label: largest |exact - beam| / tau = {worst:.4f}")


# ---- 7. the C ABI's argument checks -------------------------------------------------------------------------------------------------
def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    x = torch.zeros((4, 8), device="cuda")
    lab = torch.ones(8200, dtype=torch.int32, device="cuda")
    out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    before = None

    def call(logits=N.ptr(x), V=8, n=1, r0=(0,), frames=(4,), m=2, utt=(0, 0), labp=N.ptr(lab), l0=(0, 3), nl=(2, 1), blank=0, outp=N.ptr(out),
             uttp=True, framesp=True):
        r0, fr, ut = np.asarray(r0, np.int64), np.asarray(frames, np.int32), np.asarray(utt, np.int32)
        l0, nl = np.asarray(l0, np.int64), np.asarray(nl, np.int32)
        return lib.w2v2_ctc_score(logits, V, n, N.ptr(r0), N.ptr(fr) if framesp else None, m, N.ptr(ut) if uttp else None, labp, N.ptr(l0),
                                  N.ptr(nl), blank, outp, N.current_stream())

    assert call() == 0
    torch.cuda.synchronize()
    good = out.cpu().numpy().copy()
    assert np.isfinite(good).all()
    out.fill_(-7.0)
    for kw, msg in [(dict(logits=None), "null"), (dict(labp=None), "null"), (dict(outp=None), "null"), (dict(uttp=False), "null"),
                    (dict(framesp=False), "null"), (dict(m=0), "pairs"), (dict(n=0), "utterances"), (dict(utt=(0, 1)), "utterance"),
                    (dict(utt=(-1, 0)), "utterance"), (dict(nl=(8192, 1)), "labels"), (dict(nl=(-1, 1)), "labels"), (dict(blank=8), "blank"),
                    (dict(blank=-1), "blank"), (dict(frames=(-4,)), "frames"), (dict(frames=(0,)), "frames"), (dict(V=1), "vocabulary"),
                    (dict(r0=(-1,)), "negative"), (dict(l0=(0, -1)), "negative")]:
        assert call(**kw) != 0, kw
        assert msg in N.last_error(), (kw, N.last_error())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()                 # refused without a launch: nothing was written
    assert call(nl=(8191, 1), frames=(4,)) == 0              # the limit itself is accepted (infeasible on 4 frames: -inf)
    torch.cuda.synchronize()
    assert out.cpu().numpy()[0] == -math.inf


# ---- 8. model level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_model_rescore_confidence_score(torch_mod, name):
    import wav2vec2
    from wav2vec2.decoding import ScoredTranscript, Transcript, ctc_score
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 52345, 24000)]
    logits = m.predict_packed(waves)
    hosts = [l.cpu().numpy() for l in logits]
    # both arguments off: today's Transcripts
    plain = m.transcribe(waves, tok, beam_width=16, nbest=4)
    off = m.transcribe(waves, tok, beam_width=16, nbest=4, rescore=False, confidence=False)
    assert off == plain and all(type(t) is Transcript for t in off)
    # rescore=True: the same hypotheses with exact scores, ordered by them
    for tr, p, h in zip(m.transcribe(waves, tok, beam_width=16, nbest=4, rescore=True, timestamps=True), plain, hosts):
        assert type(tr) is Transcript and sorted(x.ids for x in tr.hypotheses) == sorted(x.ids for x in p.hypotheses)
        for x in tr.hypotheses:
            check(x.score, SR.ctc_logp(h, x.ids, cfg.pad_id), h.shape[0], x.ids)
            assert x.total == x.score
        assert all(a.total >= b.total for a, b in zip(tr.hypotheses, tr.hypotheses[1:]))
        assert tr.text == tr.texts[0] == tr.hypotheses[0].text(tok) and tr.words is not None
    # confidence=True
    for kw in (dict(), dict(posterior_scale=0.3)):
        for tr, h in zip(m.transcribe(waves, tok, beam_width=16, nbest=4, confidence=True, **kw), hosts):
            assert type(tr) is ScoredTranscript and len(tr.posteriors) == len(tr.hypotheses) == len(tr.texts) >= 2
            assert abs(sum(tr.posteriors) - 1.0) < 1e-12 and tr.confidence == tr.posteriors[0]
            assert all(a >= b for a, b in zip(tr.posteriors, tr.posteriors[1:]))
            assert len(tr.word_confidence) == len(tr.words)
            for c in tr.word_confidence:
                assert tr.posteriors[0] - 1e-12 <= c <= 1.0 + 1e-12
            assert [w.text for w in tr.words] == tr.text.split()
            for x in tr.hypotheses:
                check(x.score, SR.ctc_logp(h, x.ids, cfg.pad_id), h.shape[0], x.ids)
    for bad in (dict(beam_width=16, nbest=1), dict(beam_width=None)):
        with pytest.raises(ValueError, match="nbest"):
            m.transcribe(waves, tok, confidence=True, **bad)
    # score: the sibling of align
    texts = ["A", "HI", "THE CAT SAT", "DOG"]
    ids = [list(tok(t)) for t in texts]
    got = m.score(waves, texts, tok)
    direct = ctc_score(logits, ids, blank=cfg.pad_id)
    for (lp, per), d, h, lab in zip(got, direct, hosts, ids):
        assert lp == d and per == d / h.shape[0]
        check(lp, SR.ctc_logp(h, lab, cfg.pad_id), h.shape[0], lab)
    assert m.score(waves, ids) == got
    with pytest.raises(ValueError):
        m.score(waves, texts)                                # text without a tokenizer
    with pytest.raises(ValueError):
        m.score(waves, ids[:3])


def test_long_recording_confidence_and_segment_scores(torch_mod):
    """decode_long with rescore / confidence on synthetic logits with pauses, and score_segments over forced-aligned pieces"""
    torch = torch_mod
    from wav2vec2.alignment import forced_align_long, score_segments, split_at_pauses, token_spans, word_spans
    from wav2vec2.decoding import ScoredTranscript, ctc_score
    from wav2vec2.longform import LongTranscript, ScoredLongTranscript, decode_long
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    vocab = tok.get_vocab()
    V, delim, blank = max(vocab.values()) + 1, vocab["|"], vocab["<pad>"]
    rng = np.random.default_rng(71)
    text = "THE CAT SAT ON THE MAT AND THE DOG RAN OFF"
    path = []
    for k, word in enumerate(text.split()):
        for c in tok(word):
            path += [int(c)] * 3 + [blank]
        path += [delim] * 2 + [blank] * (40 if k % 3 == 2 else 2)
    T = len(path)
    x = rng.standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), path] += 8.0
    logits = dev(torch, x)
    cut = dict(min_pause=10, min_frames=20, max_frames=120)
    plain = decode_long(logits, tok, beam_width=8, nbest=4, blank=blank, **cut)
    assert type(plain) is LongTranscript and len(plain.segments) >= 3
    assert decode_long(logits, tok, beam_width=8, nbest=4, blank=blank, rescore=False, confidence=False, **cut) == plain
    res = decode_long(logits, tok, beam_width=8, nbest=4, blank=blank, rescore=True, **cut)
    assert type(res) is LongTranscript and len(res.segments) == len(plain.segments)
    for sg in res.segments:
        f0, f1 = int(round(sg.start_s / 0.02)), int(round(sg.end_s / 0.02))
        for h in sg.transcript.hypotheses:
            check(h.score, SR.ctc_logp(x[f0:f1], h.ids, blank), f1 - f0, h.ids)
    sc = decode_long(logits, tok, beam_width=8, nbest=4, blank=blank, confidence=True, **cut)
    assert type(sc) is ScoredLongTranscript and sc.text == res.text and len(sc.word_confidence) == len(sc.words) > 0
    logc, nw, confs = 0.0, 0, []
    for sg in sc.segments:
        tr = sg.transcript
        assert type(tr) is ScoredTranscript and abs(sum(tr.posteriors) - 1.0) < 1e-12 and tr.confidence == tr.posteriors[0]
        confs += tr.word_confidence
        logc += len(tr.words) * math.log(tr.confidence)
        nw += len(tr.words)
    assert confs == sc.word_confidence and abs(sc.confidence - math.exp(logc / nw)) < 1e-12
    assert [w.text for w in sc.words] == sc.text.split()
    with pytest.raises(ValueError, match="nbest"):
        decode_long(logits, tok, beam_width=8, nbest=1, blank=blank, confidence=True, **cut)
    # the likelihood filter: the pieces of the aligned recording, one of them with a wrong text
    ids = list(tok(text))
    a = forced_align_long(logits, ids, blank=blank)
    id_text = {i: (" " if t == "|" else t) for t, i in vocab.items()}
    words = word_spans(token_spans(a), delim, 0.02, id_text)
    segs = split_at_pauses(words, min_pause_s=0.5, max_len_s=20.0)
    assert len(segs) >= 3
    good = score_segments(logits, segs, tok, 0.02, blank)
    for sg, g in zip(segs, good):
        f0, f1 = int(round(sg.start_s / 0.02)), int(round(sg.end_s / 0.02))
        ref = SR.ctc_logp(x[f0:f1], list(tok(sg.text)), blank)
        assert abs(g * (f1 - f0) - ref) <= SR.tau(f1 - f0, ref)
    wrong = list(segs)
    wrong[1] = wrong[1]._replace(text="A DOG BIT ME")
    bad = score_segments(logits, wrong, tok, 0.02, blank)
    assert bad[0] == good[0] and bad[2] == good[2] and bad[1] < good[1] - 1.0
    assert score_segments(logits, [], tok, 0.02, blank) == []
