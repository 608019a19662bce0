"""CTC prefix beam search on the GPU (w2v2_ctc_beam_search, wav2vec2.decoding) against the fp64 numpy reference
(tests/beam_reference.py): random and peaky logits with and without language models, exact ties, the greedy disagreement and the
meaning of `score`, isolation and determinism, bad input, the C ABI's argument checks, and Wav2Vec2ForCTC.transcribe.

The kernel and numpy do not share exp / log, so scores are not bit-equal and a decision whose margin is below the rounding noise
may go either way.  The reference returns each utterance's smallest decision margin; an utterance is FRAGILE when that margin is
below tau_i = 16 T_i 2^-52 max(1, max |key|).  Non-fragile utterances must match the reference in every label, in order; fragile
ones are checked for scores only, and at most 5 % of a test's utterances may be fragile."""

import math
import os

import numpy as np
import pytest

import beam_reference as BR
import helpers as H

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def make_logits(rng, T, V, blank, peaky):
    x = rng.standard_normal((T, V)).astype(np.float32)
    if peaky:                                                # a target per frame (runs of 3) raised by 2-8, half of them the blank
        tgt = np.repeat(rng.integers(0, V, T // 3 + 1), 3)[:T]
        tgt[rng.random(T) < 0.5] = blank
        x[np.arange(T), tgt] += rng.uniform(2, 8, T).astype(np.float32)
    return x


def random_lm(rng, V, order):
    return np.log(rng.dirichlet(np.ones(V), V ** (order - 1))).astype(np.float32)


def run(torch, xs, W, nbest, blank=0, lm=None):
    from wav2vec2.decoding import beam_search
    return beam_search([torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs], beam_width=W, nbest=nbest, blank=blank, lm=lm)


def reference(x, W, nbest, blank=0, lm=None):
    if lm is None:
        return BR.search(x, W, nbest, blank)
    return BR.search(x, W, nbest, blank, lm.table, lm.order, lm.alpha, lm.beta)


def compare(got, ref, T, stats):
    """one utterance against the reference; returns True when it was fragile.  stats: [smallest margin seen, largest score error]"""
    t = BR.tau(T, ref.kmax)
    fragile = ref.margin < t
    stats[0] = min(stats[0], ref.margin)
    if not fragile:
        assert [h.ids for h in got] == [k for k, _, _ in ref.hyps], (ref.margin, t)
    else:
        assert len(got) == len(ref.hyps)
    for h, (k, s, tot) in zip(got, ref.hyps):
        if h.ids == k:
            stats[1] = max(stats[1], abs(h.score - s), abs(h.total - tot))
            assert abs(h.score - s) <= t and abs(h.total - tot) <= t, (h, s, tot, t)
        else:                                                # (fragile only) another transcript within the noise: the keys agree
            assert abs(h.total - tot) <= 2 * t, (h, k, tot, t)
    return fragile


# ---- 4. random logits -------------------------------------------------------------------------------------------------------------
CASES = [  # (V, blank, order): order 0 = no language model
    (32, 0, 0), (32, 0, 1), (32, 0, 2), (32, 31, 3), (32, 0, 4), (5, 0, 0), (5, 4, 3), (64, 0, 0), (64, 63, 2), (64, 0, 4)]
# widths 1, 4, 16, 64 (the maximum), nbest 1 and 8; the large widths on the shorter utterances
SETS = [(1, 1, [1, 2, 50, 300]), (4, 1, [1, 7, 129, 400]), (4, 4, [3, 90]), (16, 8, [1, 2, 33, 200, 350]), (16, 1, [64, 257]),
        (64, 8, [1, 2, 3, 40, 150]), (64, 1, [9, 120])]


def case_inputs(V, blank, order):
    from wav2vec2.decoding import CharNgramLM
    rng = np.random.default_rng(1000 * V + 10 * order + blank)
    lm = CharNgramLM(random_lm(rng, V, order), order, alpha=0.8, beta=-0.2 if order % 2 else 0.3) if order else None
    sets = [(W, nbest, [make_logits(rng, T, V, blank, peaky) for T in Ts]) for W, nbest, Ts in SETS for peaky in (False, True)]
    return lm, sets


@pytest.mark.parametrize("V,blank,order", CASES)
def test_random_logits_match_reference(torch_mod, V, blank, order):
    """48 utterances per case, 480 in all, flat and peaky.  The reference alone on these seeds: the smallest decision margin per case
    is 2.4e-7 (V = 64, no LM) to 1.9e-4, the largest tau 2.2e-9, so every label is compared -- except one utterance (V = 32, no LM,
    width 64, 120 peaky frames) where two candidates at the pruning boundary have bit-equal fp64 keys (margin 0): it counts as
    fragile, 1 of 48.  The test prints these figures before it asserts."""
    lm, sets = case_inputs(V, blank, order)
    nfrag, ntot, stats = 0, 0, [math.inf, 0.0]
    for W, nbest, xs in sets:
        got = run(torch_mod, xs, W, nbest, blank, lm)
        for g, x in zip(got, xs):
            nfrag += compare(g, reference(x, W, nbest, blank, lm), x.shape[0], stats)
            ntot += 1
    print(f"V={V} blank={blank} order={order}: {ntot} utterances, {nfrag} fragile, min margin {stats[0]:.3g}, max score error {stats[1]:.3g}")
    assert nfrag <= 0.05 * ntot


# ---- 5. exact ties ----------------------------------------------------------------------------------------------------------------
def tie_inputs():
    rng = np.random.default_rng(17)
    xs = []
    for _ in range(6):
        x = rng.standard_normal((8, 4)).astype(np.float32)
        x[:, 2] = x[:, 1]                                    # two identical columns: swapping the two letters leaves a key bit-equal
        xs.append(x)
    xs.append(np.zeros((8, 4), np.float32))                  # every column equal
    xs.append(rng.integers(-1, 2, size=(8, 4)).astype(np.float32))
    return xs


def test_exact_ties(torch_mod):
    """Hypotheses that swap two letters with identical columns have bit-equal keys on any correct implementation (the same operations
    on the same numbers), so the order among them is the index rule's and the labels must EQUAL the reference's, whatever the
    library functions round to.  T = 8, V = 4 at widths that prune (2, 7, 64), and the first 3 frames at the maximum width, where
    nothing is pruned (at most 40 prefixes) and every score is also the brute-force value."""
    xs = tie_inputs()
    for W, nbest in [(64, 64), (64, 8), (7, 7), (2, 2)]:
        got = run(torch_mod, xs, W, nbest)
        for g, x in zip(got, xs):
            ref = BR.search(x, W, nbest)
            assert [h.ids for h in g] == [k for k, _, _ in ref.hyps]
            for h, (k, s, tot) in zip(g, ref.hyps):
                assert abs(h.score - s) <= 1e-12 and abs(h.total - tot) <= 1e-12
    xs3 = [x[:3] for x in xs]
    got = run(torch_mod, xs3, 64, 64)
    for g, x in zip(got, xs3):
        ref = BR.search(x, 64, 64)
        assert [h.ids for h in g] == [k for k, _, _ in ref.hyps]
        exact = {k: s for k, s, _ in BR.brute_force(x) if s > -math.inf}
        assert len(g) == len(exact)
        for h in g:
            assert abs(h.score - exact[h.ids]) <= 1e-12


def test_pruned_prefix_made_again(torch_mod):
    """A prefix p can be pruned while p + c stays, and be made again from p[:-1] later: p + c must then still be recognised as the
    extension of p by c (one candidate, not two).  Small vocabularies at width 3-8 do that often; the reference counts how often
    (`rejoined`), and the test wants inputs where it happens."""
    rng = np.random.default_rng(5)
    rejoined, stats = 0, [math.inf, 0.0]
    for V, W in [(3, 3), (3, 4), (3, 8), (4, 4), (4, 8), (6, 8)]:
        xs = [make_logits(rng, 60, V, 0, s % 2 == 1) for s in range(20)]
        for g, x in zip(run(torch_mod, xs, W, W), xs):
            ref = BR.search(x, W, W)
            rejoined += ref.rejoined
            compare(g, ref, 60, stats)
    print(f"rejoined {rejoined} times, min margin {stats[0]:.3g}")
    assert rejoined >= 20


# ---- 6. greedy disagreement and the meaning of score ------------------------------------------------------------------------------
def test_beats_greedy(torch_mod):
    x = np.log(np.array([[0.4, 0.35, 0.25]] * 2)).astype(np.float32)
    assert x.argmax(1).tolist() == [0, 0]
    for W in (2, 3, 4, 64):
        (g,) = run(torch_mod, [x], W, 1)
        assert g[0].ids == (1,) and abs(math.exp(g[0].score) - 0.4025) < 1e-6
    (g,) = run(torch_mod, [x], 1, 1)
    assert g[0].ids == () and abs(math.exp(g[0].score) - 0.16) < 1e-6


def exact_logp(torch, x, ids, blank):
    if len(ids) == 0:
        lp, _ = BR.log_probs(x)
        return float(lp[:, blank].sum())
    lp = torch.log_softmax(torch.from_numpy(x).double(), dim=1)[:, None, :]
    nll = torch.nn.functional.ctc_loss(lp, torch.tensor([list(ids)]), torch.tensor([x.shape[0]]), torch.tensor([len(ids)]),
                                       blank=blank, reduction="sum", zero_infinity=False)
    return -float(nll)


def test_score_is_a_lower_bound_of_the_exact_log_probability(torch_mod):
    """`score` sums only the frame paths whose prefixes stayed in the beam at every step: score <= -ctc_nll(ids) + tau for every
    returned hypothesis, with equality within tau when the width is large enough that nothing was pruned.  (The best beam score
    need NOT reach the greedy transcript's exact log-probability: on high-entropy logits it lies 0.03-3.8 nats below it at widths
    1-64, precisely because of this bound; that is not asserted.)"""
    rng = np.random.default_rng(23)
    for V, blank in [(32, 0), (6, 5)]:
        xs = [make_logits(rng, T, V, blank, peaky) for T in (5, 40, 120) for peaky in (False, True)]
        for W, nbest in [(1, 1), (4, 4), (16, 8), (64, 8)]:
            got = run(torch_mod, xs, W, nbest, blank)
            for g, x in zip(got, xs):
                t = BR.tau(x.shape[0], abs(g[-1].total))
                for h in g:
                    assert h.score == h.total
                    assert h.score <= exact_logp(torch_mod, x, h.ids, blank) + t, (W, h)
    xs = [make_logits(rng, 3, 4, 0, False) for _ in range(5)]              # nothing pruned: at most 40 prefixes
    for g, x in zip(run(torch_mod, xs, 64, 64), xs):
        for h in g:
            assert abs(h.score - exact_logp(torch_mod, x, h.ids, 0)) <= BR.tau(3, abs(h.score))


# ---- 7. isolation and determinism -------------------------------------------------------------------------------------------------
def raw(torch, base, row0, lens, W, nbest, blank=0, lm=None):
    """the C ABI itself: (labels, length, score, total) on the host"""
    from wav2vec2 import _native as N
    n, V, max_len = len(lens), int(base.shape[1]), max(lens)
    labels = torch.full((n, nbest, max_len), -7, dtype=torch.int32, device="cuda")
    length = torch.full((n, nbest), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.zeros((n, nbest), dtype=torch.float64, device="cuda")
    table = lm.device_table(base.device) if lm is not None else None
    lib = N.load()
    N.check(lib.w2v2_ctc_beam_search(N.ptr(base), V, n, N.ptr(np.asarray(row0, np.int64)), N.ptr(np.asarray(lens, np.int32)), blank, W,
                                     nbest, N.ptr(table), lm.order if lm else 1, lm.alpha if lm else 0.0, lm.beta if lm else 0.0,
                                     max_len, N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))
    return labels.cpu().numpy(), length.cpu().numpy(), score.cpu().numpy(), total.cpu().numpy()


def raw_list(torch, xs, W, nbest, blank=0, lm=None):
    lens = [x.shape[0] for x in xs]
    out = raw(torch, torch.from_numpy(np.concatenate(xs)).cuda(), np.cumsum([0] + lens[:-1]), lens, W, nbest, blank, lm)
    # per utterance, the label rows cut to the utterance's own frame count (the row stride is the call's longest utterance)
    assert all((out[0][i][:, lens[i]:] == -1).all() for i in range(len(xs)))
    return [(out[0][i][:, :lens[i]], out[1][i], out[2][i], out[3][i]) for i in range(len(xs))]


def same_bits(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2], equal_nan=True) and np.array_equal(a[3], b[3], equal_nan=True)


def test_isolation_forms_and_determinism(torch_mod):
    torch = torch_mod
    from wav2vec2.decoding import CharNgramLM, beam_search
    rng = np.random.default_rng(31)
    Ts = [50, 7, 333, 128, 129, 90]
    xs = [make_logits(rng, T, 32, 0, i % 2 == 1) for i, T in enumerate(Ts)]
    lm = CharNgramLM(random_lm(rng, 32, 3), 3, alpha=0.5, beta=0.1)
    for W, nbest, m in [(16, 8, None), (64, 4, lm)]:
        ref = raw_list(torch, xs, W, nbest, lm=m)
        for r in ref:
            assert (r[1] >= 0).all() and not (r[0] == -7).any()      # every output element written
        for g, r in zip(raw_list(torch, xs, W, nbest, lm=m), ref):                         # two calls
            same_bits(g, r)
        xs2 = list(xs)
        xs2[2] = make_logits(rng, Ts[2], 32, 0, True)                                      # another neighbour
        for i, (g, r) in enumerate(zip(raw_list(torch, xs2, W, nbest, lm=m), ref)):
            if i != 2:
                same_bits(g, r)
        perm = [3, 0, 5, 2, 1, 4]
        for g, i in zip(raw_list(torch, [xs[i] for i in perm], W, nbest, lm=m), perm):
            same_bits(g, ref[i])
        for i, x in enumerate(xs):                                                         # alone
            same_bits(raw_list(torch, [x], W, nbest, lm=m)[0], ref[i])
        # padded (B, Tmax, V) with junk behind each utterance, through the Python entry, against the list form
        Tm = max(Ts)
        pad = rng.standard_normal((len(Ts), Tm, 32)).astype(np.float32) * 50
        for b, x in enumerate(xs):
            pad[b, :x.shape[0]] = x
        a = beam_search(torch.from_numpy(pad).cuda(), beam_width=W, nbest=nbest, frame_lengths=Ts, lm=m)
        b = run(torch, xs, W, nbest, lm=m)
        assert a == b
        for hyps, r in zip(a, ref):
            assert [h.score for h in hyps] == r[2].tolist() and [len(h.ids) for h in hyps] == r[1].tolist()


# ---- 8. bad input -----------------------------------------------------------------------------------------------------------------
def test_bad_utterances_leave_neighbours_alone(torch_mod):
    rng = np.random.default_rng(41)
    xs = [make_logits(rng, T, 32, 0, False) for T in (40, 30, 30, 25, 40)]
    xs[1][7, 13] = np.nan
    xs[2][29, 0] = np.inf
    xs[3][:, 9] = -np.inf                                    # legal: label 9 can never be emitted
    xs[3][4, 3] = -np.inf
    got = raw_list(torch_mod, xs, 16, 4)
    clean = raw_list(torch_mod, [xs[0], xs[4]], 16, 4)
    same_bits(got[0], clean[0])
    same_bits(got[4], clean[1])
    for i in (1, 2):
        lab, length, sc, tot = got[i]
        assert (length == -1).all() and np.isnan(sc).all() and np.isnan(tot).all() and (lab == -1).all()
    hyps = run(torch_mod, xs, 16, 4)
    assert hyps[1] == [] and hyps[2] == []
    stats = [math.inf, 0.0]
    for i in (0, 3, 4):
        assert not compare(hyps[i], BR.search(xs[i], 16, 4), xs[i].shape[0], stats)
    assert all(9 not in h.ids for h in hyps[3])
    # a beam that holds fewer than W entries: one frame, one of 3 labels impossible: the empty prefix and two labels
    x = np.zeros((1, 4), np.float32)
    x[0, 2] = -np.inf
    lab, length, sc, tot = raw_list(torch_mod, [x], 16, 8)[0]
    assert length.tolist() == [0, 1, 1, -1, -1, -1, -1, -1] and np.isnan(sc[3:]).all() and np.isfinite(sc[:3]).all()
    assert lab[:, 0].tolist() == [-1, 1, 3, -1, -1, -1, -1, -1]


def test_python_raises_on_host_checkable_cases(torch_mod):
    from wav2vec2.decoding import CharNgramLM, beam_search
    x = torch_mod.zeros((2, 5, 8), device="cuda")
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(beam_width=4, nbest=5), dict(nbest=0), dict(blank=8), dict(blank=-1),
               dict(lm=CharNgramLM(np.zeros((1, 4), np.float32), 1)), dict(frame_lengths=[5, 6])):
        with pytest.raises(ValueError):
            beam_search(x, **kw)
    with pytest.raises(ValueError, match="vocabulary 65"):
        beam_search(torch_mod.zeros((1, 3, 65), device="cuda"))


def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    x = torch.zeros((4, 65), device="cuda")
    labels = torch.empty((1, 2, 4), dtype=torch.int32, device="cuda")
    length = torch.empty((1, 2), dtype=torch.int32, device="cuda")
    score = torch.empty((1, 2), dtype=torch.float64, device="cuda")
    total = torch.empty((1, 2), dtype=torch.float64, device="cuda")
    row0 = np.zeros(1, np.int64)

    def call(logits=N.ptr(x), V=8, n=1, frames=(4,), blank=0, W=4, nbest=2, order=1, alpha=0.0, max_len=4, r0=row0, lab=N.ptr(labels)):
        fr = np.asarray(frames, np.int32)
        return lib.w2v2_ctc_beam_search(logits, V, n, N.ptr(r0), N.ptr(fr), blank, W, nbest, None, order, alpha, 0.0, max_len, lab,
                                        N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream())

    assert call() == 0
    torch.cuda.synchronize()
    for kw, msg in [(dict(logits=None), "null"), (dict(lab=None), "null"), (dict(n=0), "utterances"), (dict(frames=(0,)), "frames"),
                    (dict(blank=8), "blank"), (dict(blank=-1), "blank"), (dict(W=0), "beam width"), (dict(W=65), "beam width"),
                    (dict(W=1, nbest=2), "nbest"), (dict(nbest=0), "nbest"), (dict(V=65), "vocabulary"), (dict(V=0), "vocabulary"),
                    (dict(max_len=3), "max_len"), (dict(order=0), "order"), (dict(order=5), "order"),
                    (dict(alpha=float("nan")), "finite"), (dict(r0=np.full(1, -1, np.int64)), "negative")]:
        assert call(**kw) != 0, kw
        assert msg in N.last_error(), (kw, N.last_error())
    torch.cuda.synchronize()


# ---- 9. model level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_model_transcribe(torch_mod, name):
    import wav2vec2
    from wav2vec2.decoding import CharNgramLM
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 52345, 24000)]
    hosts = [l.cpu().numpy() for l in m.predict_packed(waves)]
    lm = CharNgramLM.from_text(["the quick brown fox", "jumps over the lazy dog"], tok, order=3, add_k=0.5, alpha=0.6, beta=0.2)
    nfrag = 0
    for kw in (dict(beam_width=16, nbest=4), dict(beam_width=64, nbest=1, lm=lm), dict()):
        out = m.transcribe(waves, tok, **kw)
        W, nbest, l = kw.get("beam_width", 16), kw.get("nbest", 1), kw.get("lm")
        for tr, h in zip(out, hosts):
            ref = reference(h, W, nbest, cfg.pad_id, l)
            fragile = ref.margin < BR.tau(h.shape[0], ref.kmax)
            nfrag += fragile
            assert tr.words is None and tr.texts == [x.text(tok) for x in tr.hypotheses]
            assert tr.text == (tr.texts[0] if tr.texts else "")
            if not fragile:
                assert tr.texts == [tok.decode(k, group_tokens=False) for k, _, _ in ref.hyps]
                assert [x.ids for x in tr.hypotheses] == [k for k, _, _ in ref.hyps]
    print(f"{name}: {nfrag} of 12 fragile")
    assert nfrag <= 0.05 * 12
    # the greedy path
    for tr, h in zip(m.transcribe(waves, tok, beam_width=None), hosts):
        assert tr.text == tok.decode(h.argmax(1)) and len(tr.hypotheses) == 1
    # timestamps: the words of the transcript, in order, inside the utterance
    spf = float(np.prod(cfg.strides)) / 16000.0
    delim = tok.get_vocab()["|"]
    id_text = {i: t for t, i in tok.get_vocab().items()}
    for tr, h in zip(m.transcribe(waves, tok, beam_width=16, timestamps=True), hosts):
        best = tr.hypotheses[0]
        words, cur = [], []
        for i in best.ids + (delim,):
            if i == delim:
                if cur:
                    words.append("".join(id_text[c] for c in cur))
                cur = []
            else:
                cur.append(i)
        assert [w.text for w in tr.words] == words
        if not best.ids:
            assert tr.text == "" and tr.words == []
        last = 0.0
        for w in tr.words:
            assert last <= w.start_s < w.end_s <= h.shape[0] * spf + 1e-9
            last = w.end_s


def test_views_are_read_in_place(torch_mod):
    torch = torch_mod
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import beam_search
    base = torch.randn(30, 8, device="cuda")
    parts = list(torch.split(base, [10, 5, 15]))
    got, row0, lens = _logits_base(parts, None)
    assert got.data_ptr() == base.data_ptr() and row0 == [0, 10, 15] and lens == [10, 5, 15]
    a = beam_search(parts, beam_width=8, nbest=2)
    b = beam_search([p.clone() for p in parts], beam_width=8, nbest=2)
    assert a == b
