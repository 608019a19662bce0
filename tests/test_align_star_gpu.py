"""The star (wildcard) label of the CTC forced alignment on the GPU (w2v2_ctc_align_star, w2v2_ctc_align_long_star,
wav2vec2.alignment.forced_align(..., star_score=...)) against the fp64 numpy reference
(tests/align_star_reference.py, lse_t and its sum in the kernels' order of operations): token, label_index, frame_logp and score
bit for bit at every pairs-per-thread count and with stars at the places where a thread's pairs begin, end and cross the LDS
exchange; degenerate shapes; mixed batches against the star-free call; ties, -inf and NaN logits; bad utterances; determinism;
argument errors; forced_align_long against forced_align over tile geometries, and 9000 labels against the reference;
Wav2Vec2ForCTC.align / align_long with star and free_ends."""

import os

import numpy as np
import pytest

import align_reference as AR
import align_star_reference as SR
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def rand_labels(rng, U, V, blank, rep=0.1):
    others = np.array([v for v in range(V) if v != blank])
    out = []
    for _ in range(U):
        out.append(out[-1] if out and rng.random() < rep else int(rng.choice(others)))
    return out


def put_stars(labels, ks, V):
    """the star at every k of ks that has no star beside it"""
    U = len(labels)
    for k in ks:
        if 0 <= k < U and (k == 0 or labels[k - 1] != V) and (k == U - 1 or labels[k + 1] != V):
            labels[k] = V
    return labels


def pairs_per_thread(pairs):
    return 1 if pairs <= 256 else 2 if pairs <= 512 else 4 if pairs <= 1024 else 8


def host(al):
    return al.token.cpu().numpy(), al.label_index.cpu().numpy(), al.frame_logp.cpu().numpy(), al.score


def dev(torch, xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def align(torch, xs, labels, blank=0, star_score=-0.5):
    from wav2vec2.alignment import forced_align
    return [host(a) for a in forced_align(dev(torch, xs), labels, blank=blank, star_score=star_score)]


def same_bits(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    fa, fb = np.asarray(a[2], np.float32), np.asarray(b[2], np.float32)
    both_nan = np.isnan(fa) & np.isnan(fb)
    np.testing.assert_array_equal(fa.view(np.int32)[~both_nan], fb.view(np.int32)[~both_nan])
    sa, sb = np.float64(a[3]), np.float64(b[3])
    assert (np.isnan(sa) and np.isnan(sb)) or sa.tobytes() == sb.tobytes(), (a[3], b[3])


def assert_reference_bits(got, x, labels, blank, star_score, what=""):
    """the four outputs against the reference, bit for bit (the figures are printed before they are asserted)"""
    want = SR.viterbi(x, labels, blank, star_score, device_order=True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    fa, fb = got[2], want[2]
    differ = (fa.view(np.int32) != fb.view(np.int32)) & ~(np.isnan(fa) & np.isnan(fb))
    print(f"{what} T={x.shape[0]} U={len(labels)}: frame_logp differs on {int(differ.sum())} of {fa.size} frames, "
          f"score {got[3]!r} vs {want[3]!r}")
    same_bits(got, want)


def assert_reference_decisions(got, x, labels, blank, star_score):
    want = SR.viterbi(x, labels, blank, star_score, device_order=True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def raw_align(torch, xs, labels, blank, star_score, long=None):
    """the C ABI itself, labels on the device unchecked: (rc, [(token, label_index, frame_logp, score) per utterance])"""
    from wav2vec2 import _native as N
    lens = [x.shape[0] for x in xs]
    V = xs[0].shape[1]
    base = torch.from_numpy(np.concatenate(xs)).cuda()
    lab = torch.from_numpy(np.concatenate([np.asarray(l, np.int32) for l in labels] + [np.zeros(1, np.int32)])).cuda()
    row0 = np.cumsum([0] + lens[:-1]).astype(np.int64)
    label0 = np.cumsum([0] + [len(l) for l in labels[:-1]]).astype(np.int64)
    frames = np.asarray(lens, np.int32)
    nlab = np.asarray([len(l) for l in labels], np.int32)
    tot, n = sum(lens), len(xs)
    tok = torch.full((tot,), -7, dtype=torch.int32, device="cuda")
    li = torch.full_like(tok, -7)
    fl = torch.zeros(tot, dtype=torch.float32, device="cuda")
    sc = torch.zeros(n, dtype=torch.float64, device="cuda")
    lib = N.load()
    args = (N.ptr(base), V, n, N.ptr(row0), N.ptr(frames), N.ptr(lab), N.ptr(label0), N.ptr(nlab), blank, star_score, N.ptr(tok),
            N.ptr(li), N.ptr(fl), N.ptr(sc))
    if long is None:
        rc = lib.w2v2_ctc_align_star(*args, N.current_stream())
    else:
        rc = lib.w2v2_ctc_align_long_star(*args, long[0], long[1], 0, N.current_stream())
    torch.cuda.synchronize()
    out, o = [], 0
    tok, li, fl, sc = tok.cpu().numpy(), li.cpu().numpy(), fl.cpu().numpy(), sc.cpu().numpy()
    for i, T in enumerate(lens):
        out.append((tok[o:o + T], li[o:o + T], fl[o:o + T], float(sc[i])))
        o += T
    return rc, out


# ---- 1. random logits at every pairs-per-thread count ------------------------------------------------------------------------
def star_case(rng, U, V, blank, P, d):
    """U labels with stars at label 0, at U - 1, at the first and the last pair of a thread in the middle, and between two equal
    labels; T = U + R + d"""
    labels = rand_labels(rng, U, V, blank, rep=0.15)
    tid = max(1, (U // P) // 2)
    ks = [0, U - 1, P * tid, P * tid + P - 1, P * (tid + 1) + P - 1]
    if U >= 12:
        e = min(U - 3, P * tid + 3 * P + 2)
        labels[e - 1] = labels[e + 1] = next(v for v in range(V) if v != blank)      # equal neighbours around a star
        ks.append(e)
    put_stars(labels, ks, V)
    T = U + AR.repeats(labels) + d
    return rng.standard_normal((T, V)).astype(np.float32) * 3, labels


@pytest.mark.parametrize("V,blank", [(32, 0), (400, 7)])
@pytest.mark.parametrize("Us", [[1, 5, 255], [256, 300], [511, 512], [1023, 1024], [1100]])
def test_random_logits_match_reference(torch_mod, V, blank, Us):
    rng = np.random.default_rng(V + sum(Us))
    P = pairs_per_thread(max(Us) + 1)
    cases = []
    for i, U in enumerate(Us):
        x, labels = star_case(rng, U, V, blank, P, d=9 + 3 * i)
        if i == 0:                                                   # T - 1 a multiple of 8 in the call's first utterance only
            extra = (1 - x.shape[0]) % 8
            x = np.concatenate([x, rng.standard_normal((extra, V)).astype(np.float32) * 3])
            assert (x.shape[0] - 1) % 8 == 0
        elif (x.shape[0] - 1) % 8 == 0:
            x = x[:-1] if x.shape[0] - 1 >= len(labels) + AR.repeats(labels) + 1 else np.concatenate([x, x[-1:]])
        cases.append((x, labels))
    assert all(V in l for _, l in cases)
    got = align(torch_mod, [c[0] for c in cases], [c[1] for c in cases], blank)
    for g, (x, labels) in zip(got, cases):
        assert (g[0] == V).any()
        assert_reference_bits(g, x, labels, blank, -0.5, f"V={V} P={P}")


# ---- 2. degenerate cases -----------------------------------------------------------------------------------------------------
def test_degenerate_shapes(torch_mod):
    rng = np.random.default_rng(4)
    V = 32
    labels = [[V], [V], [3, V, 3, 3, V], [V, 5, 5, V, 9], []]
    Ts = [1, 6, 5 + 1, 5 + 1, 4]                                    # the star alone in one frame; T = U + R exactly (twice)
    xs = [rng.standard_normal((T, V)).astype(np.float32) * 2 for T in Ts]
    got = align(torch_mod, xs, labels)
    for g, x, l in zip(got, xs, labels):
        assert_reference_bits(g, x, l, 0, -0.5, "degenerate")
    assert got[0][0].tolist() == [V] and got[0][1].tolist() == [0]
    assert got[2][0].tolist() == [3, V, 3, 0, 3, V]


def test_infeasible_with_a_star(torch_mod):
    rng = np.random.default_rng(14)
    V = 32
    xs = [rng.standard_normal((T, V)).astype(np.float32) for T in (20, 4, 20)]
    labels = [[4, V, 6], [V, 3, 3, V], [V]]                        # the second: 4 labels and one repeat in 4 frames
    rc, got = raw_align(torch_mod, xs, labels, 0, -0.5)
    assert rc == 0
    tok, li, fl, sc = got[1]
    assert sc == -np.inf and (tok == -1).all() and (li == -1).all() and np.isnan(fl).all()
    want = SR.viterbi(xs[1], labels[1], 0, -0.5)
    assert want[3] == -np.inf
    for i in (0, 2):
        assert_reference_bits(got[i], xs[i], labels[i], 0, -0.5, "beside an infeasible utterance")
    from wav2vec2.alignment import forced_align
    with pytest.raises(ValueError, match="utterance 1: 4 frames cannot hold 4 labels with 1 repeats"):
        forced_align(dev(torch_mod, xs), labels, star_score=-0.5)


# ---- 3. mixed batches --------------------------------------------------------------------------------------------------------
def test_mixed_batch_star_free_utterances_keep_their_bits(torch_mod):
    from wav2vec2.alignment import forced_align
    rng = np.random.default_rng(31)
    V = 32
    Us = [40, 300, 7, 120, 0, 513]                                  # (P = 4 for the call)
    labels = [rand_labels(rng, U, V, 0) for U in Us]
    for i in (1, 3):
        put_stars(labels[i], [0, len(labels[i]) // 2, len(labels[i]) - 1], V)
    xs = [rng.standard_normal((len(l) + AR.repeats(l) + 11, V)).astype(np.float32) * 2 for l in labels]
    xd = dev(torch_mod, xs)
    free = [i for i in range(len(Us)) if V not in labels[i]]
    before = [host(a) for a in forced_align([xd[i] for i in free], [labels[i] for i in free])]
    got = [host(a) for a in forced_align(xd, labels, star_score=-0.5)]
    for j, i in enumerate(free):
        same_bits(got[i], before[j])
    for i in (1, 3):
        assert_reference_bits(got[i], xs[i], labels[i], 0, -0.5, "mixed")
    after = [host(a) for a in forced_align([xd[i] for i in free], [labels[i] for i in free])]
    for a, b in zip(after, before):
        same_bits(a, b)
    # the whole star-free batch through the star call: the star-free call's bits
    both = [host(a) for a in forced_align([xd[i] for i in free], [labels[i] for i in free], star_score=-0.5)]
    for a, b in zip(both, before):
        same_bits(a, b)


# ---- 4. ties and non-finite logits ---------------------------------------------------------------------------------------------
def test_ties_and_non_finite_logits(torch_mod):
    rng = np.random.default_rng(17)
    V = 6
    xs, labels = [], []
    for U, T in [(2, 9), (5, 20), (30, 90), (200, 500), (300, 700)]:
        l = put_stars(rand_labels(rng, U, V, 0, rep=0.3), [0, U // 3, U // 2, U - 1], V)
        labels.append(l)
        xs.append(rng.integers(-1, 2, size=(max(T, U + AR.repeats(l)), V)).astype(np.float32))
    xs[2][:, 3] = -np.inf                                           # a column of -inf (some of the labels are 3)
    xs[3][41, 2] = np.nan                                           # one NaN logit: m_t ignores it
    xs[3][41, 4] = 7.0
    assert SR.frame_max(xs[3])[41] == 7.0
    got = align(torch_mod, xs, labels, star_score=0.0)              # the star ties with every frame's best token
    for g, x, l in zip(got, xs, labels):
        assert_reference_decisions(g, x, l, 0, 0.0)
    for i in (0, 1, 4):                                             # finite logits: the values too
        assert_reference_bits(got[i], xs[i], labels[i], 0, 0.0, "ties")
    # a NaN logit in the star's own frame range, at the default score
    x = rng.standard_normal((60, 32)).astype(np.float32)
    x[20, 5] = np.nan
    l = [4, 32, 9]
    g = align(torch_mod, [x], [l])[0]
    assert_reference_decisions(g, x, l, 0, -0.5)
    assert g[0][20] == 32 and np.isnan(g[2][20]) and np.isnan(g[3])       # lse_20 is NaN; m_20 is not


# ---- 5. bad utterances ---------------------------------------------------------------------------------------------------------
def test_bad_utterances_leave_neighbours_alone(torch_mod):
    rng = np.random.default_rng(8)
    V = 32
    xs = [rng.standard_normal((30, V)).astype(np.float32) for _ in range(5)]
    labels = [[3, V, 4, 9], [5, V + 1, 6], [V, 0, 6], [5, V, -1], [7, 7, V, 2]]
    rc, got = raw_align(torch_mod, xs, labels, 0, -0.5)
    assert rc == 0
    rc, clean = raw_align(torch_mod, [xs[0], xs[4]], [labels[0], labels[4]], 0, -0.5)
    assert rc == 0
    same_bits(got[0], clean[0])
    same_bits(got[4], clean[1])
    assert_reference_bits(got[0], xs[0], labels[0], 0, -0.5, "beside bad utterances")
    for i in (1, 2, 3):
        tok, li, fl, sc = got[i]
        assert np.isnan(sc) and (tok == -1).all() and (li == -1).all() and np.isnan(fl).all()
        assert np.isnan(SR.viterbi(xs[i], labels[i], 0, -0.5)[3])
    rc, lng = raw_align(torch_mod, xs, labels, 0, -0.5, long=(64, 8))
    assert rc == 0
    for a, b in zip(lng, got):
        same_bits(a, b)


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(torch_mod):
    rng = np.random.default_rng(23)
    V = 32
    labels = [put_stars(rand_labels(rng, U, V, 0), [0, U // 2, U - 1], V) for U in (50, 600, 9)]
    xs = [rng.standard_normal((len(l) + AR.repeats(l) + 20, V)).astype(np.float32) for l in labels]
    a, b = align(torch_mod, xs, labels), align(torch_mod, xs, labels)
    for u, v in zip(a, b):
        same_bits(u, v)


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(torch_mod):
    from wav2vec2 import _native as N
    from wav2vec2.alignment import forced_align, forced_align_long
    rng = np.random.default_rng(2)
    V = 8
    x = rng.standard_normal((6, V)).astype(np.float32)
    for bad in (float("nan"), 0.5, 1e-30):
        for long in (None, (64, 8)):
            rc, got = raw_align(torch_mod, [x], [[1, V]], 0, bad, long=long)
            assert rc != 0 and "star_score" in N.last_error(), (bad, long, N.last_error())
            assert (got[0][0] == -7).all()                          # nothing ran
        with pytest.raises(ValueError, match="star_score"):
            forced_align(dev(torch_mod, [x]), [[1, V]], star_score=bad)
        with pytest.raises(ValueError, match="star_score"):
            forced_align_long(dev(torch_mod, [x]), [[1, V]], star_score=bad)
    for sc in (0.0, -0.0, -1e-30, float("-inf")):
        rc, got = raw_align(torch_mod, [x], [[1, V]], 0, sc)
        assert rc == 0
    xd = dev(torch_mod, [x])
    with pytest.raises(ValueError, match=r"utterance 0: labels must lie in \[0, 8\)"):
        forced_align(xd, [[1, V]])                                  # the star without star_score
    with pytest.raises(ValueError, match="two stars next to each other"):
        forced_align(xd, [[1, V, V]], star_score=-0.5)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 8\]"):
        forced_align_long(xd, [[1, V + 1]], star_score=-0.5)
    lib = N.load()
    fr, nl = np.asarray([100], np.int32), np.asarray([70], np.int32)
    plain, star = lib.w2v2_ctc_align_long_workspace(1, N.ptr(fr), N.ptr(nl), 64, 8), lib.w2v2_ctc_align_long_star_workspace(1, N.ptr(fr), N.ptr(nl), 64, 8)
    assert star == plain + 1024                                     # xs: 100 fp64, rounded up to 256 bytes
    assert lib.w2v2_ctc_align_long_star_workspace(1, N.ptr(fr), N.ptr(nl), 96, 8) < 0 and "strip_pairs" in N.last_error()


# ---- 8. forced_align_long ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_cases():
    """recordings with stars at the strip boundary of 64 pairs (pairs 63 and 64), at labels 0 and U - 1, and with room for a
    star to span panels; shared by the tile geometries"""
    rng = np.random.default_rng(64)
    V = 32
    cases = []
    for U, ks, d in [(150, [0, 63, 149], 90), (200, [64, 128, 199], 70), (65, [64], 30), (64, [63], 17), (300, [0, 127, 191, 255, 299], 40)]:
        labels = put_stars(rand_labels(rng, U, V, 0, rep=0.15), ks, V)
        assert all(labels[k] == V for k in ks)
        T = U + AR.repeats(labels) + d
        cases.append((rng.standard_normal((T, V)).astype(np.float32) * 3, labels))
    return cases


@pytest.mark.parametrize("sp,pf", [(64, 8), (64, 16), (256, 64), (None, None)])
def test_long_equals_forced_align(torch_mod, long_cases, sp, pf):
    from wav2vec2.alignment import forced_align, forced_align_long
    xd = dev(torch_mod, [c[0] for c in long_cases])
    labels = [c[1] for c in long_cases]
    want = [host(a) for a in forced_align(xd, labels, star_score=-0.5)]
    got = [host(a) for a in forced_align_long(xd, labels, strip_pairs=sp, panel_frames=pf, star_score=-0.5)]
    for g, w in zip(got, want):
        same_bits(g, w)
    if pf is not None:                                              # a star's span crosses a panel boundary (steps p pf, p pf + 1)
        tok, li = want[0][0], want[0][1]
        t = np.arange(pf, tok.size - 1, pf)
        assert ((tok[t] == 32) & (tok[t + 1] == 32) & (li[t] == li[t + 1])).any()
    if sp is None:
        for g, (x, l) in zip(got, long_cases):
            assert_reference_bits(g, x, l, 0, -0.5, "long")
        one = forced_align_long(xd[2], labels[2], star_score=-0.5)          # one (T, V) tensor: one Alignment
        same_bits(host(one), want[2])


def test_long_9000_labels_match_reference(torch_mod):
    from wav2vec2.alignment import forced_align_long
    rng = np.random.default_rng(9000)
    V, U = 32, 9000
    labels = put_stars(rand_labels(rng, U, V, 0), [0, 1023, 1024, 4500, 8191, U - 1], V)
    T = U + AR.repeats(labels) + 500
    x = rng.standard_normal((T, V)).astype(np.float32) * 2
    got = host(forced_align_long(dev(torch_mod, [x])[0], labels, star_score=-0.5))
    assert (got[0] == V).sum() >= 5
    assert_reference_bits(got, x, labels, 0, -0.5, "9000 labels")


# ---- 9. model level ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_base(torch_mod):
    import wav2vec2
    from wav2vec2 import Wav2Vec2Processor
    cfg = H.case_config("tiny_base")
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights("tiny_base"))
    tokenizer = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))
    assert cfg.vocab_size == len(tokenizer.get_vocab())
    return cfg, m, tokenizer


def test_model_align_with_stars(torch_mod, tiny_base):
    from wav2vec2.alignment import forced_align, token_spans, word_spans, _logits_base
    cfg, m, tokenizer = tiny_base
    V = cfg.vocab_size
    tokens = tokenizer.get_vocab()
    vocab = {i: (" " if t == "|" else t) for t, i in tokens.items()}
    spf = 320 / 16000.0
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 9001, 24000)]
    texts = ["* SO IT GOES ON *", "* ALL * OF IT *", "* WE * SHALL SEE *"]
    got = m.align(waves, texts, tokenizer, star="*")
    logits = m.predict_packed(waves)
    enc = lambda t: list(tokenizer(t))
    ids = [[V] + enc("SO IT GOES ON") + [V], [V] + enc("ALL") + [V] + enc("OF IT") + [V], [V] + enc("WE") + [V] + enc("SHALL SEE") + [V]]
    als = forced_align(logits, ids, blank=cfg.pad_id, star_score=-0.5)
    want = [word_spans(token_spans(a), tokens["|"], spf, vocab, star_id=V) for a in als]
    assert got == want
    for w, t in zip(got, texts):
        assert [x.text for x in w] == t.split()
    for a, l, x in zip(als, ids, logits):
        assert_reference_bits(host(a), x.cpu().numpy(), l, cfg.pad_id, -0.5, "model")
    # free_ends writes the outer stars; ids may hold V; another star_score is passed on
    plain = ["SO IT GOES ON", "ALL * OF IT", "WE * SHALL SEE"]
    assert m.align(waves, plain, tokenizer, star="*", free_ends=True) == got
    assert m.align(waves[:1], plain[:1], tokenizer, free_ends=True) == got[:1]
    by_ids = m.align(waves, ids, delimiter_id=tokens["|"])
    assert [[(x.start_s, x.end_s, x.score) for x in w] for w in by_ids] == [[(x.start_s, x.end_s, x.score) for x in w] for w in got]
    assert by_ids[0][0].text == "*" and by_ids[0][1].text == tuple(tokens[c] for c in "SO")
    other = m.align(waves, texts, tokenizer, star="*", star_score=-3.0)
    als3 = forced_align(logits, ids, blank=cfg.pad_id, star_score=-3.0)
    assert other == [word_spans(token_spans(a), tokens["|"], spf, vocab, star_id=V) for a in als3]
    # without the new arguments: the call it was
    assert m.align(waves, ["SO IT GOES ON", "ALL OF IT", "WE SHALL SEE"], tokenizer) == \
        [word_spans(token_spans(a), tokens["|"], spf, vocab)
         for a in forced_align(logits, [list(tokenizer(t)) for t in ("SO IT GOES ON", "ALL OF IT", "WE SHALL SEE")], blank=cfg.pad_id)]
    # the packed views are read in place: nothing is copied
    base, row0, lens = _logits_base(logits, None)
    assert base.data_ptr() == min(l.data_ptr() for l in logits) and lens == [int(l.shape[0]) for l in logits]
    copies = forced_align([l.clone() for l in logits], ids, blank=cfg.pad_id, star_score=-0.5)
    for a, b in zip(als, copies):
        same_bits(host(a), host(b))


def test_model_align_long_with_stars(torch_mod, tiny_base):
    from wav2vec2.alignment import forced_align_long, token_spans, word_spans, split_at_pauses
    cfg, m, tokenizer = tiny_base
    V = cfg.vocab_size
    tokens = tokenizer.get_vocab()
    vocab = {i: (" " if t == "|" else t) for t, i in tokens.items()}
    spf = 320 / 16000.0
    window_s, margin_s = 6400 / 16000.0, 640 / 16000.0
    wave = np.random.default_rng(19).standard_normal(16000).astype(np.float32)
    kw = dict(window_s=window_s, margin_s=margin_s)
    got = m.align_long(wave, "* SO IT * GOES ON *", tokenizer, star="*", **kw)
    logits = m.predict_long(wave, window_s, margin_s)
    ids = [V] + list(tokenizer("SO IT")) + [V] + list(tokenizer("GOES ON")) + [V]
    al = forced_align_long(logits, ids, blank=cfg.pad_id, star_score=-0.5)
    assert got == word_spans(token_spans(al), tokens["|"], spf, vocab, star_id=V)
    assert [w.text for w in got] == "* SO IT * GOES ON *".split()
    assert_reference_bits(host(al), logits.cpu().numpy(), ids, cfg.pad_id, -0.5, "model, long")
    assert m.align_long(wave, "SO IT * GOES ON", tokenizer, star="*", free_ends=True, **kw) == got
    assert m.align_long([wave], ["* SO IT * GOES ON *"], tokenizer, star="*", **kw) == [got]
    assert [s.text for s in split_at_pauses(got, min_pause_s=10.0, star_text="*")] == ["SO IT", "GOES ON"]
