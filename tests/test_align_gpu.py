"""CTC forced alignment on the GPU (w2v2_ctc_align, wav2vec2.alignment): the path bit-identical to the fp64 numpy reference
(tests/align_reference.py), exact ties, greedy consistency, isolation and determinism, bad utterances, the C ABI's argument
checks, and Wav2Vec2ForCTC.align on packed utterances."""

import ctypes as C

import numpy as np
import pytest

import align_reference as AR
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def rand_labels(rng, U, V, blank, rep=0.1):
    out = []
    for _ in range(U):
        if out and rng.random() < rep:
            out.append(out[-1])
        else:
            out.append(int(rng.choice([v for v in range(V) if v != blank])))
    return out


def host(al):
    return al.token.cpu().numpy(), al.label_index.cpu().numpy(), al.frame_logp.cpu().numpy(), al.score


def assert_matches_reference(al, x, labels, blank):
    tok, li, fl, sc = host(al)
    rtok, rli, rfl, rsc = AR.viterbi(x, labels, blank)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(li, rli)
    if np.isfinite(rsc):
        assert abs(sc - rsc) <= 1e-9 * max(1.0, abs(rsc)), (sc, rsc)
        np.testing.assert_allclose(fl, rfl, rtol=0, atol=1e-6)
    else:
        assert (np.isnan(sc) and np.isnan(rsc)) or sc == rsc, (sc, rsc)


def align(torch, xs, labels, blank=0):
    from wav2vec2.alignment import forced_align
    return forced_align([torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs], labels, blank=blank)


def raw_align(torch, xs, labels, blank=0):
    """the C ABI itself, labels on the device unchecked: (token, label_index, frame_logp, score) on the host, per utterance"""
    from wav2vec2 import _native as N
    lens = [x.shape[0] for x in xs]
    V = xs[0].shape[1]
    base = torch.from_numpy(np.concatenate(xs)).cuda()
    flat = np.concatenate([np.asarray(l, np.int32) for l in labels] + [np.zeros(1, np.int32)])
    lab = torch.from_numpy(flat).cuda()
    row0 = np.cumsum([0] + lens[:-1]).astype(np.int64)
    label0 = np.cumsum([0] + [len(l) for l in labels[:-1]]).astype(np.int64)
    frames = np.asarray(lens, np.int32)
    nlab = np.asarray([len(l) for l in labels], np.int32)
    tot, n = sum(lens), len(xs)
    tok = torch.empty(tot, dtype=torch.int32, device="cuda")
    li = torch.empty_like(tok)
    fl = torch.empty(tot, dtype=torch.float32, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    lib = N.load()
    N.check(lib.w2v2_ctc_align(N.ptr(base), V, n, N.ptr(row0), N.ptr(frames), N.ptr(lab), N.ptr(label0), N.ptr(nlab), blank,
                               N.ptr(tok), N.ptr(li), N.ptr(fl), N.ptr(sc), N.current_stream()))
    out, o = [], 0
    tok, li, fl, sc = tok.cpu().numpy(), li.cpu().numpy(), fl.cpu().numpy(), sc.cpu().numpy()
    for i, T in enumerate(lens):
        out.append((tok[o:o + T], li[o:o + T], fl[o:o + T], float(sc[i])))
        o += T
    return out


def same_bits(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    assert np.array_equal(np.float64(a[3]), np.float64(b[3]), equal_nan=True)


# ---- 1. bit-identity with the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,blank", [(32, 0), (400, 7)])
def test_random_logits_match_reference(torch_mod, V, blank):
    rng = np.random.default_rng(V)
    cases = []
    for U, T in [(0, 5), (1, 1), (1, 9), (3, 40), (17, 60), (40, 300), (120, 250), (255, 600)]:
        labels = rand_labels(rng, U, V, blank, rep=0.2)
        T = max(T, U + AR.repeats(labels))
        cases.append((rng.standard_normal((T, V)).astype(np.float32) * 3, labels))
    als = align(torch_mod, [c[0] for c in cases], [c[1] for c in cases], blank)
    for al, (x, labels) in zip(als, cases):
        assert_matches_reference(al, x, labels, blank)


@pytest.mark.parametrize("Us", [[1024], [1, 300, 1024, 5], [8191]])
def test_long_transcripts_match_reference(torch_mod, Us):
    rng = np.random.default_rng(sum(Us))
    cases = []
    for U in Us:
        labels = rand_labels(rng, U, 32, 0)
        T = max(int(2.2 * U) + 1, U + AR.repeats(labels))
        cases.append((rng.standard_normal((T, 32)).astype(np.float32) * 2, labels))
    als = align(torch_mod, [c[0] for c in cases], [c[1] for c in cases])
    for al, (x, labels) in zip(als, cases):
        assert_matches_reference(al, x, labels, 0)


def test_repeats_minimal_length_and_single_frame(torch_mod):
    rng = np.random.default_rng(5)
    labels = [[3, 3, 3, 5, 5, 7], [9, 9, 9, 9], [4], [], [6, 6, 2, 2, 2, 8]]
    Ts = [6 + 3, 4 + 3, 1, 1, 6 + 3 + 7]            # forced paths (T = U + R), T = 1, and one with room
    xs = [rng.standard_normal((T, 32)).astype(np.float32) for T in Ts]
    als = align(torch_mod, xs, labels)
    for al, x, l in zip(als, xs, labels):
        assert_matches_reference(al, x, l, 0)
    assert host(als[0])[0].tolist() == [3, 0, 3, 0, 3, 5, 0, 5, 7]


# ---- 2. exact ties ------------------------------------------------------------------------------------------------------------
def test_exact_ties(torch_mod):
    rng = np.random.default_rng(11)
    xs, labels = [], []
    for U, T in [(2, 9), (5, 20), (30, 90), (200, 500)]:
        l = rand_labels(rng, U, 6, 0, rep=0.3)
        labels.append(l)
        xs.append(rng.integers(-1, 2, size=(max(T, U + AR.repeats(l)), 6)).astype(np.float32))
    als = align(torch_mod, xs, labels)
    for al, x, l in zip(als, xs, labels):
        assert_matches_reference(al, x, l, 0)


# ---- 3. greedy consistency ----------------------------------------------------------------------------------------------------
def collapse(path, blank):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(int(p))
        prev = p
    return out


def test_greedy_path_is_recovered(torch_mod):
    rng = np.random.default_rng(3)
    xs = [rng.standard_normal((T, 32)).astype(np.float32) * 4 for T in (7, 120, 500)]
    paths = [x.argmax(1) for x in xs]
    for x in xs:
        srt = np.sort(x, axis=1)
        assert (srt[:, -1] > srt[:, -2]).all()
    als = align(torch_mod, xs, [collapse(p, 0) for p in paths])
    for al, x, p in zip(als, xs, paths):
        tok, li, fl, sc = host(al)
        np.testing.assert_array_equal(tok, p)
        best = float((x.astype(np.float64).max(1) - AR.lse(x)).sum())
        assert abs(sc - best) <= 1e-9 * max(1.0, abs(best))


# ---- 4. isolation and determinism ---------------------------------------------------------------------------------------------
def test_isolation_forms_and_determinism(torch_mod):
    torch = torch_mod
    from wav2vec2.alignment import forced_align
    rng = np.random.default_rng(21)
    Ts = [50, 7, 333, 128, 129, 90]
    labels = [rand_labels(rng, T // 3, 32, 0) for T in Ts]
    xs = [rng.standard_normal((T, 32)).astype(np.float32) for T in Ts]
    ref = [host(a) for a in align(torch, xs, labels)]
    same_bits_all = lambda got, want: [same_bits(g, w) for g, w in zip(got, want)]
    same_bits_all([host(a) for a in align(torch, xs, labels)], ref)                          # two calls
    xs2 = list(xs)
    xs2[2] = rng.standard_normal((Ts[2], 32)).astype(np.float32)
    got = [host(a) for a in align(torch, xs2, labels)]
    same_bits_all([g for i, g in enumerate(got) if i != 2], [r for i, r in enumerate(ref) if i != 2])
    perm = [3, 0, 5, 2, 1, 4]
    got = [host(a) for a in align(torch, [xs[i] for i in perm], [labels[i] for i in perm])]
    same_bits_all(got, [ref[i] for i in perm])
    # padded (B, Tmax, V) with junk behind each utterance
    Tm = max(Ts)
    pad = rng.standard_normal((len(Ts), Tm, 32)).astype(np.float32) * 50
    for b, x in enumerate(xs):
        pad[b, :x.shape[0]] = x
    got = [host(a) for a in forced_align(torch.from_numpy(pad).cuda(), labels, frame_lengths=Ts)]
    same_bits_all(got, ref)


# ---- 5. bad utterances ----------------------------------------------------------------------------------------------------------
def test_bad_utterances_leave_neighbours_alone(torch_mod):
    rng = np.random.default_rng(8)
    xs = [rng.standard_normal((T, 32)).astype(np.float32) for T in (40, 5, 30, 30, 30, 30, 40)]
    labels = [rand_labels(rng, 10, 32, 0), [3, 3, 3, 4], rand_labels(rng, 8, 32, 0), [5, 0, 6], [5, 32, 6], [5, -1],
              rand_labels(rng, 12, 32, 0)]
    xs[2][7, 13] = np.nan
    got = raw_align(torch_mod, xs, labels)
    clean = raw_align(torch_mod, [xs[0], xs[6]], [labels[0], labels[6]])
    same_bits(got[0], clean[0])
    same_bits(got[6], clean[1])
    tok, li, fl, sc = got[1]                                  # infeasible: 5 frames for 4 labels with 2 repeats
    assert sc == -np.inf and (tok == -1).all() and (li == -1).all()
    tok, li, fl, sc = got[2]                                  # a NaN logit: NaN score, the reference's path
    rtok, rli, _, rsc = AR.viterbi(xs[2], labels[2], 0)
    assert np.isnan(sc) and np.isnan(rsc)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(li, rli)
    for i in (3, 4, 5):                                       # a device label equal to the blank or outside [0, V)
        tok, li, fl, sc = got[i]
        assert np.isnan(sc) and (tok == -1).all() and (li == -1).all()


def test_python_raises_on_host_checkable_cases(torch_mod):
    rng = np.random.default_rng(2)
    x = [rng.standard_normal((5, 32)).astype(np.float32), rng.standard_normal((6, 32)).astype(np.float32)]
    with pytest.raises(ValueError, match="utterance 1: 6 frames cannot hold"):
        align(torch_mod, x, [[1], [2, 2, 2, 2]])
    with pytest.raises(ValueError, match="utterance 0: label 0 is the blank"):
        align(torch_mod, x, [[0], [1]])
    with pytest.raises(ValueError, match=r"utterance 1: labels must lie in \[0, 32\)"):
        align(torch_mod, x, [[1], [32]])


def test_c_abi_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    V = 8
    x = torch.zeros((4, V), device="cuda")
    lab = torch.ones(8192, dtype=torch.int32, device="cuda")
    tok = torch.empty(4, dtype=torch.int32, device="cuda")
    li, fl, sc = torch.empty_like(tok), torch.empty(4, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    row0, label0 = np.zeros(1, np.int64), np.zeros(1, np.int64)

    def call(logits=N.ptr(x), n=1, frames=(4,), nlab=(1,), blank=0, r0=row0, tokp=N.ptr(tok), lb0=label0):
        fr, nl = np.asarray(frames, np.int32), np.asarray(nlab, np.int32)
        return lib.w2v2_ctc_align(logits, V, n, N.ptr(r0), N.ptr(fr), N.ptr(lab), N.ptr(lb0), N.ptr(nl), blank, tokp, N.ptr(li),
                                  N.ptr(fl), N.ptr(sc), N.current_stream())

    assert call() == 0
    torch.cuda.synchronize()
    for kw, msg in [(dict(logits=None), "null"), (dict(tokp=None), "null"), (dict(n=0), "utterances"),
                    (dict(frames=(0,)), "frames"), (dict(nlab=(-1,)), "labels"), (dict(blank=V), "blank"),
                    (dict(blank=-1), "blank"), (dict(nlab=(8192,)), "at most 8191"),
                    (dict(r0=np.full(1, -1, np.int64)), "negative"), (dict(lb0=np.full(1, -1, np.int64)), "negative")]:
        assert call(**kw) != 0, kw
        assert msg in N.last_error(), (kw, N.last_error())
    torch.cuda.synchronize()


# ---- 6. model level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_base", "base"])
def test_model_align_word_spans_and_views(torch_mod, name):
    torch = torch_mod
    import wav2vec2
    from wav2vec2.alignment import forced_align, token_spans, word_spans, Alignment
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 52345, 24000)]
    logits = m.predict_packed(waves)
    hosts = [l.cpu().numpy() for l in logits]
    paths = [h.argmax(1) for h in hosts]
    ids = [collapse(p, cfg.pad_id) for p in paths]
    delim = 4
    spf = float(np.prod(cfg.strides)) / 16000.0
    words = m.align(waves, ids, delimiter_id=delim)
    for w, h, p, l in zip(words, hosts, paths, ids):
        lp = (h.astype(np.float64) - AR.lse(h)[:, None])[np.arange(len(p)), p].astype(np.float32)
        li = np.full(len(p), -1, np.int32)
        k = -1
        for t in range(len(p)):
            if p[t] != cfg.pad_id and (t == 0 or p[t] != p[t - 1]):
                k += 1
            if p[t] != cfg.pad_id:
                li[t] = k
        want = word_spans(token_spans(Alignment(p.astype(np.int32), li, lp, 0.0)), delim, spf)
        assert [(x.text, x.start_s, x.end_s) for x in w] == [(x.text, x.start_s, x.end_s) for x in want]
        np.testing.assert_allclose([x.score for x in w], [x.score for x in want], rtol=0, atol=1e-6)
    # the packed views in place, concatenated copies, and the padded form: the same bits
    views = forced_align(logits, ids)
    copies = forced_align([l.clone() for l in logits], ids)
    Tm = max(h.shape[0] for h in hosts)
    pad = torch.zeros((len(hosts), Tm, cfg.vocab_size), device="cuda")
    for b, l in enumerate(logits):
        pad[b, :l.shape[0]] = l
    padded = forced_align(pad, ids, frame_lengths=[h.shape[0] for h in hosts])
    for a, b, c in zip(views, copies, padded):
        same_bits(host(a), host(b))
        same_bits(host(a), host(c))


def test_views_are_read_in_place(torch_mod):
    from wav2vec2.alignment import _logits_base
    base = torch_mod.randn(30, 8, device="cuda")
    parts = list(torch_mod.split(base, [10, 5, 15]))
    got, row0, lens = _logits_base(parts, None)
    assert got.data_ptr() == base.data_ptr() and row0 == [0, 10, 15] and lens == [10, 5, 15]
