"""The edit distance kernel (w2v2_edit_distance, wav2vec2.metrics) against the plain-Python DP (tests/edit_reference.py):
every comparison is exact integer equality.  Stripe edges, long and thin pairs on both boundary-row paths, special token
values, a large mixed call with its permutation, duplication and repetition, aliasing, the C ABI's argument checks, and
Wav2Vec2ForCTC.evaluate end to end."""

import os

import numpy as np
import pytest

import edit_reference as ER
import helpers as H

pytestmark = pytest.mark.gpu

VOCAB = os.path.join(H.GOLDEN, "vocab.json")
_CACHE = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def reference(a, b):
    """(distance, substitutions, deletions, insertions), computed once per distinct pair of sequences"""
    key = (np.asarray(a, np.int64).tobytes(), np.asarray(b, np.int64).tobytes())
    if key not in _CACHE:
        _CACHE[key] = ER.edit_counts(np.asarray(a).tolist(), np.asarray(b).tolist())
    return _CACHE[key]


def as_tuple(c):
    assert c.hits == c.ref_len - c.substitutions - c.deletions and c.distance == c.substitutions + c.deletions + c.insertions
    return (c.distance, c.substitutions, c.deletions, c.insertions)


def check_pairs(hyps, refs):
    from wav2vec2.metrics import edit_distance
    got = edit_distance(hyps, refs)
    assert len(got) == len(hyps)
    for k, (g, a, b) in enumerate(zip(got, hyps, refs)):
        assert g.ref_len == len(b)
        assert as_tuple(g) == reference(a, b), (k, len(a), len(b))
    return got


def test_stripe_edges(torch_mod):
    """all (m, n) around the 64-row stripe and the 64-column group, over three symbols: nearly every cell ties"""
    rng = np.random.default_rng(0)
    sizes = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]
    hyps, refs = [], []
    for m in sizes:
        for n in sizes:
            hyps.append(rng.integers(0, 3, m).astype(np.int32))
            refs.append(rng.integers(0, 3, n).astype(np.int32))
    check_pairs(hyps, refs)


def test_long_and_thin(torch_mod):
    rng = np.random.default_rng(1)
    r = lambda n, k=4: rng.integers(0, k, n).astype(np.int32)
    same = r(1000, 7)
    hyps = [r(1), r(300), r(600), r(5000), r(64), same, rng.integers(0, 5, 300).astype(np.int32)]
    refs = [r(300), r(1), r(700), r(64), r(5000), same.copy(), rng.integers(10, 15, 200).astype(np.int32)]
    got = check_pairs(hyps, refs)
    assert as_tuple(got[5]) == (0, 0, 0, 0) and got[5].hits == 1000
    # disjoint alphabets: every reference token substituted, the extra hypothesis tokens inserted
    assert as_tuple(got[6]) == (300, 200, 0, 100)
    # the 5000-token reference is beyond the LDS row: the same pair through the workspace, and once more in the call
    assert as_tuple(got[4]) == reference(hyps[4], refs[4])
    again = check_pairs([hyps[4], hyps[4], r(3)], [refs[4], refs[4], refs[4]])
    assert again[0] == again[1] == got[4]


def test_special_values(torch_mod):
    from wav2vec2.metrics import edit_distance
    lo, hi = -2 ** 31, 2 ** 31 - 1
    hyps = [[lo, hi, -1, 0, hi], [ord("a"), ord("b")], [-5, -4, -3], [hi] * 70]
    refs = [[hi, lo, -1, hi], [ord("b"), ord("a")], [-5, -3], [hi] * 69 + [lo]]
    got = check_pairs(hyps, refs)
    assert as_tuple(got[1]) == (2, 0, 1, 1) and got[1].hits == 1          # `ab` against `ba`: no substitution
    assert as_tuple(got[2]) == (1, 0, 0, 1)
    assert as_tuple(edit_distance([[]], [[]])[0]) == (0, 0, 0, 0)
    assert as_tuple(edit_distance([[]], [[1, 2, 3]])[0]) == (3, 0, 3, 0)
    assert as_tuple(edit_distance([[1, 2, 3]], [[]])[0]) == (3, 0, 0, 3)


def test_large_mixed_call(torch_mod):
    """about 2000 pairs from one pool, short ones mixed with three long pairs: equal to the reference, and the same bits under
    a permutation, with pairs duplicated, and on a second call"""
    from wav2vec2.metrics import edit_distance_pairs
    rng = np.random.default_rng(2)
    pool = [rng.integers(0, 4, rng.integers(0, 131) if k % 3 == 0 else rng.integers(0, 41)).astype(np.int32) for k in range(150)]
    pool += [rng.integers(0, 4, n).astype(np.int32) for n in (200, 2100, 700, 400, 2300, 150)]
    pairs = [(int(h), int(r)) for h, r in rng.integers(0, 150, (1997, 2))]
    pairs[500:500] = [(150, 151)]
    pairs[1200:1200] = [(152, 153)]
    pairs.append((154, 155))
    got = edit_distance_pairs(pool, pairs)
    for (h, r), g in zip(pairs, got):
        assert as_tuple(g) == reference(pool[h], pool[r]) and g.ref_len == len(pool[r]), (h, r)
    assert edit_distance_pairs(pool, pairs) == got
    perm = rng.permutation(len(pairs))
    shuffled = edit_distance_pairs(pool, [pairs[i] for i in perm])
    assert shuffled == [got[i] for i in perm]
    dup = rng.integers(0, len(pairs), 700).tolist() + [500, 500, 1201, len(pairs) - 1]
    assert edit_distance_pairs(pool, [pairs[i] for i in dup]) == [got[i] for i in dup]
    # a pair alone
    for i in (0, 500, 1201):
        assert edit_distance_pairs(pool, [pairs[i]]) == [got[i]]


def test_aliasing_pool_against_itself(torch_mod):
    from wav2vec2.metrics import edit_distance_pairs
    rng = np.random.default_rng(3)
    base = rng.integers(0, 5, 90)
    pool = []
    for k in range(24):
        s = base.copy()
        s[rng.integers(0, 90, 6)] = rng.integers(0, 5, 6)
        pool.append(s[:rng.integers(0, 91)].astype(np.int32))
    K = len(pool)
    pairs = [(i, j) for i in range(K) for j in range(K)]
    got = edit_distance_pairs(pool, pairs)
    D = np.array([g.distance for g in got]).reshape(K, K)
    assert (np.diag(D) == 0).all() and (D == D.T).all()
    for (i, j), g in zip(pairs, got):
        t = got[j * K + i]
        # the transposed pair swaps deletions and insertions
        assert (g.substitutions, g.deletions, g.insertions) == (t.substitutions, t.insertions, t.deletions)
        if i <= j:
            assert as_tuple(g) == reference(pool[i], pool[j])


def test_argument_errors(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    assert N.EDIT_MAX_LEN == 65535
    ntok = 65535 + 8
    flat = np.full(ntok, 7, np.int32)
    flat[65535] = 9
    tokens = torch.from_numpy(flat).cuda()
    out = torch.full((2, 4), -77, dtype=torch.int32, device="cuda")

    def call(hyp0=(0, 0), hyp_len=(3, 4), ref0=(2, 1), ref_len=(2, 5), n_pairs=2, n_tokens=ntok, null=None):
        host = dict(hyp0=np.asarray(hyp0, np.int64), hyp_len=np.asarray(hyp_len, np.int32), ref0=np.asarray(ref0, np.int64),
                    ref_len=np.asarray(ref_len, np.int32))                 # (alive until the call returns)
        args = dict(tokens=N.ptr(tokens), out=N.ptr(out), **{k: N.ptr(v) for k, v in host.items()})
        if null:
            args[null] = None
        return lib.w2v2_edit_distance(args["tokens"], n_tokens, n_pairs, args["hyp0"], args["hyp_len"], args["ref0"], args["ref_len"],
                                      args["out"], N.current_stream())

    bad = [(dict(null=k), "null") for k in ("tokens", "hyp0", "hyp_len", "ref0", "ref_len", "out")]
    bad += [(dict(n_pairs=0), "pairs"), (dict(n_pairs=-3), "pairs"),
            (dict(hyp0=(0, -1)), "negative offset"), (dict(ref0=(-2, 0)), "negative offset"),
            (dict(hyp_len=(3, -1)), "negative length"), (dict(ref_len=(-1, 5)), "negative length"),
            (dict(hyp0=(0, ntok - 3)), "past"), (dict(ref0=(2, ntok)), "past"), (dict(n_tokens=5), "past"),
            (dict(hyp_len=(3, 65536), n_tokens=1 << 20), "at most 65535"), (dict(ref_len=(65536, 5), n_tokens=1 << 20), "at most 65535")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw                      # W2V2_EINVAL
        assert msg in N.last_error(), (kw, N.last_error())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -77).all()              # nothing was launched
    # the limit itself is legal; its partner of one token keeps the run short, and the cost reaches the top of the packed range
    assert call(hyp0=(0, 65535), hyp_len=(65535, 1), ref0=(65535, 0), ref_len=(1, 65535)) == 0, N.last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().tolist()
    assert got[0] == [65535, 1, 0, 65534] == list(reference(flat[:65535], flat[65535:65536]))
    assert got[1] == [65535, 1, 65534, 0]


@pytest.mark.parametrize("name", ["tiny_base"])
def test_model_evaluate(torch_mod, name):
    import wav2vec2
    from wav2vec2 import metrics as M
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)
    delim = tok.get_vocab()["|"]
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name))
    rng = np.random.default_rng(6)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (16000, 3001, 52345, 24000)]
    plain = m.transcribe(waves, tok, beam_width=16, nbest=4)
    # made-up references: each transcript with a word dropped, a word changed and a character changed, so that hits and errors mix
    refs = []
    for t in plain:
        w = t.text.split()
        w = w[1:2] + ["QZ"] + w[2:]
        refs.append(" ".join(w)[:-1] + " X")
    ev = m.evaluate(waves, refs, tok, beam_width=16, nbest=4)
    assert ev.transcripts == plain                       # transcribe is what it was
    words = lambda s: s.split()
    chars = lambda s: list(" ".join(s.split()))

    def rate(hyp_texts, split):
        tot = [ER.edit_counts(split(h), split(r)) for h, r in zip(hyp_texts, refs)]
        n = sum(len(split(r)) for r in refs)
        return sum(c[0] for c in tot) / n, sum(c[0] for c in tot), n, [c for c in tot]

    for got, split in ((ev.wer, words), (ev.cer, chars)):
        r, e, n, per = rate([t.text for t in plain], split)
        assert (got.rate, got.errors, got.ref_len) == (r, e, n)
        assert [as_tuple(c) for c in got.per_utterance] == per
    best = [min(ER.edit_counts(words(h), words(r))[0] for h in (t.texts or [""])) for t, r in zip(plain, refs)]
    assert ev.oracle_wer.errors == sum(best) and ev.oracle_wer.errors <= ev.wer.errors
    oracle, chosen = M.oracle_wer(plain, refs)
    assert oracle == ev.oracle_wer
    for t, r, k, b in zip(plain, refs, chosen, best):
        errs = [ER.edit_counts(words(h), words(r))[0] for h in t.texts]
        assert k == (errs.index(b) if errs else -1)
    assert m.evaluate(waves, refs, tok).oracle_wer is None
    # minimum Bayes risk on the same lists
    lists = [t.hypotheses for t in plain]
    pairs = [[(h.ids, h.total) for h in l] for l in lists]

    def id_words(ids):
        out, cur = [], []
        for x in list(ids) + [delim]:
            if x == delim:
                if cur:
                    out.append(tuple(cur))
                cur = []
            else:
                cur.append(x)
        return out

    for unit, split in (("word", id_words), ("char", list)):
        idx, risks = M.mbr_select(lists, tok, unit=unit, scale=0.7)
        want_idx, want_risks = ER.mbr_reference(pairs, split, 0.7)
        assert idx == want_idx
        for a, b in zip(risks, want_risks):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
