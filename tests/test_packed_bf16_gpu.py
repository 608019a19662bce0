"""Packed variable-length inference in the precision mode "bf16" (option "bf16_packed"; DESIGN.md sections 10 and 26).

The two segment kernels against the dense bf16 kernels on each utterance alone, bit for bit; the option's gate; the logits
against HF fp64 at the bar the dense mode is held to (what torch.autocast(bfloat16) costs the same model,
tests/golden/hf_bf16_autocast.json); the windowed route against dense bf16 runs of each window, bit for bit; isolation of
the utterances of one call, bit for bit; no value of an earlier call in a later one; and the entry points on top."""

import json
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

with open(os.path.join(H.GOLDEN, "hf_bf16_autocast.json")) as _f:
    HF_BF16_AUTOCAST = json.load(_f)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def build(name, weights=None):
    import wav2vec2
    m = wav2vec2.Wav2Vec2ForCTC(H.case_config(name), input_shape=(1, 2048))
    m.set_weights(H.case_weights(name) if weights is None else weights)
    return m


def bf16_packed(m):
    m.set_precision("bf16")
    m.set_option("bf16_packed", True)
    return m


@pytest.fixture(scope="module")
def base_weights():
    return H.case_weights("base_sample_unpadded")


@pytest.fixture(scope="module")
def base(torch_mod, base_weights):
    """one base-width model (H = 768, 12 heads of 64, 128 taps in 16 groups: both new kernels run) in "bf16" with the option on"""
    m = bf16_packed(build("base_sample_unpadded", base_weights))
    yield m
    m.set_option("bf16_packed", False)
    m.set_precision("fp32")


def packed(m, waves):
    return [o.numpy() for o in m.predict_packed(waves)]


def noise(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def bf16_round(x):
    """fp32 -> the nearest-even bf16, as its 16 bits (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---------------------------------------------------------------- 1. the attention kernel, bitwise --
def test_segment_bf16_attention_is_bitwise_the_alone_kernel(torch_mod):
    """1 / 2 / 3 / 4 / 5 key tiles (the ring's prologue with its clamped second tile), one and several query blocks, partly
    filled waves; the last utterance ends at the last row of buffers that are exactly the stream's size"""
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    Hh, heads = 768, 12
    nfs = [1, 31, 32, 33, 64, 65, 127, 128, 129, 193, 257]
    cu = np.concatenate([[0], np.cumsum(nfs)]).astype(np.int32)
    rows = int(cu[-1])
    qkv_h = np.random.default_rng(5).standard_normal((rows, 3 * Hh)).astype(np.float32)
    qkv_h[cu[7]:cu[8]] *= 30.0          # one utterance whose running maximum keeps moving
    qkv = torch.from_numpy(qkv_h).cuda()
    ctx = torch.full((rows, Hh), float("nan"), device="cuda")
    ctx16 = torch.full((rows, Hh), -1, dtype=torch.int16, device="cuda")      # 0xFFFF: a bf16 NaN
    N.check(lib.w2v2_op_attention_packed_bf16(N.ptr(qkv), None, len(nfs), N.ptr(cu), N.ptr(ctx), N.ptr(ctx16), Hh, heads, N.current_stream()),
            "w2v2_op_attention_packed_bf16")
    torch.cuda.synchronize()
    got, got16 = ctx.cpu().numpy(), ctx16.cpu().numpy().view(np.uint16)
    assert np.isfinite(got).all()                   # every row was written
    assert not (got16 == 0xFFFF).all(axis=1).any()
    keep = []
    N.check(lib.w2v2_op_set_precision(1))
    try:
        for i, nf in enumerate(nfs):
            f0 = int(cu[i])
            one = torch.full((nf, Hh), float("nan"), device="cuda")
            q1 = qkv[f0:f0 + nf].contiguous()
            keep.extend([one, q1])
            N.check(lib.w2v2_op_attention(N.ptr(q1), None, N.ptr(one), 1, nf, Hh, heads, N.current_stream()), "w2v2_op_attention")
            ref = one.cpu().numpy()
            assert np.array_equal(got[f0:f0 + nf], ref), nf
            assert np.array_equal(got16[f0:f0 + nf], bf16_round(ref)), nf
    finally:
        N.check(lib.w2v2_op_set_precision(0))
    # only the shadow asked for, from the caller's own shadow of qkv: the same bits
    q16 = torch.from_numpy(bf16_round(qkv_h).view(np.int16)).cuda()
    only16 = torch.full((rows, Hh), -1, dtype=torch.int16, device="cuda")
    N.check(lib.w2v2_op_attention_packed_bf16(None, N.ptr(q16), len(nfs), N.ptr(cu), None, N.ptr(only16), Hh, heads, N.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(only16, ctx16)


# ---------------------------------------------------------------- 2. the positional conv, bitwise --
def test_segment_bf16_pos_conv_is_bitwise_the_alone_kernel(torch_mod):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    Hh, K, G = 768, 128, 16
    cg = Hh // G
    nfs = [1, 2, 63, 64, 65, 127, 128, 129, 300]
    cu = np.concatenate([[0], np.cumsum(nfs)]).astype(np.int32)
    rows = int(cu[-1])
    rng = np.random.default_rng(9)
    x_h = rng.standard_normal((rows, Hh)).astype(np.float32)
    wg = torch.from_numpy((rng.standard_normal((G, K, cg, cg)) / np.sqrt(K * cg)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(Hh).astype(np.float32)).cuda()
    w16 = torch.zeros(G * K * cg * cg, dtype=torch.int16, device="cuda")
    N.check(lib.w2v2_op_pos_conv_weight_shadow(N.ptr(wg), N.ptr(w16), K, cg, G, N.current_stream()))

    def run_packed(x_np):
        x = torch.from_numpy(x_np).cuda()
        y = torch.full((rows, Hh), float("nan"), device="cuda")
        N.check(lib.w2v2_op_pos_conv_packed_bf16(N.ptr(x), N.ptr(w16), N.ptr(bias), len(nfs), N.ptr(cu), N.ptr(y), Hh, K, G, 1, N.current_stream()),
                "w2v2_op_pos_conv_packed_bf16")
        torch.cuda.synchronize()
        return y.cpu().numpy()

    got = run_packed(x_h)
    assert np.isfinite(got).all()
    keep = []
    for i, nf in enumerate(nfs):
        f0 = int(cu[i])
        x1 = torch.from_numpy(x_h[f0:f0 + nf]).cuda()
        y1 = torch.full((nf, Hh), float("nan"), device="cuda")
        pack = torch.zeros(lib.w2v2_op_pos_conv_bf16_pack_elems(1, nf, Hh, K), dtype=torch.int16, device="cuda")
        keep.extend([x1, y1, pack])
        N.check(lib.w2v2_op_pos_conv_bf16(N.ptr(x1), N.ptr(w16), N.ptr(bias), None, N.ptr(y1), None, N.ptr(pack), None, 1, nf, Hh, K, G, 1, K // 2, 1,
                                          N.current_stream()), "w2v2_op_pos_conv_bf16")
        assert np.array_equal(got[f0:f0 + nf], y1.cpu().numpy()), nf
    # an utterance shorter than K / 2 frames sees nothing of its neighbours: every other utterance 1e4 times as loud changes no bit of it
    short = [i for i, nf in enumerate(nfs) if nf < K // 2]
    assert short == [0, 1, 2]
    for i in short:
        loud = 1e4 * x_h
        loud[cu[i]:cu[i + 1]] = x_h[cu[i]:cu[i + 1]]
        got2 = run_packed(loud.astype(np.float32))
        assert np.array_equal(got2[cu[i]:cu[i + 1]], got[cu[i]:cu[i + 1]]), nfs[i]
        assert not np.array_equal(got2[cu[i + 1]:cu[i + 2]], got[cu[i + 1]:cu[i + 2]])


# ---------------------------------------------------------------- 3. the option --
def test_option_off_is_the_refusal_and_on_runs(torch_mod):
    from wav2vec2.processor import Wav2Vec2Processor
    m = build("tiny_base")
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))
    waves = [noise(1, 4000), noise(2, 700)]
    assert m.get_option("bf16_packed") is False
    m.set_precision("bf16")
    with pytest.raises(RuntimeError, match="precision mode bf16"):
        m.predict_packed(waves)
    with pytest.raises(RuntimeError, match='the model is in "bf16"'):
        m.stream(tok)
    m.set_option("bf16_packed", True)
    assert m.get_option("bf16_packed") is True
    outs = packed(m, waves)
    assert [o.shape[0] for o in outs] == [m.num_frames(4000), m.num_frames(700)] and all(np.isfinite(o).all() for o in outs)
    s = m.stream(tok, window_s=0.4, margin_s=0.04)
    s.feed([noise(3, 9000)])
    assert s.finish()[0].hypotheses
    m.set_option("bf16_packed", False)
    with pytest.raises(RuntimeError, match="precision mode bf16"):
        m.predict_packed(waves)
    m.set_precision("fp32")
    ref = packed(m, waves)
    m.set_option("bf16_packed", True)                  # no effect outside "bf16"
    assert all(np.array_equal(a, b) for a, b in zip(ref, packed(m, waves)))


# ---------------------------------------------------------------- 4. HF fp64, the external bar --
def fixture_utterances(name):
    """the fixture's rows as whole utterances the packed forward can take, and their HF fp64 logits.  tiny_robust's logits were
    made under an attention mask: its rows are taken without the mask, as their valid prefixes, whose frames the mask leaves as
    an unmasked run of the prefix computes them (tests/test_packed_gpu.py::test_masked_valid_prefixes_match_hf_f64)"""
    g = H.golden(name)
    cfg = H.case_config(name)
    lens = g["attention_mask"].sum(1).astype(int) if "attention_mask" in g else [g["wave"].shape[1]] * g["wave"].shape[0]
    waves, refs = [], []
    for b, n in enumerate(lens):
        t = int(n)
        for k, s in zip(cfg.kernal_sizes, cfg.strides):
            t = 1 + (t - k) // s
        assert 1 <= t <= g["logits_f64"].shape[1]
        if "attention_mask" in g:
            assert g["attention_mask"][b, :n].all() and not g["attention_mask"][b, n:].any()
        else:
            assert t == g["logits_f64"].shape[1]
        waves.append(np.ascontiguousarray(g["wave"][b, :n]))
        refs.append(g["logits_f64"][b, :t])
    return waves, refs


@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust", "base_sample_unpadded"])
def test_packed_bf16_meets_the_autocast_bar_against_hf_f64(torch_mod, base, name):
    """tiny_*: head size 32, so attention is the fp32 segment kernel (the fallback route) and the positional conv the new one;
    base: both new kernels"""
    waves, refs = fixture_utterances(name)
    m = base if name == "base_sample_unpadded" else bf16_packed(build(name))
    extra = [noise(31, 5000), noise(32, 1234)]
    outs = packed(m, [extra[0]] + waves + [extra[1]])[1:-1]
    bar = HF_BF16_AUTOCAST[name]["autocast_bf16_max_abs_err"]
    for b, (o, r) in enumerate(zip(outs, refs)):
        assert o.shape == r.shape
        err = H.max_err(o, r)
        print(f"{name}[{b}]: max|packed bf16 - HF fp64| = {err:.3e} (HF autocast(bf16): {bar:.3e})")
        assert np.isfinite(o).all() and err <= bar, (err, bar)


# ---------------------------------------------------------------- 5. the windowed route, bitwise --
def test_windows_equal_dense_bf16_runs_bitwise(torch_mod, base):
    from wav2vec2.longform import predict_long, window_plan
    m = base
    wave = noise(40, 80000)
    window, margin = 32000, 3200
    plan = window_plan(len(wave), window, margin, m.config)
    assert len(plan) >= 3 and len({w.samples for w in plan}) >= 2        # one window shorter than the rest
    out = predict_long(m, wave, normalize=False, window=window, margin=margin).numpy()
    assert out.shape[0] == m.num_frames(len(wave))
    for w in plan:
        ref = m(wave[w.sample0:w.sample0 + w.samples][None]).numpy()[0][w.keep0:w.keep0 + w.keepn]
        got = out[w.out0:w.out0 + w.keepn]
        assert np.array_equal(got, ref), (w, H.max_err(got, ref))


# ---------------------------------------------------------------- 6. isolation, bitwise --
SET_LENS = [400, 4000, 12345, 33333, 64000]


def the_set():
    return [noise(50 + i, n) for i, n in enumerate(SET_LENS)]


@pytest.fixture(scope="module")
def set_outputs(base):
    """the five utterances through one packed bf16 call, computed once for the tests that compare against it"""
    outs = packed(base, the_set())
    for o in outs:
        o.setflags(write=False)
    return outs


def test_isolation_is_bitwise(base, set_outputs):
    waves, ref = the_set(), set_outputs
    assert ref[0].shape[0] == 1 and all(np.isfinite(o).all() for o in ref)
    perm = [3, 0, 4, 2, 1]
    out = packed(base, [waves[j] for j in perm])
    for pos, j in enumerate(perm):
        assert np.array_equal(out[pos], ref[j]), ("permutation", pos, j)
    same = list(waves)
    same[2] = noise(999, SET_LENS[2])               # a neighbour of the same length: every launch keeps its shape
    out = packed(base, same)
    assert not np.array_equal(out[2], ref[2])
    for i in (0, 1, 3, 4):
        assert np.array_equal(out[i], ref[i]), ("same length", i)
    other = list(waves)
    other[2] = noise(998, 20001)                    # another length: the stream's rows, and with them GEMM tiles, change
    out = packed(base, other)
    for i in (0, 1, 3, 4):
        assert np.array_equal(out[i], ref[i]), ("other length", i)


# ---------------------------------------------------------------- 7. no stale rows --
def test_nothing_of_a_non_finite_call_survives(torch_mod, base, base_weights, set_outputs):
    """a longer stream of samples 1e30 times the usual, then one whose samples overflow fp32 altogether (conv0's GroupNorm takes its
    statistics in fp64 and can normalise the first back into range; nothing survives the second), then the five utterances"""
    hot = [noise(60, 90000), noise(61, 70001), noise(62, 30000)]
    for scale in (1e30, 3e38):
        with np.errstate(over="ignore"):
            outs = packed(base, [(scale * w).astype(np.float32) for w in hot])
        print(f"samples x {scale:g}: finite outputs {[bool(np.isfinite(o).all()) for o in outs]}")
    assert not all(np.isfinite(o).all() for o in outs)
    outs = packed(base, the_set())
    assert all(np.isfinite(o).all() for o in outs)
    fresh = packed(bf16_packed(build("base_sample_unpadded", base_weights)), the_set())
    for i, (a, b, c) in enumerate(zip(outs, fresh, set_outputs)):
        assert np.array_equal(a, b), i
        assert np.array_equal(a, c), i


# ---------------------------------------------------------------- 8. the entry points --
def test_transcribe_and_stream_in_bf16(torch_mod):
    from wav2vec2.decoding import beam_search
    from wav2vec2.longform import predict_long
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))
    m = bf16_packed(build("tiny_base"))
    assert m.config.vocab_size == len(tok.get_vocab())
    got = m.transcribe([noise(70, 16000), noise(71, 5000)], tok, beam_width=4)
    assert len(got) == 2 and all(isinstance(t.text, str) and t.hypotheses for t in got)

    window, margin = 6400, 640
    waves = [noise(72, 3 * (window - 2 * margin) + window + 1), noise(73, 2 * (window - 2 * margin) + window + 719)]
    blank = m.config.pad_id
    want = [beam_search([predict_long(m, w, normalize=True, window=window, margin=margin)], beam_width=8, nbest=2, blank=blank)[0] for w in waves]
    s = m.stream(tok, n_streams=2, window_s=window / 16000.0, margin_s=margin / 16000.0, beam_width=8, nbest=2)
    assert (s.window, s.margin) == (window, margin)
    rng = np.random.default_rng(5)
    pos = [0, 0]
    while any(p < len(w) for p, w in zip(pos, waves)):
        chunks = []
        for j, w in enumerate(waves):
            c = int(rng.integers(1, 7000)) if j == 0 else 3200
            chunks.append(None if pos[j] >= len(w) else w[pos[j]:pos[j] + c])
            if chunks[-1] is not None:
                pos[j] += len(chunks[-1])
        s.feed(chunks)

    def bits(hyps):
        return [(h.ids, int(np.float64(h.score).view(np.int64)), int(np.float64(h.total).view(np.int64))) for h in hyps]

    for j, t in enumerate(s.finish()):
        assert bits(t.hypotheses) == bits(want[j]), j
        assert t.text == want[j][0].text(tok)
