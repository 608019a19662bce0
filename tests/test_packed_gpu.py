"""Packed variable-length inference (w2v2_forward_packed / predict_packed): every utterance of a packed call must come out as
its own B = 1 forward does -- against the HF fp64 fixtures, the fp64 oracle and alone runs -- and bit for bit independent of
its neighbours."""

import os

import numpy as np
import pytest

import helpers as H
from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def build(name, with_head=True):
    import wav2vec2
    cfg = H.case_config(name)
    cls = wav2vec2.Wav2Vec2ForCTC if with_head else wav2vec2.Wav2Vec2Model
    m = cls(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name, with_lm_head=with_head))
    return m, cfg


def packed(m, waves):
    return [o.numpy() for o in m.predict_packed(waves)]


def alone(m, w):
    return m(np.asarray(w, np.float32)[None]).numpy()[0]


def noise(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def gap_frames(m, n):
    """junk frames the stream carries behind an utterance of n samples (alignment unit 320 samples)."""
    return -(-n // 320) - m.num_frames(n)


def edge_lengths(m):
    """400 (one frame), 719 (one frame, maximal remainder), lengths behind which the stream has a 1-frame and a 2-frame gap,
    and one utterance longer than a 128-frame pos-conv tile and several 256-query attention tiles."""
    one = next(n for n in range(16000, 17000) if gap_frames(m, n) == 1)
    two = next(n for n in range(9000, 10000) if gap_frames(m, n) == 2)
    lens = [400, 719, one, two, 300000, 3001, 52345]
    assert m.num_frames(400) == 1 and m.num_frames(399) == 0 and m.num_frames(719) == 1 and m.num_frames(720) == 2
    assert gap_frames(m, one) == 1 and gap_frames(m, two) == 2 and m.num_frames(300000) > 3 * 256
    return lens


def test_base_sample_matches_hf_f64_and_is_not_padding(torch_mod):
    g = H.golden("base_sample_unpadded")
    m, _ = build("base_sample_unpadded")
    outs = packed(m, list(g["wave"]))
    for b, o in enumerate(outs):
        assert o.shape == g["logits_f64"][b].shape
        err = H.max_err(o, g["logits_f64"][b])
        print(f"base_sample_unpadded[{b}]: max|packed - HF fp64| = {err:.3e}")
        assert err < H.ATOL_AIM
        # padded to the notebooks' 246000 samples, the zeros enter conv0's GroupNorm statistics and move the valid frames
        pad = np.pad(g["wave"][b], (0, 246000 - g["wave"].shape[1]))
        assert np.abs(alone(m, pad)[:o.shape[0]] - o).max() > 0.1


@pytest.mark.parametrize("name", ["robust_masked", "tiny_robust"])
def test_masked_valid_prefixes_match_hf_f64(torch_mod, name):
    g = H.golden(name)
    m, _ = build(name)
    lens = g["attention_mask"].sum(1).astype(int)
    assert len(set(lens.tolist())) == 2
    outs = packed(m, [g["wave"][b, :n] for b, n in enumerate(lens)])
    for b, (o, n) in enumerate(zip(outs, lens)):
        T = m.num_frames(n)
        assert o.shape == (T, g["logits_f64"].shape[2])
        err = H.max_err(o, g["logits_f64"][b, :T])
        print(f"{name}[{b}] ({n} samples): max|packed - HF fp64| = {err:.3e}")
        assert err < H.ATOL_AIM


@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_segment_edges_match_alone_and_oracle(torch_mod, name):
    m, cfg = build(name)
    w = H.case_weights(name)
    lens = edge_lengths(m)
    waves = [noise(100 + i, n) for i, n in enumerate(lens)]
    outs = packed(m, waves)
    for i, (o, x) in enumerate(zip(outs, waves)):
        assert o.shape == (m.num_frames(len(x)), cfg.vocab_size)
        e_alone = H.max_err(o, alone(m, x))
        e_oracle = H.max_err(o, O.ctc_forward(cfg, w, x[None].astype(np.float64), dtype=np.float64)[0])
        print(f"{name} utterance {i} ({len(x)} samples): vs alone {e_alone:.2e}, vs fp64 oracle {e_oracle:.2e}")
        assert e_alone < H.ATOL_AIM and e_oracle < H.ATOL_AIM


def check_isolation(m, waves):
    """replacing one utterance by noise leaves every other output bitwise unchanged; so does a permutation."""
    ref = packed(m, waves)
    k = len(waves) // 2
    other = list(waves)
    other[k] = noise(999, len(waves[k]))
    out = packed(m, other)
    assert not np.array_equal(out[k], ref[k])
    for i in range(len(waves)):
        if i != k:
            assert np.array_equal(out[i], ref[i]), i
    perm = np.random.default_rng(7).permutation(len(waves))
    out = packed(m, [waves[j] for j in perm])
    for pos, j in enumerate(perm):
        assert np.array_equal(out[pos], ref[j]), (pos, j)


@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
def test_isolation_is_bitwise_tiny(torch_mod, name):
    m, _ = build(name)
    check_isolation(m, [noise(200 + i, n) for i, n in enumerate(edge_lengths(m))])


def test_base_width_matches_alone_and_is_isolated(torch_mod):
    """H = 768, 12 heads, 16 pos-conv groups, K = 128, on 12 utterances of 1-15 s; then a smaller call in the same workspace."""
    import wav2vec2
    from wav2vec2 import variables as V
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=3))
    lens = np.random.default_rng(11).integers(16000, 15 * 16000, size=12)
    waves = [noise(300 + i, int(n)) for i, n in enumerate(lens)]
    outs = packed(m, waves)
    for i, (o, x) in enumerate(zip(outs, waves)):
        err = H.max_err(o, alone(m, x))
        print(f"base utterance {i} ({len(x)} samples, {o.shape[0]} frames): max|packed - alone| = {err:.2e}")
        assert err < H.ATOL_AIM
    check_isolation(m, waves)
    few = packed(m, waves[3:6])
    for o, x in zip(few, waves[3:6]):
        assert H.max_err(o, alone(m, x)) < H.ATOL_AIM


def test_backbone_hidden_states(torch_mod):
    m, cfg = build("tiny_base", with_head=False)
    waves = [noise(400 + i, n) for i, n in enumerate([4000, 719, 12345])]
    outs = m.predict_packed(waves)
    assert [tuple(o.shape) for o in outs] == [(m.num_frames(len(x)), cfg.hidden_size) for x in waves]
    # views of one packed output
    assert all(o.untyped_storage().data_ptr() == outs[0].untyped_storage().data_ptr() for o in outs)
    for o, x in zip(outs, waves):
        assert H.max_err(o.numpy(), alone(m, x)) < H.ATOL_AIM


def test_torch_inputs_and_no_mask_warning(torch_mod, caplog):
    m, _ = build("tiny_robust")
    waves = [noise(500, 5000), noise(501, 3000)]
    with caplog.at_level("WARNING"):
        a = packed(m, [torch_mod.from_numpy(x).cuda() for x in waves])
    assert not caplog.records
    b = packed(m, waves)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_errors(torch_mod):
    from wav2vec2 import _native as N
    m, _ = build("tiny_base")
    with pytest.raises(ValueError, match="non-empty"):
        m.predict_packed([])
    with pytest.raises(ValueError, match="utterance 1 must be 1-D"):
        m.predict_packed([noise(1, 4000), noise(2, 8000).reshape(2, 4000)])
    with pytest.raises(ValueError, match="utterance 2 has 399 samples"):
        m.predict_packed([noise(1, 4000), noise(2, 400), noise(3, 399)])
    m.set_precision("bf16")
    with pytest.raises(RuntimeError, match="precision mode bf16"):
        m.predict_packed([noise(1, 4000)])
    m.set_precision("fp32")
    assert len(m.predict_packed([noise(1, 4000)])) == 1

    # the C ABI: a call before w2v2_finalize, and its own checks
    torch = torch_mod
    fresh, _ = build("tiny_base")
    wave = torch.from_numpy(noise(4, 16399)).cuda()
    out = torch.empty((64, 32), device="cuda")
    lib = fresh._lib

    def call(cu, n=None):
        cu = np.asarray(cu, np.int64)
        return lib.w2v2_forward_packed(fresh._handle, N.ptr(wave), len(cu) - 1 if n is None else n, N.ptr(cu), N.ptr(out),
                                       N.current_stream())

    assert call([0, 16000]) == -4                      # W2V2_ESTATE
    fresh._finalize()
    assert call([0, 16000, 16399]) == -1 and b"utterance 1" in lib.w2v2_last_error()
    assert call([0, 16000], n=0) == -1
    assert call([5, 16000]) == -1
    assert call([0, 16000]) == 0


def test_decode_of_sample_slices(torch_mod):
    import wave
    import wav2vec2
    with wave.open(os.path.join(H.GOLDEN, "sample.wav")) as f:
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0
    proc = wav2vec2.Wav2Vec2Processor(is_tokenizer=False)
    tok = wav2vec2.Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(H.GOLDEN, "vocab.json"))
    n = len(pcm)
    cuts = [(0, min(n, 40000)), (n // 4, n // 4 + min(n // 2, 30000)), (n // 3, n), (0, n)]
    xs = [proc(pcm[a:b]) for a, b in cuts]
    m, _ = build("base_sample_unpadded")
    outs = packed(m, xs)
    for x, o in zip(xs, outs):
        assert tok.decode(o.argmax(-1)) == tok.decode(alone(m, x).argmax(-1))
