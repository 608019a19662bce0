"""Packed variable-length inference in the split precision modes "bf16x3" and "f16x2": the segment form of the split attention
kernel (csrc/attention_split.hip) must be bit-identical to the dense kernel run on each utterance alone; predict_packed must meet
the fp32 bar against HF fp64, match alone runs, stay bitwise isolated, report f16x2 saturation exactly when it happens, and leave
no stale value in the stream rows between utterances."""

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "f16x2"]
OP_MODE = {"fp32": 0, "bf16": 1, "bf16x3": 2, "f16x2": 3}      # W2V2_PRECISION_*
PLANES = {"bf16x3": (0, 3), "f16x2": (1, 2)}                   # W2V2_PLANES_*, planes per element


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    torch.cuda.set_device(0)
    return torch


def build(name, with_head=True, weights=None):
    import wav2vec2
    cfg = H.case_config(name)
    cls = wav2vec2.Wav2Vec2ForCTC if with_head else wav2vec2.Wav2Vec2Model
    m = cls(cfg, input_shape=(1, 2048))
    m.set_weights(H.case_weights(name, with_lm_head=with_head) if weights is None else weights)
    return m, cfg


@pytest.fixture(scope="module")
def base(torch_mod):
    """one base-width model (H = 768, 12 heads: the segment split kernel runs) for the whole module; each test sets its mode"""
    m, _ = build("base_sample_unpadded")
    yield m
    m.set_precision("fp32")


@pytest.fixture
def in_mode(base, request):
    """the base model in the test's mode, back in fp32 afterwards, with the f16x2 flag cleared on entry"""
    mode = request.param
    base.range_overflow()
    base.set_precision(mode)
    yield base, mode
    base.set_precision("fp32")


def packed(m, waves):
    return [o.numpy() for o in m.predict_packed(waves)]


def alone(m, w):
    return m(np.asarray(w, np.float32)[None]).numpy()[0]


def noise(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def stream_frames(m, lens):
    """frames of the aligned stream a packed call runs on: each utterance padded to a multiple of 320 samples"""
    return m.num_frames(int(sum(-(-int(n) // 320) * 320 for n in lens)))


# ---------------------------------------------------------------- 1. the kernel, bitwise --
@pytest.mark.parametrize("mode", MODES)
def test_segment_split_attention_is_bitwise_the_alone_kernel(torch_mod, mode):
    torch = torch_mod
    from wav2vec2 import _native as N
    lib = N.load()
    Hh, heads = 768, 12
    nfs = [1, 31, 64, 65, 255, 256, 257, 700]
    cu = np.concatenate([[0], np.cumsum(nfs)]).astype(np.int32)
    rows = int(cu[-1])
    qkv_h = (2.0 * np.random.default_rng(5).standard_normal((rows, 3 * Hh))).astype(np.float32)
    fmt, npl = PLANES[mode]
    keep = []

    def run_packed(qkv_np):
        qkv = torch.from_numpy(qkv_np).cuda()
        ctx = torch.full((rows, Hh), float("nan"), device="cuda")
        pl = torch.zeros(npl * rows * Hh, dtype=torch.int16, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        keep.extend([qkv, ctx, pl, flag])
        N.check(lib.w2v2_op_attention_packed(N.ptr(qkv), len(nfs), N.ptr(cu), N.ptr(ctx), N.ptr(pl), rows * Hh, N.ptr(flag), Hh, heads,
                                             N.current_stream()), "w2v2_op_attention_packed")
        torch.cuda.synchronize()
        return qkv, ctx, pl, int(flag.item())

    N.check(lib.w2v2_op_set_precision(OP_MODE[mode]))
    try:
        qkv, ctx, pl, flag = run_packed(qkv_h)
        assert flag == 0
        got = ctx.cpu().numpy()
        assert np.isfinite(got).all()
        for i, nf in enumerate(nfs):
            f0 = int(cu[i])
            one = torch.full((nf, Hh), float("nan"), device="cuda")
            q1 = qkv[f0:f0 + nf].contiguous()
            keep.extend([one, q1])
            N.check(lib.w2v2_op_attention(N.ptr(q1), None, N.ptr(one), 1, nf, Hh, heads, N.current_stream()), "w2v2_op_attention")
            assert np.array_equal(got[f0:f0 + nf], one.cpu().numpy()), (mode, nf)
        # the planes the kernel wrote are the split of its own fp32 output
        ref = torch.zeros_like(pl)
        flag2 = torch.zeros(1, dtype=torch.int32, device="cuda")
        keep.extend([ref, flag2])
        N.check(lib.w2v2_op_split_planes(N.ptr(ctx), N.ptr(ref), rows * Hh, rows * Hh, fmt, N.ptr(flag2), N.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(pl, ref)

        # one utterance's v past f16x2's scaled range (|v| >= 4094): the f16x2 kernel saturates it and says so; exact splits do not
        big = qkv_h.copy()
        big[cu[6]:cu[7], 2 * Hh:] *= 3000.0
        _, ctx_b, _, flag_b = run_packed(big)
        assert flag_b == (1 if mode == "f16x2" else 0)
        assert bool(torch.isfinite(ctx_b).all())
        # bf16 (the training policy) has no segment form
        N.check(lib.w2v2_op_set_precision(1))
        assert lib.w2v2_op_attention_packed(N.ptr(qkv), len(nfs), N.ptr(cu), N.ptr(ctx), None, 0, None, Hh, heads, N.current_stream()) == -1
        assert b"precision mode bf16" in lib.w2v2_last_error()
    finally:
        N.check(lib.w2v2_op_set_precision(0))


# ---------------------------------------------------------------- 2. HF fp64 --
def check_hf(m, mode, waves, refs, label):
    e32 = [H.max_err(o, r) for o, r in zip(packed(m, waves), refs)]
    m.set_precision(mode)
    try:
        outs = packed(m, waves)
    finally:
        m.set_precision("fp32")
    for b, (o, r) in enumerate(zip(outs, refs)):
        assert o.shape == r.shape
        err = H.max_err(o, r)
        print(f"{label}[{b}]: max|packed {mode} - HF fp64| = {err:.3e} (packed fp32 {e32[b]:.3e})")
        assert err < H.ATOL_AIM
        assert err < 1.5 * e32[b] + 2e-5


@pytest.mark.parametrize("mode", MODES)
def test_base_sample_matches_hf_f64(base, mode):
    g = H.golden("base_sample_unpadded")
    check_hf(base, mode, list(g["wave"]), list(g["logits_f64"]), "base_sample_unpadded")


@pytest.fixture(scope="module")
def robust(torch_mod):
    m, _ = build("robust_masked")
    return m


@pytest.mark.parametrize("mode", MODES)
def test_robust_valid_prefixes_match_hf_f64(robust, mode):
    """LayerNorm extractor, prenorm encoder, 16 heads of 64"""
    g = H.golden("robust_masked")
    lens = g["attention_mask"].sum(1).astype(int)
    refs = [g["logits_f64"][b, :robust.num_frames(n)] for b, n in enumerate(lens)]
    check_hf(robust, mode, [g["wave"][b, :n] for b, n in enumerate(lens)], refs, "robust_masked")


# ---------------------------------------------------------------- 3. alone and isolation --
def check_isolation(m, waves, ref):
    """replacing one utterance by noise leaves every other output bitwise unchanged; so does a permutation"""
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


@pytest.mark.parametrize("in_mode", MODES, indirect=True)
def test_base_width_matches_alone_and_is_isolated(in_mode):
    """12 utterances of 1-15 s: the stream is long enough for the plane-streaming GEMMs; then a smaller call in the same workspace"""
    m, mode = in_mode
    lens = np.random.default_rng(11).integers(16000, 15 * 16000, size=12)
    waves = [noise(300 + i, int(n)) for i, n in enumerate(lens)]
    outs = packed(m, waves)
    for i, (o, x) in enumerate(zip(outs, waves)):
        err = H.max_err(o, alone(m, x))
        print(f"{mode} base utterance {i} ({len(x)} samples, {o.shape[0]} frames): max|packed - alone| = {err:.2e}")
        assert err < H.ATOL_AIM
    check_isolation(m, waves, outs)
    few = packed(m, waves[3:6])
    for o, x in zip(few, waves[3:6]):
        assert H.max_err(o, alone(m, x)) < H.ATOL_AIM
    assert m.range_overflow() is False


# ---------------------------------------------------------------- 4. the range flag --
@pytest.mark.parametrize("in_mode", MODES, indirect=True)
def test_range_flag_stays_clear_on_normal_inputs(in_mode):
    """whatever a dense forward of another shape and a packed call of other lengths left in the buffers sets no flag"""
    m, mode = in_mode
    m(noise(40, 2 * 48000).reshape(2, 48000))
    packed(m, [noise(41 + i, n) for i, n in enumerate([70000, 23456, 150001])])
    outs = packed(m, [noise(50 + i, n) for i, n in enumerate([160000, 31999, 99999, 200000, 5000])])
    assert all(np.isfinite(o).all() for o in outs)
    assert m.range_overflow() is False


@pytest.fixture(scope="module")
def hot(torch_mod):
    """base_sample_padded's weights with +1e4 on layer 0's intermediate dense bias (test_f16x2_reports_values_beyond_its_range)"""
    w = H.case_weights("base_sample_padded")
    w["encoder/layers/0/feed_forward/intermediate_dense/bias"] = w["encoder/layers/0/feed_forward/intermediate_dense/bias"] + 1e4
    m, _ = build("base_sample_padded", weights=w)
    yield m
    m.set_precision("fp32")


@pytest.mark.parametrize("mode", MODES)
def test_range_flag_reports_saturation(hot, mode):
    g = H.golden("base_sample_padded")
    waves = list(g["wave"]) * 4           # 8 x 768 frames: every GEMM site streams planes, as in the dense test
    hot.range_overflow()
    hot.set_precision(mode)
    outs = packed(hot, waves)
    assert all(np.isfinite(o).all() for o in outs)
    assert hot.range_overflow() is (mode == "f16x2")
    assert hot.range_overflow() is False                  # reading clears it


# ---------------------------------------------------------------- 5. the gap rows --
@pytest.mark.parametrize("in_mode", MODES, indirect=True)
def test_gap_rows_depend_only_on_the_call(in_mode):
    """A, then B (other lengths, same workspace), then A again: every stream row of A's taps -- the 1-2 junk rows behind each
    utterance included -- comes out bit for bit the same, so nothing B left behind is read"""
    m, mode = in_mode
    lens_a, lens_b = [48000, 16399, 9999, 81234], [30000, 70001, 17777, 12345, 1000]
    wa = [noise(60 + i, n) for i, n in enumerate(lens_a)]
    wb = [noise(70 + i, n) for i, n in enumerate(lens_b)]
    m.set_option("keep_activations", True)
    try:
        packed(m, wa)
        first = {k: m.activation(k) for k in ("encoder_in", "layer0")}
        packed(m, wb)
        packed(m, wa)
        again = {k: m.activation(k) for k in ("encoder_in", "layer0")}
    finally:
        m.set_option("keep_activations", False)
    T = stream_frames(m, lens_a)
    for k in first:
        assert first[k].shape[0] == 1 and first[k].shape[1] >= T
        assert np.isfinite(first[k][0, :T]).all()
        assert np.array_equal(first[k][0, :T], again[k][0, :T]), k


# ---------------------------------------------------------------- 6. surface --
@pytest.mark.parametrize("mode", MODES)
def test_fp32_after_a_split_mode_is_unchanged_and_bf16_is_refused(base, mode):
    waves = [noise(80 + i, n) for i, n in enumerate([33333, 12000, 64000])]
    ref = packed(base, waves)
    base.set_precision(mode)
    try:
        split = packed(base, waves)
    finally:
        base.set_precision("fp32")
    assert not all(np.array_equal(a, b) for a, b in zip(ref, split))     # a split path did run
    assert all(np.array_equal(a, b) for a, b in zip(ref, packed(base, waves)))
    base.set_precision("bf16")
    try:
        with pytest.raises(RuntimeError, match="precision mode bf16"):
            base.predict_packed(waves)
    finally:
        base.set_precision("fp32")


@pytest.mark.parametrize("name", ["tiny_base", "tiny_robust"])
@pytest.mark.parametrize("mode", MODES)
def test_tiny_configs_match_alone(torch_mod, name, mode):
    """head size 32: the fp32 segment attention, then the split of its output where planes are wanted"""
    m, _ = build(name)
    m.set_precision(mode)
    waves = [noise(90 + i, n) for i, n in enumerate([400, 719, 16399, 9999, 52345, 3001])]
    for i, (o, x) in enumerate(zip(packed(m, waves), waves)):
        err = H.max_err(o, alone(m, x))
        print(f"{name} {mode} utterance {i} ({len(x)} samples): max|packed - alone| = {err:.2e}")
        assert err < H.ATOL_AIM
