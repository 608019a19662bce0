"""The extended optimizer on the GPU: gradient accumulation, clipping by the global norm, AdamW, non-finite
step skip.  Operator level: the two norm kernels over raw buffers that reach every chunk edge (w2v2_op_grad_norm), against
numpy in fp64.  Trainer level: tiny_base at L = 4000 (dropout 0, no spec-augment unless said), against the default Trainer
(bit for bit where the arithmetic is the same) and against oracle/w2v2_torch_train.py::adam_reference in fp64."""

import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
from oracle import w2v2_torch_train as TT
from wav2vec2 import _native as N
from wav2vec2 import variables as V
from wav2vec2.config import Wav2Vec2Config

pytestmark = pytest.mark.gpu

L = 4000
KERNEL = "encoder/layers/1/feed_forward/output_dense/kernel"      # (128, 64): two whole chunks
BIAS = "encoder/layers/1/feed_forward/output_dense/bias"
GAMMA = "encoder/layers/1/layer_norm/gamma"


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


# ------------------------------------------------------------------ operator: w2v2_op_grad_norm ----
SIZES = [1, 3, 4095, 4096, 4097, 70001, 1200003]      # the last: 293 partials for the 256 threads of the finishing block


@functools.lru_cache(maxsize=None)
def gradient(n, planted=True):
    """(g fp32 with a handful of +-1e18 planted -- their squares overflow fp32 --, its sum of squares in fp64).  Read-only.
    The planted squares (1e36) hide everything else from an fp64 sum, so `planted=False` checks the ordinary elements."""
    g = V.hash_normal(f"opt/g{n}", n, 5).astype(np.float32)
    for k, i in enumerate(sorted({0, n // 3, n // 2, (2 * n) // 3, n - 1}) if planted else ()):
        g[i] = 1e18 if k % 2 == 0 else -1e18
    g.setflags(write=False)
    return g, float(np.sum(g.astype(np.float64) ** 2))


def op_grad_norm(env, g_dev, n, max_norm=0.0, skip_nonfinite=0):
    lib, torch, dev = env
    rec = torch.full((C.sizeof(N.W2V2OptStats),), 0xFF, dtype=torch.uint8, device=dev)       # (the call clears it itself)
    N.check(lib.w2v2_op_grad_norm(N.ptr(g_dev), n, float(max_norm), skip_nonfinite, N.ptr(rec), N.current_stream()), "w2v2_op_grad_norm")
    return N.W2V2OptStats.from_buffer_copy(rec.cpu().numpy().tobytes())


def ulp_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("planted", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_sum_of_squares_norm_and_clip_factor(env, n, planted):
    """sumsq against numpy's fp64 sum to 1e-13 relative: both sides add non-negative terms at a depth of at most ~40 additions
    (numpy pairwise; the kernels 16 per thread + 8 tree levels + <= 2 + 8 in the finish), each within 40 * 2^-53 = 4.4e-15 of the
    exact sum; the bar leaves an order of magnitude over the sum of the two.  The clip factor to 1 ulp of fp32; two runs agree
    bit for bit."""
    _, torch, dev = env
    g, want = gradient(n, planted)
    t = torch.from_numpy(np.array(g)).to(dev)
    norm64 = np.sqrt(want)
    max_norm = float(np.float32(0.5 * norm64))
    st = op_grad_norm(env, t, n, max_norm)
    rel = abs(st.sumsq - want) / want
    print(f"n = {n}, planted {planted}: sumsq {st.sumsq!r} vs {want!r}, relative error {rel:.3e}; norm {st.norm!r}; scale {st.scale!r}")
    assert rel <= 1e-13
    assert st.norm == np.float32(norm64) or ulp_apart(st.norm, norm64) <= 1
    assert ulp_apart(st.scale, np.float32(min(1.0, max_norm / (norm64 + 1e-6)))) <= 1
    assert (st.nonfinite, st.skip, st.skipped_total) == (0, 0, 0)
    again = op_grad_norm(env, t, n, max_norm)
    assert np.float64(again.sumsq).view(np.int64) == np.float64(st.sumsq).view(np.int64)
    # clipping off, and a bound above the norm: the factor is exactly 1
    assert op_grad_norm(env, t, n, 0.0).scale == 1.0
    assert op_grad_norm(env, t, n, float(np.float32(4.0 * norm64))).scale == 1.0


def test_unaligned_buffer_takes_the_scalar_path(env):
    """A buffer that starts 4 bytes past a 16-byte boundary: every chunk is read with scalar loads, to the same accuracy."""
    _, torch, dev = env
    g, _ = gradient(70001)
    t = torch.from_numpy(np.array(g)).to(dev)[1:]
    want = float(np.sum(g[1:].astype(np.float64) ** 2))
    st = op_grad_norm(env, t, 70000)
    assert abs(st.sumsq - want) / want <= 1e-13


def test_zero_gradient(env):
    _, torch, dev = env
    st = op_grad_norm(env, torch.zeros(4097, device=dev), 4097, 1.0, 1)
    assert (st.sumsq, st.norm, st.scale, st.nonfinite, st.skip) == (0.0, 0.0, 1.0, 0, 0)


@pytest.mark.parametrize("where", ["first", "last", 4095, 4096])
@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
def test_non_finite_detection(env, where, value):
    _, torch, dev = env
    n = 70001
    g, _ = gradient(n)
    t = torch.from_numpy(np.array(g)).to(dev)
    t[{"first": 0, "last": n - 1}.get(where, where)] = float(value)
    for skip_nonfinite in (0, 1):
        st = op_grad_norm(env, t, n, 1.0, skip_nonfinite)
        assert st.nonfinite == 1 and st.skip == skip_nonfinite and st.skipped_total == skip_nonfinite
        assert not np.isfinite(st.norm)


def test_nothing_planted_leaves_the_flags_clear(env):
    _, torch, dev = env
    g, _ = gradient(70001)
    st = op_grad_norm(env, torch.from_numpy(np.array(g)).to(dev), 70001, 1.0, 1)
    assert (st.nonfinite, st.skip, st.skipped_total) == (0, 0, 0) and np.isfinite(st.norm)


# ------------------------------------------------------------------ Trainer ---------------------------
def build(name, vocab_size=None):
    """tests/test_train_gpu.py's recipe; `vocab_size` = 31 gives lm_head/bias a 3-element scalar tail (every slot of tiny_base
    is a multiple of four elements)."""
    import wav2vec2
    cfg = H.case_config(name) if vocab_size is None else Wav2Vec2Config(**H.TINY, vocab_size=vocab_size)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(2, L))
    w = H.case_weights(name) if vocab_size is None else V.seeded_weights(cfg, seed=0)
    m.set_weights(w)
    m.freeze_feature_extractor()
    return m, cfg, w


def trainer(vocab_size=None, B=2, division_factor=2, **kw):
    import wav2vec2
    m, cfg, w = build("tiny_base", vocab_size)
    kw.setdefault("learning_rate", 1e-3)
    tr = wav2vec2.Trainer(m, wav2vec2.CTCLoss(cfg, (B, L), division_factor=division_factor), dropout=kw.pop("dropout", 0.0),
                          apply_spec_augment=False, **kw)
    return m, tr, w


def batch():
    g = H.golden("tiny_base")
    return g["wave"], g["labels"]


def forward_backward(tr, x, labels):
    logits = tr.forward(x, step_seed=1)
    _, dlog = tr.loss.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)


def snapshot(m, tr):
    """Every variable and both moment buffers, on the host."""
    am, av = tr._adam_views()
    return m.get_weights(), am.cpu().numpy().copy(), av.cpu().numpy().copy()


def same_bits(a, b):
    return (all(np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)) for k in a[0])
            and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def variable(m, name):
    return [v for v in m.variables if v.local_name == name][0].numpy()


@pytest.mark.parametrize("vocab_size", [None, 31])
def test_clip_and_skip_that_never_fire_equal_the_default_trainer(env, vocab_size):
    """max_grad_norm = 1e30 and skip_nonfinite route the step through grad_norm + adamw_multi with scale == 1, wd == 0, skip == 0:
    every variable and both moments bit-identical to adam_multi_kernel after three steps."""
    x, labels = batch()
    m0, t0, _ = trainer(vocab_size)
    m1, t1, _ = trainer(vocab_size, max_grad_norm=1e30, skip_nonfinite=True)
    for _ in range(3):
        l0, l1 = float(t0.step(x, labels)), float(t1.step(x, labels))
        assert l0 == l1
    a, b = snapshot(m0, t0), snapshot(m1, t1)
    assert np.abs(a[1]).max() > 0 and np.abs(a[2]).max() > 0
    assert same_bits(a, b)
    assert t1.last_clip_scale == 1.0 and t1.last_grad_norm > 0 and t1.skipped_steps == 0
    assert t0._optimizer_stats() == (0.0, 1.0, 0, 0)          # the default path never created the record


def test_adamw_step_needs_a_norm_since_the_backward(env):
    lib = env[0]
    x, labels = batch()
    m, tr, _ = trainer(max_grad_norm=1.0)
    forward_backward(tr, x, labels)
    assert lib.w2v2_adamw_step(m._handle, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1, N.current_stream()) == -4      # W2V2_ESTATE
    tr.apply_gradients()
    forward_backward(tr, x, labels)                                                                      # a new gradient: the old record is stale
    assert lib.w2v2_adamw_step(m._handle, 1e-3, 0.9, 0.999, 1e-7, 0.0, 2, N.current_stream()) == -4


def test_clipping(env):
    x, labels = batch()
    m, tr, w = trainer(max_grad_norm=1.0)
    forward_backward(tr, x, labels)
    g = tr.grad_buffer().cpu().numpy().astype(np.float64)           # (frozen slots and padding are zero: the norm of the trainable set)
    norm64 = float(np.sqrt(np.sum(g * g)))
    tr.max_grad_norm = float(np.float32(0.5 * norm64))
    scale = np.float32(min(1.0, tr.max_grad_norm / (norm64 + 1e-6)))
    grads = {n: tr.gradient(n) for n in (KERNEL, BIAS)}
    tr.apply_gradients()
    assert abs(tr.last_grad_norm - norm64) <= 1e-6 * norm64
    assert ulp_apart(tr.last_clip_scale, scale) <= 1 and 0.49 < float(scale) < 0.51
    for n, gr in grads.items():
        clipped = (gr * scale).astype(np.float32).astype(np.float64)
        want, _, _ = TT.adam_reference(w[n].astype(np.float64), clipped, 0.0, 0.0, 1e-3, 0.9, 0.999, 1e-7, 1)
        assert H.max_err(variable(m, n), want) < 1e-6, n


def test_weight_decay_reaches_kernels_only(env):
    x, labels = batch()
    lr, wd = 1e-3, 0.1
    m, tr, w = trainer(weight_decay=wd, learning_rate=lr)
    forward_backward(tr, x, labels)
    grads = {n: tr.gradient(n) for n in (KERNEL, BIAS, GAMMA)}
    tr.apply_gradients()
    for n, gr in grads.items():
        p = w[n].astype(np.float64)
        want, _, _ = TT.adam_reference(p, gr.astype(np.float64), 0.0, 0.0, lr, 0.9, 0.999, 1e-7, 1)
        if n == KERNEL:
            want = want - p * lr * wd            # p (1 - lr wd) - lr_t m / (sqrt(v) + eps)
            assert np.abs(p * lr * wd).max() > 1e-5       # (the decay term is well above the bar)
        assert H.max_err(variable(m, n), want) < 1e-6, n


@pytest.mark.parametrize("vocab_size", [None, 31])
def test_accumulating_the_same_batch_twice_doubles_the_gradient_exactly(env, vocab_size):
    x, labels = batch()
    m0, t0, w = trainer(vocab_size)
    forward_backward(t0, x, labels)
    g = t0.grad_buffer().cpu().numpy().copy()
    m1, t1, _ = trainer(vocab_size, accumulation_steps=2)
    t1.step(x, labels)
    assert t1.iterations == 0
    got = m1.get_weights()
    for n in w:
        assert np.array_equal(got[n].view(np.uint32), w[n].view(np.uint32)), n
    t1.step(x, labels)
    assert t1.iterations == 1
    g2 = t1.grad_buffer().cpu().numpy()
    assert np.abs(g).max() > 0 and np.array_equal(g2.view(np.uint32), (2.0 * g).astype(np.float32).view(np.uint32))
    assert not np.array_equal(variable(m1, KERNEL), w[KERNEL])


def test_two_micro_batches_against_the_big_batch(env):
    """Two different (2, 4000) micro-batches with division_factor = 4 against one (4, 4000) step: each variable's gradient to
    2e-4 of its max |g| (the bar and the k_proj/bias rule of tests/test_train_gpu.py::grads_close)."""
    x = V.hash_normal("opt/wave4", 4 * L, 9).reshape(4, L)
    labels = np.array([[5, 6, 7, 0], [9, 9, 0, 0], [3, 4, 0, 0], [11, 2, 8, 1]], np.int32)
    m0, t0, w = trainer(B=4, division_factor=4)
    forward_backward(t0, x, labels)
    names = [v.local_name for v in m0.trainable_variables]
    ref = {n: t0.gradient(n) for n in names}
    m1, t1, _ = trainer(division_factor=4, accumulation_steps=2)
    t1.step(x[:2], labels[:2])
    t1.step(x[2:], labels[2:])
    worst = ("", 0.0)
    for n in names:
        if n == "masked_spec_embed":          # no spec-augment mask: unused, zero on both sides
            assert not np.any(ref[n]) and not np.any(t1.gradient(n))
            continue
        scale = max(1e-3, float(np.abs(ref[n]).max()))
        if n.endswith("k_proj/bias"):
            scale = max(scale, float(np.abs(ref[n[:-4] + "kernel"]).max()))
        e = H.max_err(t1.gradient(n), ref[n]) / scale
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e < 2e-4, f"{n}: relative gradient error {e:.3e} (max |g| = {scale:.3e})"
    print("worst:", worst)


def test_non_finite_gradient_skips_the_step(env):
    _, torch, _ = env
    x, labels = batch()
    m, tr, _ = trainer(skip_nonfinite=True)
    tr.step(x, labels)                             # (moments are no longer zero: "unchanged" means something)
    assert tr.skipped_steps == 0
    before = snapshot(m, tr)
    forward_backward(tr, x, labels)
    off, n = tr.gradient_slot(KERNEL)
    tr.grad_buffer()[off + n // 2] = float("nan")
    tr.apply_gradients()
    assert same_bits(before, snapshot(m, tr))
    assert tr.skipped_steps == 1 and tr.iterations == 2
    tr.step(x, labels)
    after = snapshot(m, tr)
    assert not np.array_equal(after[0][KERNEL], before[0][KERNEL]) and np.isfinite(after[0][KERNEL]).all()
    assert tr.skipped_steps == 1


def test_clipped_decayed_accumulated_steps_are_bitwise_reproducible(env):
    x, labels = batch()

    def run():
        m, tr, _ = trainer(max_grad_norm=1e-3, weight_decay=0.01, accumulation_steps=2, dropout=0.1, seed=3)
        for _ in range(4):
            tr.step(x, labels)
        assert tr.iterations == 2 and tr.last_clip_scale < 1.0
        return snapshot(m, tr)

    assert same_bits(run(), run())


def test_checkpoint_state(env):
    x, labels = batch()
    m, tr, _ = trainer(accumulation_steps=2, skip_nonfinite=True)
    tr.step(x, labels)
    with pytest.raises(RuntimeError, match="accumulation"):
        tr.state_dict()
    tr.step(x, labels)
    assert tr.state_dict()["skipped_steps"] == 0
    # a skipped step travels with the state ...
    m1, t1, _ = trainer(skip_nonfinite=True)
    forward_backward(t1, x, labels)
    t1.grad_buffer()[t1.gradient_slot(KERNEL)[0]] = float("inf")
    t1.apply_gradients()
    state = t1.state_dict()
    assert state["skipped_steps"] == 1
    m2, t2, _ = trainer(skip_nonfinite=True)
    t2.load_state_dict(state)
    assert t2.skipped_steps == 1 and t2.iterations == 1
    # ... and a state from before the key existed loads as "none skipped"
    del state["skipped_steps"]
    t2.load_state_dict(state)
    assert t2.skipped_steps == 0
