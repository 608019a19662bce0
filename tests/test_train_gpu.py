"""Training step parity: the HIP training forward / backward / Adam against
the torch-autograd oracle (oracle/w2v2_torch_train.py, fp64 CPU) on the same seeded weights and the SAME
dropout masks (the build's counter-based hash is evaluated by both sides)."""

import ctypes as C

import numpy as np
import pytest

import helpers as H
from oracle import w2v2_oracle as O
from oracle import w2v2_torch_train as TT
from test_weight_grad_plan_cpu import plan as weight_grad_plan, problem as weight_grad_problem
from wav2vec2 import _native as N
from wav2vec2 import variables as V
from wav2vec2.spec_augment import compute_mask_indices

pytestmark = pytest.mark.gpu

_KEEP = []


@pytest.fixture(autouse=True)
def _keepalive():
    _KEEP.clear()
    yield
    _KEEP.clear()


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


def dev_t(torch, dev, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    _KEEP.append(t)
    return t


def rnd(tag, shape, scale=1.0):
    n = int(np.prod(shape))
    return ((V.hash_uniform(tag, n, 21) * 2 - 1) * scale).reshape(shape).astype(np.float32)


# ------------------------------------------------------------------ operators --------------
@pytest.mark.parametrize("n,p,stream", [(1000, 0.1, 3), (70001, 0.5, 17), (256, 0.0, 1)])
def test_dropout_hash_matches_host(env, n, p, stream):
    lib, torch, dev = env
    x = rnd("dx", (n,))
    res = rnd("dr", (n,))
    y = torch.empty((n,), device=dev)
    N.check(lib.w2v2_op_dropout(N.ptr(dev_t(torch, dev, x)), N.ptr(dev_t(torch, dev, res)), N.ptr(y), n, 0, p,
                                C.c_uint64(0xDEADBEEF12345), stream, N.current_stream()))
    keep = V.dropout_keep(0xDEADBEEF12345, stream, n, p)
    ref = np.where(keep, x / np.float32(1 - p), 0).astype(np.float32) + res
    assert np.allclose(y.cpu().numpy(), ref, atol=1e-6)
    if p > 0:
        assert abs(keep.mean() - (1 - p)) < 4.0 * np.sqrt(p * (1 - p) / n)       # four standard deviations of the sample mean


@pytest.mark.parametrize("rows,Cn,p", [(37, 768, 0.1), (3001, 1024, 0.1), (9, 64, 0.5), (130, 768, 0.0), (5000, 1280, 0.1)])
def test_layer_norm_dropout_fused_equals_the_two_kernels(env, rows, Cn, p):
    """t1 = dropout(x) + residual, y = LayerNorm(t1) in one pass (layernorm.hip::layer_norm_drop_kernel, the training forward's
    encoder.py:116-124) against (a) the two separate operators, bit for bit -- fp32 y, the bf16 copy and t1 -- and (b) the host's
    keep mask + a float64 LayerNorm."""
    lib, torch, dev = env
    x, res = rnd("ldx", (rows, Cn), 2.0), rnd("ldr", (rows, Cn))
    g, b = 1 + rnd("ldg", (Cn,), 0.3), rnd("ldb", (Cn,), 0.2)
    seed, stream = C.c_uint64(0xC0FFEE1234), 21
    xd, rd, gd, bd = (dev_t(torch, dev, a) for a in (x, res, g, b))
    t1a = torch.empty((rows, Cn), device=dev)
    N.check(lib.w2v2_op_dropout(N.ptr(xd), N.ptr(rd), N.ptr(t1a), rows * Cn, 0, p, seed, stream, N.current_stream()))
    ya = torch.empty((rows, Cn), device=dev)
    N.check(lib.w2v2_op_layer_norm(N.ptr(t1a), N.ptr(ya), N.ptr(gd), N.ptr(bd), rows, Cn, 1e-5, 0, N.current_stream()))
    t1b, yb = torch.empty((rows, Cn), device=dev), torch.empty((rows, Cn), device=dev)
    y16 = torch.empty((rows, Cn), device=dev, dtype=torch.bfloat16)
    N.check(lib.w2v2_op_layer_norm_dropout(N.ptr(xd), N.ptr(rd), N.ptr(t1b), N.ptr(yb), N.ptr(y16), N.ptr(gd), N.ptr(bd), rows, Cn, 1e-5, p,
                                           seed, stream, N.current_stream()))
    assert torch.equal(t1a, t1b) and torch.equal(ya, yb)
    assert torch.equal(y16, yb.to(torch.bfloat16))                       # nearest-even, as torch rounds
    keep = V.dropout_keep(0xC0FFEE1234, stream, rows * Cn, p).reshape(rows, Cn)
    t1 = np.where(keep, x.astype(np.float64) / (1 - np.float64(np.float32(p))), 0) + res
    mu, var = t1.mean(-1, keepdims=True), t1.var(-1, keepdims=True)
    ref = (t1 - mu) / np.sqrt(var + 1e-5) * g + b
    assert H.max_err(t1b.cpu().numpy(), t1) < 2e-6 * max(1.0, np.abs(t1).max())
    assert H.max_err(yb.cpu().numpy(), ref) < 2e-5


@pytest.mark.parametrize("rows,Cn", [(37, 512), (130, 768), (9, 64), (5, 50), (3000, 768)])
def test_layer_norm_backward(env, rows, Cn):
    lib, torch, dev = env
    x, dy = rnd("lx", (rows, Cn), 2.0) + 0.5, rnd("ldy", (rows, Cn))
    g = 1 + rnd("lg", (Cn,), 0.3)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    gt = torch.from_numpy(g.astype(np.float64)).requires_grad_(True)
    bt = torch.zeros(Cn, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(xt, (Cn,), gt, bt, 1e-5)
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    dx = torch.empty((rows, Cn), device=dev)
    dg = torch.empty((Cn,), device=dev)
    db = torch.empty((Cn,), device=dev)
    ws = torch.empty((int(lib.w2v2_ln_bwd_ws_floats(rows, Cn)),), device=dev)
    N.check(lib.w2v2_op_layer_norm_bwd(N.ptr(dev_t(torch, dev, x)), N.ptr(dev_t(torch, dev, g)), N.ptr(dev_t(torch, dev, dy)),
                                       N.ptr(dx), N.ptr(dg), N.ptr(db), rows, Cn, 1e-5, N.ptr(ws), N.current_stream()))
    assert H.max_err(dx.cpu().numpy(), xt.grad.numpy()) < 2e-5
    assert H.max_err(dg.cpu().numpy(), gt.grad.numpy()) < 2e-4 * max(1.0, rows / 100)
    assert H.max_err(db.cpu().numpy(), bt.grad.numpy()) < 2e-4 * max(1.0, rows / 100)


@pytest.mark.parametrize("B,T,Hh,heads,p,flen", [(2, 12, 64, 2, 0.0, None), (2, 150, 128, 2, 0.1, None),
                                                  (1, 200, 768, 12, 0.1, None), (2, 97, 128, 2, 0.2, [97, 40])])
def test_attention_train_forward_backward(env, B, T, Hh, heads, p, flen):
    """softmax-dropout attention and its gradient w.r.t. the packed q|k|v vs torch autograd."""
    lib, torch, dev = env
    d = Hh // heads
    seed, stream = 991, 16
    qkv = rnd("aq", (B, T, 3 * Hh), 1.5)
    dctx = rnd("ad", (B, T, Hh))
    qt = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    q, k, v = [qt[:, :, i * Hh:(i + 1) * Hh].reshape(B, T, heads, d).transpose(1, 2) for i in range(3)]
    s = (q * d ** -0.5) @ k.transpose(-1, -2)
    if flen is not None:
        keepk = torch.from_numpy(np.arange(T)[None, :] < np.asarray(flen)[:, None])
        s = s + ((~keepk).double() * -10000.0)[:, None, None, :]
    pr = torch.softmax(s, -1)
    lse_ref = torch.logsumexp(s, -1).detach().numpy()
    if p > 0:
        keep = torch.from_numpy(np.ascontiguousarray(V.attention_keep(seed, stream, B * heads * T, T, p)).reshape(B, heads, T, T))
        pr = torch.where(keep, pr / (1 - p), torch.zeros_like(pr))
    ctx_ref = (pr @ v).transpose(1, 2).reshape(B, T, Hh)
    ctx_ref.backward(torch.from_numpy(dctx.astype(np.float64)))

    tq = dev_t(torch, dev, qkv)
    tf = dev_t(torch, dev, np.asarray(flen, dtype=np.int32)) if flen is not None else None
    ctx = torch.full((B, T, Hh), float("nan"), device=dev)
    lse = torch.full((B, heads, T), float("nan"), device=dev)
    N.check(lib.w2v2_op_attention_train(N.ptr(tq), N.ptr(tf), N.ptr(ctx), N.ptr(lse), B, T, Hh, heads, p,
                                        C.c_uint64(seed), stream, N.current_stream()))
    assert H.max_err(ctx.cpu().numpy(), ctx_ref.detach().numpy()) < 3e-5
    assert H.max_err(lse.cpu().numpy(), lse_ref) < 3e-5
    dqkv = torch.full((B, T, 3 * Hh), float("nan"), device=dev)
    ws = torch.empty((B, heads, T), device=dev)
    N.check(lib.w2v2_op_attention_bwd(N.ptr(tq), N.ptr(tf), N.ptr(ctx), N.ptr(lse), N.ptr(dev_t(torch, dev, dctx)), N.ptr(dqkv),
                                      N.ptr(ws), B, T, Hh, heads, p, C.c_uint64(seed), stream, N.current_stream()))
    got, ref = dqkv.cpu().numpy(), qt.grad.numpy()
    assert np.isfinite(got).all()
    for name, sl in (("dq", slice(0, Hh)), ("dk", slice(Hh, 2 * Hh)), ("dv", slice(2 * Hh, 3 * Hh))):
        e = H.max_err(got[:, :, sl], ref[:, :, sl])
        assert e < 5e-5 * max(1.0, np.abs(ref[:, :, sl]).max()), f"{name}: {e:.3e}"


@pytest.mark.parametrize("B,T,Hh,heads,p,flen", [(2, 150, 128, 2, 0.1, None), (1, 200, 768, 12, 0.1, None),
                                                  (2, 97, 128, 2, 0.2, [97, 40]), (1, 64, 64, 1, 0.0, None)])
def test_attention_train_forward_backward_bf16(env, B, T, Hh, heads, p, flen):
    """bf16 matrix-pipe attention, training forward + backward (head size 64): torch autograd in fp64 on
    bf16-rounded q d^-0.5, k, v.  Unrounded in the reference: P, dO, dS -- their 2^-9 relative roundings average
    out over the contraction, so the bar is 1e-2 of the gradient's magnitude (a layout error shows at O(1))."""
    lib, torch, dev = env
    d = Hh // heads
    assert d == 64
    seed, stream = 991, 16
    qkv = rnd("aq16", (B, T, 3 * Hh), 1.5)
    dctx = rnd("ad16", (B, T, Hh))
    qkv_r = qkv.copy()
    qkv_r[:, :, :Hh] = O.round_bf16(qkv[:, :, :Hh] * np.float32(0.125)) * 8.0     # scale is a power of two
    qkv_r[:, :, Hh:] = O.round_bf16(qkv[:, :, Hh:])
    qt = torch.from_numpy(qkv_r.astype(np.float64)).requires_grad_(True)
    q, k, v = [qt[:, :, i * Hh:(i + 1) * Hh].reshape(B, T, heads, d).transpose(1, 2) for i in range(3)]
    s = (q * d ** -0.5) @ k.transpose(-1, -2)
    if flen is not None:
        keepk = torch.from_numpy(np.arange(T)[None, :] < np.asarray(flen)[:, None])
        s = s + ((~keepk).double() * -10000.0)[:, None, None, :]
    pr = torch.softmax(s, -1)
    lse_ref = torch.logsumexp(s, -1).detach().numpy()
    if p > 0:
        keep = torch.from_numpy(np.ascontiguousarray(V.attention_keep(seed, stream, B * heads * T, T, p)).reshape(B, heads, T, T))
        pr = torch.where(keep, pr / (1 - p), torch.zeros_like(pr))
    ctx_ref = (pr @ v).transpose(1, 2).reshape(B, T, Hh)
    ctx_ref.backward(torch.from_numpy(dctx.astype(np.float64)))

    N.check(lib.w2v2_op_set_precision(1))
    try:
        tq = dev_t(torch, dev, qkv)
        tf = dev_t(torch, dev, np.asarray(flen, dtype=np.int32)) if flen is not None else None
        ctx = torch.full((B, T, Hh), float("nan"), device=dev)
        lse = torch.full((B, heads, T), float("nan"), device=dev)
        N.check(lib.w2v2_op_attention_train(N.ptr(tq), N.ptr(tf), N.ptr(ctx), N.ptr(lse), B, T, Hh, heads, p,
                                            C.c_uint64(seed), stream, N.current_stream()))
        dqkv = torch.full((B, T, 3 * Hh), float("nan"), device=dev)
        ws = torch.empty((B, heads, T), device=dev)
        N.check(lib.w2v2_op_attention_bwd(N.ptr(tq), N.ptr(tf), N.ptr(ctx), N.ptr(lse), N.ptr(dev_t(torch, dev, dctx)), N.ptr(dqkv),
                                          N.ptr(ws), B, T, Hh, heads, p, C.c_uint64(seed), stream, N.current_stream()))
        torch.cuda.synchronize()
    finally:
        N.check(lib.w2v2_op_set_precision(0))
    e_ctx = H.max_err(ctx.cpu().numpy(), ctx_ref.detach().numpy())
    e_lse = H.max_err(-lse.cpu().numpy() * np.log(2.0), lse_ref)       # (the bf16 kernels save -log2-sum-exp2: include/w2v2.h)
    print(f"bf16 attention train: ctx err {e_ctx:.3e}, lse err {e_lse:.3e}")
    assert e_ctx < 1e-2 and e_lse < 1e-4          # scores are fp32 sums of exact products: lse is tight
    got, ref = dqkv.cpu().numpy(), qt.grad.numpy()
    assert np.isfinite(got).all()
    for name, sl in (("dq", slice(0, Hh)), ("dk", slice(Hh, 2 * Hh)), ("dv", slice(2 * Hh, 3 * Hh))):
        err = np.abs(got[:, :, sl] - ref[:, :, sl])
        scale = max(1.0, np.abs(ref[:, :, sl]).max())
        print(f"   {name}: max err {err.max():.3e}, mean err {err.mean():.3e}, max|ref| {scale:.3f}")
        assert err.max() < 1e-2 * scale and err.mean() < 1e-3 * scale, f"{name}: {err.max():.3e}"


@pytest.mark.parametrize("precision", [0, 1])
def test_attention_train_is_bitwise_reproducible(env, precision):
    """The same launch 25 times gives the same bits (forward ctx / lse, backward dqkv).  Regression guard: a first version of
    the paired dropout decisions (32 lane masks alive at once in the bf16 forward) produced run-to-run differences on gfx950."""
    lib, torch, dev = env
    B, T, Hh, heads, p, seed, stream = 2, 150, 128, 2, 0.5, 7, V.layer_stream(1, 0)
    tq = dev_t(torch, dev, rnd("attn/repro", (B, T, 3 * Hh)))
    td = dev_t(torch, dev, rnd("attn/repro_d", (B, T, Hh)))
    N.check(lib.w2v2_op_set_precision(precision))
    try:
        first = None
        for it in range(25):
            ctx = torch.zeros((B, T, Hh), device=dev)
            lse = torch.zeros((B, heads, T), device=dev)
            dqkv = torch.zeros((B, T, 3 * Hh), device=dev)
            ws = torch.empty((B, heads, T), device=dev)
            N.check(lib.w2v2_op_attention_train(N.ptr(tq), None, N.ptr(ctx), N.ptr(lse), B, T, Hh, heads, p, C.c_uint64(seed), stream,
                                                N.current_stream()))
            N.check(lib.w2v2_op_attention_bwd(N.ptr(tq), None, N.ptr(ctx), N.ptr(lse), N.ptr(td), N.ptr(dqkv), N.ptr(ws), B, T, Hh, heads, p,
                                              C.c_uint64(seed), stream, N.current_stream()))
            torch.cuda.synchronize()
            got = (ctx.cpu().numpy(), lse.cpu().numpy(), dqkv.cpu().numpy())
            if first is None:
                first = got
            else:
                for a, b, name in zip(got, first, ("ctx", "lse", "dqkv")):
                    assert np.array_equal(a, b), f"run {it}: {name} differs in {int((a != b).sum())} elements"
    finally:
        N.check(lib.w2v2_op_set_precision(0))


# ------------------------------------------------------------------ whole step ---------------
def build(name, L):
    import wav2vec2
    cfg = H.case_config(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(2, L))
    w = H.case_weights(name)
    m.set_weights(w)
    m.freeze_feature_extractor()
    return m, cfg, w


def grads_close(trainer, ref_grads, rtol=2e-4):
    worst = ("", 0.0)
    for name, g in ref_grads.items():
        got = trainer.gradient(name)
        if g is None:                      # variable unused in this forward (e.g. masked_spec_embed without a mask)
            assert not np.any(got), name
            continue
        scale = max(1e-3, float(np.abs(g).max()))
        if name.endswith("k_proj/bias"):
            # exactly zero in exact arithmetic (softmax ignores a per-query constant shift of the scores): what is
            # left is rounding noise, so measure it against the k_proj kernel gradient it is the column sum of
            scale = max(scale, float(np.abs(ref_grads[name[:-4] + "kernel"]).max()))
        e = H.max_err(got, g) / scale
        if e > worst[1]:
            worst = (name, e)
        assert e < rtol, f"{name}: relative gradient error {e:.3e} (max |g| = {scale:.3e})"
    return worst


def test_training_forward_without_randomness_equals_inference(env):
    import wav2vec2
    g = H.golden("tiny_base")
    m, cfg, w = build("tiny_base", 4000)
    tr = wav2vec2.Trainer(m, wav2vec2.CTCLoss(cfg, g["wave"].shape), dropout=0.0, apply_spec_augment=False)
    a = tr.forward(g["wave"]).cpu().numpy()
    b = m(g["wave"]).numpy()
    assert np.allclose(a, b, atol=2e-6)


@pytest.mark.parametrize("case,precision", [("tiny_base", "fp32"), ("tiny_base", "bf16"), ("tiny_robust", "bf16"), ("tiny_robust", "fp32")])
def test_backward_overwrites_every_trainable_gradient(env, case, precision):
    """The backward no longer zero-fills the whole gradient buffer (round 6: 0.23 / 0.8 ms of runtime fill kernels per step): every
    producer stores its gradient, and only the slots nothing writes are cleared (csrc/w2v2_train.hip, at the top of the backward).
    Pinned here by poisoning the buffer with NaN between two backward passes of the same step: the second must reproduce the first
    bit for bit in every trainable variable -- with and without a spec-augment mask (masked_spec_embed is written only with one),
    with a layer dropped by stochastic depth (that step and the one after take the full clear), and across a change of the
    trainable set (stage 1 <-> stage 2 of the reference, main.py:210,234-237)."""
    import torch
    import wav2vec2
    g = H.golden(case)
    m, cfg, w = build(case, 4000)
    m.freeze_feature_extractor()
    m.set_precision(precision)
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=3)
    mask = g.get("attention_mask")
    mask = None if mask is None else mask.astype(np.int32)
    T = cfg.num_frames(g["wave"].shape[1])
    spec = compute_mask_indices((2, T), 0.3, 2, rng=np.random.RandomState(1))
    names = [n for n in V.variable_specs(cfg) if "feature_extractor" not in n]
    labels = np.array([[5, 9, 9, 11, 0, 0], [7, 6, 0, 0, 0, 0]], np.int32)

    def grads():
        torch.cuda.synchronize()
        return {n: tr.gradient(n).copy() for n in names}

    def check(tag, only=None, **fw):
        logits = tr.forward(g["wave"], mask, step_seed=11, **fw)
        _, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(dlog)
        first = grads()
        tr.grad_buffer().fill_(float("nan"))
        tr.backward(dlog)
        second = grads()
        for n in (only or names):
            assert np.isfinite(second[n]).all(), f"{tag}: {n} was not written by the backward"
            assert np.array_equal(first[n], second[n]), f"{tag}: {n}"
        return first

    try:
        a = check("spec mask", spec_mask=spec)
        assert np.any(a["masked_spec_embed"])
        b = check("no spec mask")
        assert not np.any(b["masked_spec_embed"])                     # cleared, not left over from the step before
        sd = np.ones(cfg.num_layers, np.float32)
        sd[-1] = 0.0
        c = check("dropped layer", sd_keep=sd)
        last = f"encoder/layers/{cfg.num_layers - 1}/feed_forward/intermediate_dense/kernel"
        assert not np.any(c[last]) and np.any(b[last])
        d = check("after a dropped layer")
        assert np.any(d[last])
        m.layers[0].trainable = False                                 # stage 1: only lm_head trains
        tr._ranges_cache = {}
        e = check("stage 1", only=["lm_head/kernel", "lm_head/bias"])
        assert np.any(e["lm_head/kernel"]) and not np.any(e[last])    # the frozen variables' slots read zero, not the last stage-2 gradient
    finally:
        m.set_precision("fp32")


@pytest.mark.parametrize("p,use_spec,use_sd", [(0.0, False, False), (0.1, True, True)])
def test_gradients_match_autograd_tiny(env, p, use_spec, use_sd):
    import wav2vec2
    g = H.golden("tiny_base")
    m, cfg, w = build("tiny_base", 4000)
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=p, apply_spec_augment=False, seed=3)
    spec = compute_mask_indices((2, 12), 0.3, 2, rng=np.random.RandomState(1)) if use_spec else None
    sd = np.array([1.0, 0.0], np.float32) if use_sd else None
    logits = tr.forward(g["wave"], spec_mask=spec, sd_keep=sd, step_seed=777)
    nll, dlog = loss_fn.per_sample(g["labels"], logits, with_grad=True)
    tr.backward(dlog)
    loss, ref_nll, ref_logits, ref_grads = TT.loss_and_grads(cfg, w, g["wave"], g["labels"], p=p, seed=777, spec_mask=spec,
                                                             sd_keep=sd, division_factor=2)
    assert H.max_err(logits.cpu().numpy(), ref_logits) < 2e-5
    assert np.allclose(nll.cpu().numpy(), ref_nll, atol=1e-3)
    assert len(ref_grads) == len(V.variable_specs(cfg)) - 9
    worst = grads_close(tr, ref_grads)
    print("worst relative gradient error", worst)
    # frozen conv stack: gradient slots stay zero
    assert not np.any(tr.gradient("feature_extractor/conv_layers/3/conv/kernel"))


def test_gradients_match_autograd_prenorm_with_mask(env):
    """Robust / xlsr flavour: prenorm transformer, LayerNorm conv stack with bias, attention mask
    (padded frames zeroed before the positional conv, key-padding mask in attention)."""
    import wav2vec2
    g = H.golden("tiny_robust")
    m, cfg, w = build("tiny_robust", 4000)
    mask = g["attention_mask"].astype(np.int32)
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=3)
    spec = compute_mask_indices((2, 12), 0.3, 2, rng=np.random.RandomState(2))
    labels = np.array([[3, 4, 0], [5, 0, 0]], np.int32)
    logits = tr.forward(g["wave"], attention_mask=mask, spec_mask=spec, step_seed=99)
    nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)
    loss, ref_nll, ref_logits, ref_grads = TT.loss_and_grads(cfg, w, g["wave"], labels, attention_mask=mask, p=0.1, seed=99,
                                                             spec_mask=spec, division_factor=2)
    assert H.max_err(logits.cpu().numpy(), ref_logits) < 2e-5
    assert np.allclose(nll.cpu().numpy(), ref_nll, atol=1e-3)
    worst = grads_close(tr, ref_grads)
    print("worst relative gradient error (prenorm + mask)", worst)


def test_gradients_match_autograd_base_dims(env):
    """Real base dimensions (768 / 12 heads / 3072 / 16 x 48-channel groups / 128 taps) on a short input."""
    import wav2vec2
    L = 12000
    m, cfg, w = build("base_sample_padded", L)
    x = V.hash_normal("train/wave", 2 * L, 8).reshape(2, L)
    labels = np.array([[5, 9, 9, 11, 0, 0], [7, 6, 0, 0, 0, 0]], np.int32)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    T = cfg.num_frames(L)
    spec = compute_mask_indices((2, T), 0.05, 10, rng=np.random.RandomState(4))
    logits = tr.forward(x, spec_mask=spec, step_seed=42)
    nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)
    loss, ref_nll, ref_logits, ref_grads = TT.loss_and_grads(cfg, w, x, labels, p=0.1, seed=42, spec_mask=spec, division_factor=2)
    assert H.max_err(logits.cpu().numpy(), ref_logits) < 1e-4
    worst = grads_close(tr, ref_grads, rtol=5e-4)
    print("worst relative gradient error (base dims)", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case,L,B", [("base_sample_padded", 61520, 2), ("tiny_robust", 4000, 2)])
def test_weight_gradient_side_stream_is_bit_identical(env, case, L, B):
    """Model option "wgrad_stream" (W2V2_OPT_WGRAD_STREAM): the encoder layers' weight-gradient GEMMs on the model's second HIP stream,
    ordered by events.  Same kernels on the same operands: the WHOLE flat gradient buffer is bit-identical to the one-stream backward,
    five backward passes in a row (a missing wait would let the main stream overwrite a dY a weight gradient is still reading), for the
    postnorm (base) and the prenorm (robust) layer loop."""
    import wav2vec2
    _, torch, dev = env
    labels = np.tile(np.array([[5, 9, 9, 11, 0, 0]], np.int32), (B, 1))
    x = V.hash_normal("train/wave_side", B * L, 8).reshape(B, L)
    m, cfg, w = build(case, L)
    m.set_precision("bf16")
    assert m.get_option("wgrad_stream") is False            # (measured neutral on one GPU: off by default)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=B)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    ref = None
    for flag, reps in ((False, 1), (True, 5), (False, 1)):
        m.set_option("wgrad_stream", flag)
        for _ in range(reps):
            logits = tr.forward(x, step_seed=7)
            nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
            tr.backward(dlog)
            g = tr.grad_buffer().clone()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(g).all())
            if ref is None:
                ref = g
                assert float(ref.abs().max()) > 0
            else:
                assert torch.equal(g, ref), (flag, int((g != ref).sum()))
    m.set_option("wgrad_stream", False)


@pytest.mark.gpu
def test_bf16_step_keeps_the_bf16_only_activation_path_after_an_optimizer_step(env):
    """The bf16 fine-tune step keeps q|k|v, the attention output, the FFN hidden activation and its pre-activation only as bf16 and does
    not even allocate their fp32 buffers (w2v2_train_storage).  That decision reads the bf16 weight shadows' validity, which every
    optimizer step resets -- so it must be taken AFTER the forward has refreshed them: a step that silently fell back to the fp32
    activations is numerically fine and twice as slow in the element-wise kernels (this happened once: caught by the bench, not by a test).
    Also: the workspace really shrinks, and a precision switch on the same shapes rebuilds it."""
    import wav2vec2
    _, torch, dev = env
    B, L = 2, 61520
    m, cfg, w = build("base_sample_padded", L)
    x = V.hash_normal("train/wave_lean", B * L, 8).reshape(B, L)
    labels = np.tile(np.array([[5, 9, 9, 11, 0, 0]], np.int32), (B, 1))
    m.set_precision("bf16")
    m.freeze_feature_extractor()
    tr = wav2vec2.Trainer(m, wav2vec2.CTCLoss(cfg, x.shape, division_factor=B), dropout=0.1, seed=1)
    for _ in range(3):                       # the 2nd and 3rd forward follow an optimizer step
        assert np.isfinite(float(tr.step(x, labels)))
        names, lean_bytes = tr.activation_storage()
        assert names == {"qkv", "ctx", "ffn", "u"}, names
    m.set_precision("fp32")
    assert np.isfinite(float(tr.step(x, labels)))
    names, full_bytes = tr.activation_storage()
    assert names == set(), names
    T, H, F, N = cfg.num_frames(L), cfg.hidden_size, cfg.intermediate_size, cfg.num_layers
    saved = N * B * T * (3 * H + H + F + F // 2) * 4          # q|k|v, ctx, gd and half of u per layer, fp32
    # (the bf16 step also owns ~40 MB of positional-conv kernel-gradient scratch the fp32 step does not allocate: hence 0.6, not 1.0)
    assert full_bytes - lean_bytes >= 0.6 * saved, (full_bytes, lean_bytes, saved)
    m.set_precision("bf16")
    assert np.isfinite(float(tr.step(x, labels)))
    assert tr.activation_storage()[0] == {"qkv", "ctx", "ffn", "u"}
    m.set_precision("fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("case,L,B", [("base_sample_padded", 61520, 2), ("tiny_robust", 4000, 2), ("base_sample_padded", 24080, 3)])
def test_deferred_folds_do_not_change_results(env, case, L, B, precision):
    """Model option "defer_folds" (W2V2_OPT_DEFER_FOLDS, default on): the nine small reductions that finish an encoder layer's gradients
    (split-K slab sums of the four weight gradients with the q|k|v unpack, LayerNorm / dropout / attention column-sum folds) run as ONE
    launch over a job table in front of the layer's bucket event.  Each job keeps the summation order of the kernel it replaces, so the
    WHOLE flat gradient buffer must be bit-identical to the one-launch-per-producer backward -- postnorm (base) and prenorm (robust)
    loops, whole and ragged row counts (B T = 3 x 75 = 225), both precisions, three passes in a row (a partial buffer recycled before
    its fold ran would show up as a changed gradient), and with a stochastic-depth drop of one layer (fewer jobs in that layer's table)."""
    import wav2vec2
    _, torch, dev = env
    labels = np.tile(np.array([[5, 9, 9, 11, 0, 0]], np.int32), (B, 1))
    x = V.hash_normal("train/wave_fold", B * L, 8).reshape(B, L)
    m, cfg, w = build(case, L)
    m.set_precision(precision)
    assert m.get_option("defer_folds") is True
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=B)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    for sd_keep in (None, [1.0] + [0.0] + [1.0] * (cfg.num_layers - 2)):
        ref = None
        for flag, reps in ((False, 1), (True, 3), (False, 1)):
            m.set_option("defer_folds", flag)
            for _ in range(reps):
                logits = tr.forward(x, step_seed=7, sd_keep=sd_keep)
                nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
                tr.backward(dlog)
                g = tr.grad_buffer().clone()
                torch.cuda.synchronize()
                assert bool(torch.isfinite(g).all())
                if ref is None:
                    ref = g
                    assert float(ref.abs().max()) > 0
                else:
                    assert torch.equal(g, ref), (flag, sd_keep is not None, int((g != ref).sum()))
    m.set_option("defer_folds", True)
    m.set_precision("fp32")


@pytest.mark.parametrize("L,frames", [(20560, 64), (24080, 75)])
def test_bf16_precision_training_step(env, L, frames):
    """bf16 fine-tune arithmetic (BASELINE configs 3 / 5): training-mode logits equal the torch oracle with
    bf16-rounded Dense operands; gradients agree at a bf16-sized tolerance (the build also rounds dY inside its
    backward GEMMs, autograd's straight-through rounding does not).
    T = 64: B T = 128 rows, the weight-gradient GEMMs take the split-K, transposed-A path with two 64-row slabs.
    T = 75: B T = 150 = 2 x 64 + 22: the same plus the leftover-row slab (what T = 1499 at 480000 samples needs)."""
    import wav2vec2
    m, cfg, w = build("base_sample_padded", L)
    assert cfg.num_frames(L) == frames
    m.set_precision("bf16")
    x = V.hash_normal("train/wave16", 2 * L, 8).reshape(2, L)
    labels = np.array([[5, 9, 9, 11, 0, 0], [7, 6, 0, 0, 0, 0]], np.int32)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    T = cfg.num_frames(L)
    spec = compute_mask_indices((2, T), 0.05, 10, rng=np.random.RandomState(4))
    logits = tr.forward(x, spec_mask=spec, step_seed=42)
    nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)
    with H.oracle_operands("bf16"):
        loss, ref_nll, ref_logits, ref_grads = TT.loss_and_grads(cfg, w, x, labels, p=0.1, seed=42, spec_mask=spec, division_factor=2)
    err = H.max_err(logits.cpu().numpy(), ref_logits)
    print("bf16 training logits vs rounded-operand oracle", err)
    assert err < 0.06                      # bf16-sized bar: half of what HF's own torch.autocast(bf16) costs the tiny fixture (0.12, tests/golden/hf_bf16_autocast.json); measured 0.038-0.040
    assert np.allclose(nll.cpu().numpy(), ref_nll, rtol=2e-2)
    worst = grads_close(tr, ref_grads, rtol=5e-2)          # measured 2.6e-2 / 3.4e-2 of max|g|
    print("worst relative gradient error (bf16 operands)", worst)
    fp32_loss, _, _, fp32_grads = TT.loss_and_grads(cfg, w, x, labels, p=0.1, seed=42, spec_mask=spec, division_factor=2)
    assert abs(loss - fp32_loss) / abs(fp32_loss) < 2e-2


def test_bf16_training_shadows_do_not_change_results(env):
    """The bf16 shadows of the training forward (LayerNorm / dropout / GEMM / attention producers, (N, K) weight
    shadows) carry exactly the values the GEMMs would round to: logits and every gradient are bit-identical with
    the model option "bf16_shadows" off."""
    import wav2vec2
    L = 20560
    labels = np.array([[5, 9, 9, 11, 0, 0], [7, 6, 0, 0, 0, 0]], np.int32)
    x = V.hash_normal("train/wave16s", 2 * L, 8).reshape(2, L)
    res = {}
    for flag in ("0", "1"):
        m, cfg, w = build("base_sample_padded", L)
        m.set_precision("bf16")
        m.set_option("bf16_shadows", flag == "1")
        loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=2)
        tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
        logits = tr.forward(x, step_seed=7)
        nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(dlog)
        res[flag] = dict(logits=logits.cpu().numpy(),
                         grads={n: tr.gradient(n) for n in ("lm_head/kernel", "encoder/layers/11/feed_forward/output_dense/kernel",
                                                            "encoder/layers/0/attention/q_proj/kernel",
                                                            "feature_projection/projection/kernel", "encoder/layer_norm/gamma")},
                         biases={n: tr.gradient(n) for n in ("encoder/layers/11/feed_forward/output_dense/bias",
                                                             "encoder/layers/3/feed_forward/intermediate_dense/bias",
                                                             "encoder/layers/0/attention/q_proj/bias",
                                                             "encoder/layers/5/attention/out_proj/bias")})
    assert np.array_equal(res["0"]["logits"], res["1"]["logits"])
    for n, g in res["0"]["grads"].items():
        assert np.array_equal(g, res["1"]["grads"][n]), n
    # bias gradients are column sums taken by different kernels in the two modes (fused into the fp32 weight-gradient GEMM vs left by
    # the producers of dY): equal up to fp32 summation order
    for n, g in res["0"]["biases"].items():
        g1 = res["1"]["biases"][n]
        assert np.abs(g - g1).max() <= 2e-5 * max(np.abs(g).max(), 1e-6), (n, float(np.abs(g - g1).max()), float(np.abs(g).max()))


def test_backward_refuses_a_precision_change_since_the_forward(env):
    """The saved activations are in the forms, and the attention's saved lse in the domain (log2 for the bf16 kernels, natural for
    fp32), of the mode the forward ran in.  A backward after set_precision or a toggled "bf16_shadows" would read them wrongly, so
    it is refused with both settings named; with the setting restored, a fresh forward + backward gives the gradient buffer of a
    model that was never toggled, bit for bit."""
    import wav2vec2
    _, torch, dev = env
    B, L = 2, 4000
    x = V.hash_normal("train/wave_plan", B * L, 8).reshape(B, L)

    def step(m, tr):
        logits = tr.forward(x, step_seed=7)
        tr.backward(torch.sin(logits))
        g = tr.grad_buffer().clone()
        torch.cuda.synchronize()
        return g

    def trainer():
        m, cfg, w = build("tiny_base", L)
        return m, wav2vec2.Trainer(m, None, dropout=0.1, apply_spec_augment=False, seed=1)

    ref = {}
    for precision in ("fp32", "bf16"):
        m, tr = trainer()
        m.set_precision(precision)
        ref[precision] = step(m, tr)
        assert float(ref[precision].abs().max()) > 0
    m, tr = trainer()
    for first, then in (("fp32", "bf16"), ("bf16", "fp32")):
        m.set_precision(first)
        logits = tr.forward(x, step_seed=7)
        m.set_precision(then)
        with pytest.raises(RuntimeError) as err:
            tr.backward(torch.sin(logits))
        assert f"precision {first}" in str(err.value) and f"precision {then}" in str(err.value), str(err.value)
        m.set_precision(first)
        assert torch.equal(step(m, tr), ref[first])
    m.set_precision("bf16")
    logits = tr.forward(x, step_seed=7)
    m.set_option("bf16_shadows", False)
    with pytest.raises(RuntimeError) as err:
        tr.backward(torch.sin(logits))
    assert "bf16_shadows on" in str(err.value) and "bf16_shadows off" in str(err.value), str(err.value)
    m.set_option("bf16_shadows", True)
    assert torch.equal(step(m, tr), ref["bf16"])
    m.set_precision("fp32")


def test_stage1_only_lm_head_trains(env):
    import wav2vec2
    g = H.golden("tiny_base")
    m, cfg, w = build("tiny_base", 4000)
    m.set_trainable("", False)
    m.set_trainable("lm_head/", True)              # main.py:210: model.layers[0].trainable = False
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.0, apply_spec_augment=False)
    logits = tr.forward(g["wave"], step_seed=1)
    _, dlog = loss_fn.per_sample(g["labels"], logits, with_grad=True)
    tr.backward(dlog)
    _, _, _, ref = TT.loss_and_grads(cfg, w, g["wave"], g["labels"], trainable=lambda k: k.startswith("lm_head/"))
    assert set(ref) == {"lm_head/kernel", "lm_head/bias"}
    grads_close(tr, ref)
    assert not np.any(tr.gradient("encoder/layers/0/attention/q_proj/kernel"))


def test_adam_step_and_loss_decreases(env):
    import wav2vec2
    g = H.golden("tiny_base")
    m, cfg, w = build("tiny_base", 4000)
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, learning_rate=1e-3, dropout=0.0, apply_spec_augment=False)
    # one step: parameters move exactly as Keras Adam moves them
    logits = tr.forward(g["wave"], step_seed=1)
    _, dlog = loss_fn.per_sample(g["labels"], logits, with_grad=True)
    tr.backward(dlog)
    name = "encoder/layers/1/feed_forward/output_dense/kernel"
    gr = tr.gradient(name)
    tr.apply_gradients()
    want, _, _ = TT.adam_reference(w[name].astype(np.float64), gr.astype(np.float64), 0.0, 0.0, 1e-3, 0.9, 0.999, 1e-7, 1)
    got = [v for v in m.variables if v.local_name == name][0].numpy()
    assert H.max_err(got, want) < 1e-6
    frozen = "feature_extractor/conv_layers/2/conv/kernel"
    assert np.array_equal([v for v in m.variables if v.local_name == frozen][0].numpy(), w[frozen])
    # a few more steps on the same batch: the loss must go down
    losses = [float(tr.step(g["wave"], g["labels"])) for _ in range(8)]
    assert losses[-1] < losses[0] * 0.9, losses
    # and the inference path sees the updated weights (packed q|k|v / positional kernel re-derived)
    assert np.isfinite(m(g["wave"]).numpy()).all()


def test_trainer_defaults_run_with_dropout_and_spec_augment(env):
    import wav2vec2
    L = 24000
    m, cfg, w = build("base_sample_padded", L)
    x = V.hash_normal("train/wave2", 2 * L, 9).reshape(2, L)
    labels = np.array([[5, 9, 9, 11, 0, 0], [7, 6, 8, 0, 0, 0]], np.int32)
    tr = wav2vec2.Trainer(m, wav2vec2.CTCLoss(cfg, x.shape, division_factor=2), learning_rate=1e-4)
    l0 = float(tr.step(x, labels))
    l1 = float(tr.step(x, labels))
    assert np.isfinite([l0, l1]).all()
    assert tr.last["spec_mask"].shape == (2, cfg.num_frames(L)) and tr.last["spec_mask"].sum() > 0
    buf = tr.grad_buffer()
    assert buf.numel() >= 94_396_320 and bool(buf.isfinite().all())


def test_gradient_buckets_tile_the_flat_buffer_and_overlap_path_is_exact(env):
    """The data-parallel all-reduce is issued per gradient bucket on a side stream that waits for that bucket's event only
    (Trainer.all_reduce_gradients).  On one rank a SUM all-reduce is the identity, so running the bucketed path through
    RCCL (world size 1) must leave every gradient bit-identical -- which also proves the event waits: a collective that
    ran before its slice was final would copy stale values back over it."""
    import os
    import torch
    import torch.distributed as dist
    import wav2vec2
    m, cfg, w = build("tiny_base", 4000)
    g = H.golden("tiny_base")
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=3)
    logits = tr.forward(g["wave"], step_seed=5)
    _, dlog = loss_fn.per_sample(g["labels"], logits, with_grad=True)
    tr.backward(dlog)
    buckets = tr.gradient_buckets()
    total = tr.grad_buffer().numel()
    assert len(buckets) == cfg.num_layers + 2
    covered = sorted(buckets)
    assert covered[0][0] == 0 and covered[-1][0] + covered[-1][1] == total
    for (o0, n0), (o1, _) in zip(covered, covered[1:]):
        assert o0 + n0 == o1                                  # contiguous, no overlap, no gap
    lm = tr.gradient("lm_head/kernel")
    ref = tr.grad_buffer().clone()
    created = False
    if not dist.is_initialized():
        import socket
        with socket.socket() as sock:                         # a free port: no clash with another test process on the box
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
        created = True
    try:
        tr.backward(dlog)                                     # enqueue the backward again ...
        tr.all_reduce_gradients(force=True)                   # ... and the per-bucket collectives right behind it
        torch.cuda.synchronize()
        assert torch.equal(tr.grad_buffer(), ref)
        tr.overlap_all_reduce = False
        tr.backward(dlog)
        tr.all_reduce_gradients(force=True)
        torch.cuda.synchronize()
        assert torch.equal(tr.grad_buffer(), ref)
    finally:
        if created:
            dist.destroy_process_group()
    assert np.array_equal(lm, tr.gradient("lm_head/kernel"))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_weight_gradient_slabs_with_awkward_row_counts(env, precision):
    """B T = 1190 rows: 37 units of 32 (fp32) / 18 of 64 plus 38 rows (bf16).  37 is prime, so the weight-gradient GEMMs
    hand one unit to the leftover slab and split the other 36 into equal slabs; either way every row must be counted once.
    fp32 against torch autograd at the usual tolerance; the bf16 run against the fp32 run at a bf16-sized one."""
    import wav2vec2
    L = 190640
    m, cfg, w = build("tiny_base", L)
    assert cfg.num_frames(L) == 595
    x = V.hash_normal("train/wave_long", 2 * L, 8).reshape(2, L)
    labels = np.zeros((2, 40), np.int32)
    labels[0, :30] = 1 + np.arange(30) % 31
    labels[1, :17] = 3 + np.arange(17) % 20
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.0, apply_spec_augment=False, seed=3)
    m.set_precision(precision)
    logits = tr.forward(x, step_seed=5)
    nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)
    loss, ref_nll, ref_logits, ref_grads = TT.loss_and_grads(cfg, w, x, labels, p=0.0, seed=5, division_factor=2)
    if precision == "fp32":
        assert H.max_err(logits.cpu().numpy(), ref_logits) < 5e-5
        grads_close(tr, ref_grads, rtol=5e-4)
    else:
        grads_close(tr, ref_grads, rtol=8e-2)
    # Deferred folds (each site's own slab scratch) at B T = 32 x 64 + 5 = 2053 rows: one output tile, so the FFN and out-projection
    # weight gradients take S = 32 slabs plus the leftover-row slab -- 33, with the fold's scratch a 34th: the most a site ever holds.
    # Bit for bit the gradients of the run with "defer_folds" off (shared scratch).
    _, torch, dev = env
    L2, Hh, F = 400 + 320 * 2052, cfg.hidden_size, cfg.intermediate_size
    assert cfg.num_frames(L2) == 2053
    for Kin, Nout in ((F, Hh), (Hh, F), (Hh, Hh)):      # (64 x 128: no whole 128-tiles, so mode bf16 takes the fp32 operands too)
        assert weight_grad_plan(weight_grad_problem(2053, Kin, Nout, int(precision != "fp32"), A=1, dY=1, shared=33 * max(F * Hh, 3 * Hh * Hh)))["nslabs"] == 33
    x2 = V.hash_normal("train/wave_2053", L2, 8).reshape(1, L2)
    res = []
    for flag in (False, True):
        m.set_option("defer_folds", flag)
        logits = tr.forward(x2, step_seed=5)
        tr.backward(torch.sin(logits))
        res.append(tr.grad_buffer().clone())
        torch.cuda.synchronize()
    assert float(res[0].abs().max()) > 0 and bool(torch.isfinite(res[0]).all())
    assert torch.equal(res[0], res[1]), int((res[0] != res[1]).sum())


def test_bf16x3_training_matches_fp32_path(env):
    """Precision mode bf16x3 in the training step: the forward GEMMs and the data-gradient GEMMs (planes of the transposed
    weight copies) take the three-term split kernel once they have >= 128 tiles, i.e. only at real batch sizes -- too large
    for the autograd oracle.  So the reference here is the library's own fp32 path (pinned to torch autograd by the tests
    above) on the same input, masks and seed, B = 8 x 246000: logits within 1e-4, gradients within 5e-4 of max|g|."""
    import wav2vec2
    B, L = 8, 246000
    cfg = H.case_config("base_sample_padded")
    w = H.case_weights("base_sample_padded")
    x = V.hash_normal("train/wave_big", B * L, 8).reshape(B, L)
    rs = np.random.RandomState(3)
    labels = np.zeros((B, 64), np.int32)
    for b in range(B):
        n = rs.randint(20, 60)
        labels[b, :n] = rs.randint(1, 32, size=n)
    names = ("lm_head/kernel", "encoder/layers/11/feed_forward/output_dense/kernel", "encoder/layers/5/feed_forward/intermediate_dense/kernel",
             "encoder/layers/5/attention/q_proj/kernel", "encoder/layers/0/attention/out_proj/kernel",
             "encoder/layers/0/layer_norm/gamma", "encoder/pos_conv_embed/conv/weight_v", "feature_projection/projection/kernel")
    res = {}
    for prec in ("fp32", "bf16x3"):
        m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(B, L))
        m.set_weights(w)
        m.freeze_feature_extractor()
        m.set_precision(prec)
        loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=B)
        tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
        logits = tr.forward(x, step_seed=11)
        _, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(dlog)
        res[prec] = dict(logits=logits.cpu().numpy(), grads={n: tr.gradient(n) for n in names})
        del tr, m
    assert not np.array_equal(res["fp32"]["logits"], res["bf16x3"]["logits"])       # the split kernels did run
    assert H.max_err(res["fp32"]["logits"], res["bf16x3"]["logits"]) < 1e-4
    for n in names:
        a, b = res["fp32"]["grads"][n], res["bf16x3"]["grads"][n]
        assert np.abs(a).max() > 0
        assert np.abs(a - b).max() <= 5e-4 * np.abs(a).max(), (n, np.abs(a - b).max(), np.abs(a).max())


def test_trainer_checkpoint_resume_is_exact(env, tmp_path):
    """Three optimizer steps in one run == two steps, save (variables + Trainer.state_dict), load into a fresh model and
    trainer, one more step: bit-identical variables (dropout seeds follow the restored step count, spec-augment spans the
    restored host RNG, Adam its restored moments)."""
    import pickle
    import wav2vec2
    g = H.golden("tiny_base")
    x, labels = g["wave"], g["labels"]

    def fresh():
        m, cfg, w = build("tiny_base", 4000)
        tr = wav2vec2.Trainer(m, wav2vec2.CTCLoss(cfg, x.shape, division_factor=2), learning_rate=1e-3, dropout=0.1,
                              apply_spec_augment=True, seed=9)
        return m, tr

    m1, t1 = fresh()
    for _ in range(3):
        t1.step(x, labels)
    want = m1.get_weights()

    m2, t2 = fresh()
    for _ in range(2):
        t2.step(x, labels)
    m2.save_weights(str(tmp_path / "tf_model.npz"))
    with open(tmp_path / "trainer.pkl", "wb") as f:
        pickle.dump(t2.state_dict(), f)
    del m2, t2

    m3, t3 = fresh()
    m3.load_weights(str(tmp_path / "tf_model.npz"))
    with open(tmp_path / "trainer.pkl", "rb") as f:
        t3.load_state_dict(pickle.load(f), batch_shape=x.shape)
    assert t3.iterations == 2
    t3.step(x, labels)
    got = m3.get_weights()
    for n in want:
        assert np.array_equal(want[n], got[n]), n


# ------------------------------------------------------------------ external pins (HF fixtures) and full-size configs ----
@pytest.mark.parametrize("name,case", [("train_tiny_base", "tiny_base"), ("train_tiny_robust", "tiny_robust"),
                                       ("train_base_sample", "base_sample_unpadded")])
def test_loss_and_gradients_match_hf_fixture(env, name, case):
    """CTC loss and gradient slices captured from the HuggingFace-PyTorch import (fp64, conv stack frozen,
    no dropout / spec-augment) -- tests/golden/make_train_golden.py; the comparator and the 1e-3 loss bar of the
    reference's tests/test_wav2vec2.py:191-237.  `train_base_sample` is that test's own recipe: [sample.wav ; noise] at
    46797 samples, labels randint(1, 30, (2, 24))."""
    import wav2vec2
    g = H.golden(name)
    L = g["wave"].shape[1]
    m, cfg, w = build(case, L)
    mask = g["attention_mask"].astype(np.int32) if "attention_mask" in g else None
    div = float(g["division_factor"])
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape, division_factor=div)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.0, apply_spec_augment=False)
    logits = tr.forward(g["wave"], attention_mask=mask, step_seed=1)
    nll, dlog = loss_fn.per_sample(g["labels"], logits, with_grad=True)
    tr.backward(dlog)
    e_log = H.max_err(logits.cpu().numpy(), g["logits_f64"])
    e_nll = float(np.abs(nll.cpu().numpy().astype(np.float64) - g["nll"]).max())
    loss = float((nll.double() / div).sum())
    wname, worst = H.grad_slice_errors(tr.gradient, g)
    print(f"{name}: logits {e_log:.2e}, nll {e_nll:.2e}, loss {loss:.6f} vs HF {float(g['loss']):.6f}, "
          f"worst gradient slice {wname}: {worst:.2e}")
    assert e_log < H.ATOL_AIM
    assert e_nll < 1e-3 and abs(loss - float(g["loss"])) < 1e-3          # the reference's bar (absolute, fp32)
    assert worst < 5e-4
    assert not np.any(tr.gradient("feature_extractor/conv_layers/0/conv/kernel"))


def _ragged_labels(B, U, lo, hi, seed):
    rs = np.random.RandomState(seed)
    labels = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rs.randint(lo, hi)
        labels[b, :n] = rs.randint(1, 32, size=n)
    return labels


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_is_bitwise_reproducible(env, precision):
    """Forward + loss + backward of the same batch with the same seeds, five times: identical logits and an identical flat
    gradient buffer (no atomics on floats anywhere, fixed reduction orders, dropout from counters)."""
    import wav2vec2
    m, cfg, w = build("base_sample", 46797)
    m.set_precision(precision)
    x = V.hash_normal("train/repro", 2 * 46797, 8).reshape(2, 46797)
    labels = _ragged_labels(2, 64, 10, 40, 3)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    spec = compute_mask_indices((2, cfg.num_frames(46797)), 0.05, 10, rng=np.random.RandomState(4))
    first = None
    for it in range(5):
        logits = tr.forward(x, spec_mask=spec, step_seed=42)
        nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(dlog)
        got = (logits.cpu().numpy().copy(), tr.grad_buffer().cpu().numpy().copy())
        if first is None:
            first = got
        else:
            assert np.array_equal(got[0], first[0]), f"run {it}: logits differ"
            assert np.array_equal(got[1], first[1]), f"run {it}: {int((got[1] != first[1]).sum())} gradient elements differ"
    assert np.isfinite(first[1]).all() and np.abs(first[1]).max() > 0


@pytest.mark.parametrize("case,L,frames", [("base_sample_padded", 246000, 768), ("robust_masked", 480000, 1499)])
def test_bf16_fine_tune_step_at_full_length(env, case, L, frames):
    """BASELINE configs[2] / configs[4] at their real sequence lengths on a 2-row batch: base (12 L / 768) at 2 x 246000
    (T = 768) and large-robust (24 L / 1024, prenorm, LayerNorm convs, attention mask) at 2 x 480000 (T = 1499), precision
    mode bf16, dropout 0.1 + spec-augment, conv stack frozen.  Checker: the torch-autograd oracle (pinned to HF by
    tests/test_train_oracle_golden.py) with bf16-rounded Dense / Conv1D operands, one layer's T x T tensors alive at a time.
    Bars are bf16-sized and self-declared (the reference has no mixed precision), 1.5 x the measured values: logits 0.054 abs,
    NLL 0.2 %, every gradient within 3.2 % of its max|g| and 0.35 % on average.  Measured (rounds 2-3): logits 3.4e-2 / 3.6e-2, NLL
    4e-4 relative, worst gradient 1.1-2.1 % of max|g|, worst mean error 0.23 % / 0.13 % (base / large)."""
    import time
    import wav2vec2
    m, cfg, w = build(case, L)
    assert cfg.num_frames(L) == frames
    m.set_precision("bf16")
    x = V.hash_normal("train/full_" + case, 2 * L, 8).reshape(2, L)
    mask = None
    if cfg.is_robust:
        mask = np.ones((2, L), np.int32)
        mask[1, -70000:] = 0
        x = (x * mask).astype(np.float32)
    labels = _ragged_labels(2, 128, 40, 120, 5)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=2)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    spec = compute_mask_indices((2, frames), 0.05, 10, rng=np.random.RandomState(4))
    logits = tr.forward(x, attention_mask=mask, spec_mask=spec, step_seed=42)
    nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)
    # the step really ran on the bf16-only activations (prenorm: the in-layer LayerNorm outputs too), whose fp32 buffers do not exist
    assert tr.activation_storage()[0] == ({"qkv", "ctx", "ffn", "u", "ln"} if cfg.is_robust else {"qkv", "ctx", "ffn", "u"})
    t0 = time.time()
    with H.oracle_operands("bf16"):
        loss, ref_nll, ref_logits, ref_grads = TT.loss_and_grads(cfg, w, x, labels, attention_mask=mask, p=0.1, seed=42,
                                                                 spec_mask=spec, division_factor=2, checkpoint_layers=True)
    print(f"{case}: oracle took {time.time() - t0:.1f} s")
    err = H.max_err(logits.cpu().numpy(), ref_logits)
    print(f"{case}: bf16 training logits vs rounded-operand oracle {err:.3e}; nll {nll.cpu().numpy()} vs {ref_nll}")
    assert err < 0.054
    assert np.allclose(nll.cpu().numpy(), ref_nll, rtol=2e-3)
    worst, worst_mean = ("", 0.0), ("", 0.0)
    for name, gref in ref_grads.items():
        got = tr.gradient(name)
        if gref is None:
            assert not np.any(got), name
            continue
        scale = max(1e-3, float(np.abs(gref).max()))
        if name.endswith("k_proj/bias"):
            scale = max(scale, float(np.abs(ref_grads[name[:-4] + "kernel"]).max()))
        d = np.abs(got.astype(np.float64) - gref)
        if d.max() / scale > worst[1]:
            worst = (name, d.max() / scale)
        if d.mean() / scale > worst_mean[1]:
            worst_mean = (name, d.mean() / scale)
    print(f"{case}: worst gradient max-error / max|g| {worst}, worst mean-error / max|g| {worst_mean}")
    assert worst[1] < 3.2e-2 and worst_mean[1] < 3.5e-3


def test_configs2_full_batch_bf16_step(env):
    """BASELINE configs[2] at its full per-GPU batch: base, bf16, 32 x 246000, dropout 0.1 + spec-augment, conv stack frozen.
    Properties that need no oracle at this size: the loss and every gradient are finite; the step is bit-reproducible (same seeds,
    twice: identical logits and flat gradient buffer); and rows 0-1 of the 32-row training forward equal the 2-row training forward's
    logits bit for bit (dropout masks are counters of (seed, site, element index), rows are independent, and every output row
    sums its products in the same order whatever slab / tile routing B T = 24576 rows take)."""
    import wav2vec2
    B, L = 32, 246000
    m, cfg, w = build("base_sample_padded", L)
    m.set_precision("bf16")
    T = cfg.num_frames(L)
    x = V.hash_normal("configs2/wave", B * L, 12).reshape(B, L).astype(np.float32)
    labels = _ragged_labels(B, 256, 24, 200, 6)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=B)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=1)
    spec = compute_mask_indices((B, T), 0.05, 10, rng=np.random.RandomState(4))
    runs = []
    for _ in range(2):
        logits = tr.forward(x, spec_mask=spec, step_seed=42)
        nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(dlog)
        runs.append((logits.cpu().numpy().copy(), tr.grad_buffer().cpu().numpy().copy(), nll.cpu().numpy().copy()))
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all() and np.isfinite(runs[0][2]).all()
    assert np.abs(runs[0][1]).max() > 0
    assert np.array_equal(runs[0][0], runs[1][0]), "logits differ between two identical steps"
    assert np.array_equal(runs[0][1], runs[1][1]), f"{int((runs[0][1] != runs[1][1]).sum())} gradient elements differ"
    two = tr.forward(x[:2], spec_mask=spec[:2], step_seed=42).cpu().numpy()
    assert np.array_equal(two, runs[0][0][:2]), f"rows 0-1 of the full batch differ from the 2-row forward by {H.max_err(two, runs[0][0][:2]):.3e}"


def test_configs4_full_batch_bf16_step(env):
    """BASELINE configs[4] at its full per-GPU batch: large-robust (24 L / 1024 d, prenorm, LayerNorm convs, attention mask), bf16,
    16 x 480000 (T = 1499: B T = 23984 rows, not a multiple of the 64-row K tile of the weight gradients), dropout 0.1 + spec-augment,
    conv stack frozen.  The same oracle-free properties as configs[2]: finite loss and gradients, a bit-reproducible step (logits and the
    whole flat gradient buffer), and rows 0-1 of the 16-row training forward equal to the 2-row training forward bit for bit -- the
    slab routing of the ragged weight-gradient rows and the 128 x 256 tiles at this size are exercised under assertion, not only in
    bench.py."""
    import wav2vec2
    B, L = 16, 480000
    m, cfg, w = build("robust_masked", L)
    m.set_precision("bf16")
    T = cfg.num_frames(L)
    assert T == 1499
    x = V.hash_normal("configs4/wave", B * L, 13).reshape(B, L).astype(np.float32)
    mask = np.ones((B, L), np.int32)
    mask[1, -70000:] = 0
    mask[5, -200001:] = 0
    x = (x * mask).astype(np.float32)
    labels = _ragged_labels(B, 256, 24, 200, 7)
    loss_fn = wav2vec2.CTCLoss(cfg, x.shape, division_factor=B)
    tr = wav2vec2.Trainer(m, loss_fn, dropout=0.1, apply_spec_augment=False, seed=2)
    spec = compute_mask_indices((B, T), 0.05, 10, rng=np.random.RandomState(5))
    runs = []
    for _ in range(2):
        logits = tr.forward(x, attention_mask=mask, spec_mask=spec, step_seed=43)
        nll, dlog = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(dlog)
        runs.append((logits.cpu().numpy().copy(), tr.grad_buffer().cpu().numpy().copy(), nll.cpu().numpy().copy()))
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all() and np.isfinite(runs[0][2]).all()
    assert np.abs(runs[0][1]).max() > 0
    assert np.array_equal(runs[0][0], runs[1][0]), "logits differ between two identical steps"
    assert np.array_equal(runs[0][1], runs[1][1]), f"{int((runs[0][1] != runs[1][1]).sum())} gradient elements differ"
    two = tr.forward(x[:2], attention_mask=mask[:2], spec_mask=spec[:2], step_seed=43).cpu().numpy()
    assert np.array_equal(two, runs[0][0][:2]), f"rows 0-1 of the full batch differ from the 2-row forward by {H.max_err(two, runs[0][0][:2]):.3e}"


def test_new_trainer_is_a_fresh_optimizer(env):
    """The reference builds a new Adam for stage 2 (src/main.py:213,240): iteration 0 AND zero moments.  The moments live in
    the model's native state, so a second Trainer on a used model must reset them; `reset_optimizer=False` adopts them."""
    import wav2vec2
    g = H.golden("tiny_base")
    m, cfg, w = build("tiny_base", 4000)
    loss_fn = wav2vec2.CTCLoss(cfg, g["wave"].shape, division_factor=2)
    t1 = wav2vec2.Trainer(m, loss_fn, learning_rate=1e-3, dropout=0.0, apply_spec_augment=False)
    for _ in range(3):
        t1.step(g["wave"], g["labels"])
    am, _ = t1._adam_views()
    assert float(am.abs().max()) > 0
    assert "adam_m" in t1.state_dict()
    keep = wav2vec2.Trainer(m, loss_fn, reset_optimizer=False)
    assert float(keep._adam_views()[0].abs().max()) > 0
    t2 = wav2vec2.Trainer(m, loss_fn, learning_rate=1e-3, dropout=0.0, apply_spec_augment=False)      # stage 2
    am, av = t2._adam_views()
    assert t2.iterations == 0 and float(am.abs().max()) == 0 and float(av.abs().max()) == 0
    # its first update is Keras Adam's first update from zero moments
    name = "encoder/layers/1/feed_forward/output_dense/kernel"
    before = m.get_weights()[name].astype(np.float64)
    logits = t2.forward(g["wave"], step_seed=1)
    _, dlog = loss_fn.per_sample(g["labels"], logits, with_grad=True)
    t2.backward(dlog)
    gr = t2.gradient(name).astype(np.float64)
    t2.apply_gradients()
    want, _, _ = TT.adam_reference(before, gr, 0.0, 0.0, 1e-3, 0.9, 0.999, 1e-7, 1)
    assert H.max_err(m.get_weights()[name], want) < 1e-6
    # a state without moments zeroes them on load
    st = t2.state_dict()
    st.pop("adam_m"), st.pop("adam_v")
    t2.load_state_dict(st)
    assert float(t2._adam_views()[0].abs().max()) == 0


def test_shape_change_keeps_transposed_kernels_and_bf16x3_planes_valid(env):
    """The transposed kernel copies (and the bf16x3 plane cache keyed by their addresses) survive a change of batch shape:
    forward + backward at a new (B, L) without an optimizer step in between gives the gradients of a fresh model."""
    import wav2vec2
    cfgname = "tiny_base"
    xa = V.hash_normal("train/shape_a", 2 * 4000, 3).reshape(2, 4000)
    xb = V.hash_normal("train/shape_b", 3 * 5000, 3).reshape(3, 5000)
    la, lb = np.array([[3, 4, 0], [5, 0, 0]], np.int32), np.array([[3, 4, 0], [5, 0, 0], [9, 9, 1]], np.int32)

    def run(m, cfg, x, labels):
        loss_fn = wav2vec2.CTCLoss(cfg, x.shape)
        tr = wav2vec2.Trainer(m, loss_fn, dropout=0.0, apply_spec_augment=False)
        logits = tr.forward(x, step_seed=1)
        _, d = loss_fn.per_sample(labels, logits, with_grad=True)
        tr.backward(d)
        return {n: tr.gradient(n) for n in ("lm_head/kernel", "encoder/layers/0/feed_forward/intermediate_dense/kernel",
                                             "encoder/layers/1/attention/q_proj/kernel", "feature_projection/projection/kernel")}

    for prec in ("fp32", "bf16x3"):
        m, cfg, w = build(cfgname, 4000)
        m.set_precision(prec)
        run(m, cfg, xa, la)
        got = run(m, cfg, xb, lb)                  # new shape, no optimizer step in between
        fresh, cfg2, _ = build(cfgname, 5000)
        fresh.set_precision(prec)
        want = run(fresh, cfg2, xb, lb)
        for n in want:
            assert np.array_equal(got[n], want[n]), (prec, n)


def test_ctc_rejects_out_of_range_labels_and_is_deterministic(env):
    lib, torch, dev = env
    import wav2vec2
    cfg = H.case_config("tiny_base")
    B, T, Vn = 3, 50, cfg.vocab_size
    logits = rnd("ctc_det", (B, T, Vn), 2.0)
    labels = np.array([[3, 4, 4, 7, 0], [5, 31, 0, 0, 0], [1, 2, 3, 4, 5]], np.int32)
    L = 16000
    while cfg.num_frames(L) != T:
        L += 80
    loss_fn = wav2vec2.CTCLoss(cfg, (B, L))
    nll, grad = loss_fn.per_sample(labels, logits, with_grad=True)
    ref_total, ref_nll = O.ctc_loss(cfg, labels, logits, (B, L))
    assert np.allclose(nll.cpu().numpy(), ref_nll, atol=1e-4)
    # bitwise reproducible gradient (integer fixed-point occupancy sums, no floating-point atomics)
    for _ in range(3):
        _, again = loss_fn.per_sample(labels, logits, with_grad=True)
        assert torch.equal(grad, again)
    # a label outside [0, V): host arrays are checked before the launch ...
    bad = labels.copy()
    bad[1, 1] = Vn
    with pytest.raises(ValueError):
        loss_fn.per_sample(bad, logits)
    bad[1, 1] = -1
    with pytest.raises(ValueError):
        loss_fn.per_sample(bad, logits)
    # ... device-resident labels are checked on the device: that sample's loss is NaN, its gradient rows are zero, the rest intact
    bad[1, 1] = Vn + 3
    nll_b, grad_b = loss_fn.per_sample(torch.from_numpy(bad).to(dev), logits, with_grad=True)
    nb = nll_b.cpu().numpy()
    assert np.isnan(nb[1]) and np.allclose(nb[[0, 2]], ref_nll[[0, 2]], atol=1e-4)
    assert not bool(grad_b[1].any()) and torch.equal(grad_b[0], grad[0]) and torch.equal(grad_b[2], grad[2])
