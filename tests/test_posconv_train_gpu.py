"""The positional convolution's training launch paths, one entry at a time, against tests/posconv_reference.py.

Exact tests: small-integer operands make every product and partial sum an integer below 2^24, exact in fp32 and in bf16, so the
fp32 kernels and the bf16 GEMM forms must equal the int64 reference bit for bit whatever their summation order; a wrong tap,
sample, segment stride, tile edge or pad cannot pass.  Float tests: seeded operands against the fp64 reference (the bf16 entries
against the fp64 reference of the bf16-rounded operands, which leaves the accumulation order only), with the error of a plain
fp32 evaluation of the same formula (e32) printed beside each kernel error."""

import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import posconv_reference as R
from wav2vec2 import _native as N
from wav2vec2 import variables as V

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import torch
    lib = N.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    return lib, torch, dev


def rnd(tag, shape, scale=1.0):
    n = int(np.prod(shape))
    return ((V.hash_uniform(tag, n, 11) * 2 - 1) * scale).reshape(shape).astype(np.float32)


def ints(tag, shape):
    """Integers in [-3, 3]."""
    n = int(np.prod(shape))
    return (np.minimum(np.floor(V.hash_uniform(tag, n, 11) * 7), 6).astype(np.int64) - 3).reshape(shape)


_KEEP = []


@pytest.fixture(autouse=True)
def _keepalive():
    """Raw pointers are handed to the C ABI: every device tensor must outlive the call."""
    _KEEP.clear()
    yield
    _KEEP.clear()


def dev_t(torch, dev, a, dtype=np.float32):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(dev)
    _KEEP.append(t)
    return t


def nan_t(torch, dev, shape):
    t = torch.full(tuple(shape), NAN, device=dev)
    _KEEP.append(t)
    return t


def nan16_t(torch, dev, n):
    """n bf16 elements, every one a NaN (0xFFFF)."""
    t = torch.full((int(n),), -1, dtype=torch.int16, device=dev)
    _KEEP.append(t)
    return t


def stream():
    return N.current_stream()


# ---------------------------------------------------------------- the entries ----------
def run_forward(env, path, x, wg, bias, flen, act, pad_left, add_residual, want_pre, expect_rc=0):
    """w2v2_op_pos_conv_ex (path "fp32") or w2v2_op_pos_conv_weight_shadow + w2v2_op_pos_conv_bf16 (path "bf16") -> (y, pre_act)."""
    lib, torch, dev = env
    B, T, Hh = x.shape
    G, K, cg, _ = wg.shape
    tx, tw, tb = dev_t(torch, dev, x), dev_t(torch, dev, wg), dev_t(torch, dev, bias)
    tf = dev_t(torch, dev, flen, np.int32)
    y = nan_t(torch, dev, (B, T, Hh))
    pre = nan_t(torch, dev, (B, T, Hh)) if want_pre else None
    if path == "fp32":
        rc = lib.w2v2_op_pos_conv_ex(N.ptr(tx), N.ptr(tw), N.ptr(tb), N.ptr(tf), N.ptr(y), N.ptr(pre), B, T, Hh, K, G, act, pad_left,
                                     add_residual, stream())
    else:
        w16 = nan16_t(torch, dev, G * K * cg * cg)
        N.check(lib.w2v2_op_pos_conv_weight_shadow(N.ptr(tw), N.ptr(w16), K, cg, G, stream()))
        pack = nan16_t(torch, dev, lib.w2v2_op_pos_conv_bf16_pack_elems(B, T, Hh, K))
        xz_ws = nan_t(torch, dev, (B, T, Hh)) if (flen is not None and add_residual) else None
        rc = lib.w2v2_op_pos_conv_bf16(N.ptr(tx), N.ptr(w16), N.ptr(tb), N.ptr(tf), N.ptr(y), N.ptr(pre), N.ptr(pack), N.ptr(xz_ws),
                                       B, T, Hh, K, G, act, pad_left, add_residual, stream())
    assert rc == expect_rc, (rc, N.last_error())
    return y.cpu().numpy(), (pre.cpu().numpy() if want_pre else None)


def dw_query(lib, B, T, Hh, K, G):
    sizes, S = (C.c_int64 * 4)(), C.c_int32(-1)
    N.check(lib.w2v2_pos_conv_dw_bf16_ws_floats(B, T, Hh, K, G, sizes, C.byref(S)))
    return list(sizes), S.value


def run_kernel_grad(env, path, xz, dc, K, G, expect_S=None):
    """w2v2_op_pos_conv_dw (fp32) or w2v2_op_pos_conv_dw_bf16 with the scratch its query asks for -> dwg (G, K, cg, cg)."""
    lib, torch, dev = env
    B, T, Hh = xz.shape
    cg = Hh // G
    tx, td = dev_t(torch, dev, xz), dev_t(torch, dev, dc)
    out = nan_t(torch, dev, (G, K, cg, cg))
    if path == "fp32":
        N.check(lib.w2v2_op_pos_conv_dw(N.ptr(tx), N.ptr(td), N.ptr(out), B, T, Hh, K, G, stream()))
    else:
        sizes, S = dw_query(lib, B, T, Hh, K, G)
        if expect_S is not None:
            assert S == expect_S, f"the slab rule picks S = {S} at (B, H, K, G) = {(B, Hh, K, G)}: this case was chosen for S = {expect_S}"
        Tk = (T + 63) // 64 * 64
        assert sizes[0] == B * (Tk + K - 1) * Hh and sizes[1] == S * K * cg * Hh and sizes[3] == (B * Tk * Hh if Tk != T else 0)
        pack32, slabs, red = (nan_t(torch, dev, (max(n, 1),)) for n in sizes[:3])
        dc_pad = nan_t(torch, dev, (sizes[3],)) if sizes[3] else None
        N.check(lib.w2v2_op_pos_conv_dw_bf16(N.ptr(tx), N.ptr(td), N.ptr(out), N.ptr(pack32), N.ptr(slabs), N.ptr(red), N.ptr(dc_pad),
                                             B, T, Hh, K, G, stream()))
    return out.cpu().numpy()


def run_flip(env, wg):
    lib, torch, dev = env
    G, K, cg, _ = wg.shape
    out = nan_t(torch, dev, wg.shape)
    N.check(lib.w2v2_op_pos_conv_flip_regroup(N.ptr(dev_t(torch, dev, wg)), N.ptr(out), K, cg, G, stream()))
    return out.cpu().numpy()


def run_weight_norm_bwd(env, wv, wgain, dwg, G):
    lib, torch, dev = env
    K, cg, Hh = wv.shape
    dv, dg = nan_t(torch, dev, wv.shape), nan_t(torch, dev, (K,))
    N.check(lib.w2v2_op_weight_norm_bwd(N.ptr(dev_t(torch, dev, wv)), N.ptr(dev_t(torch, dev, wgain)), N.ptr(dev_t(torch, dev, dwg)),
                                        N.ptr(dv), N.ptr(dg), K, cg, Hh, G, stream()))
    return dv.cpu().numpy(), dg.cpu().numpy()


# ---------------------------------------------------------------- exact: forward and data pass ----------
# (B, T, H, K, G, frame_len, role); role "fwd": bias, residual, pad_left = K/2; "data": no bias, no mask, no residual,
# pad_left = K-1-K/2, exactly the data-gradient call of the training step; an integer role is a pad_left of the forward form.
FWD_EXACT = [
    (2, 1, 64, 16, 4, None, "fwd"),               # cg 16; one frame
    (2, 12, 384, 128, 8, [12, 7], "fwd"),         # cg 48; T < K/2: every tap sees padding; groups % 8 == 0 (the XCD block map)
    (2, 63, 64, 16, 4, [63, 61], "fwd"),
    (2, 64, 128, 16, 4, [64, 61], "fwd"),         # cg 32
    (2, 65, 256, 16, 4, [65, 61], "fwd"),         # cg 64
    (1, 65, 64, 16, 4, [0], "fwd"),               # an empty sample: y = act(bias)
    (2, 127, 64, 128, 4, None, "fwd"),            # one frame short of the 128-frame block, K = 128
    (2, 128, 256, 16, 8, [128, 61], "fwd"),       # cg 32, groups % 8 == 0, exactly one block
    (2, 129, 384, 128, 8, [129, 61], "fwd"),      # second block of one frame, K = 128, cg 48
    (2, 200, 128, 16, 2, [200, 61], "fwd"),       # cg 64, two ragged blocks, 2 groups
    (2, 129, 384, 128, 8, None, "data"),
    (2, 200, 64, 16, 4, None, "data"),            # even K: pad_left 7 where the forward has 8
    (3, 65, 128, 16, 4, None, "data"),
    (2, 129, 64, 15, 4, [129, 61], "fwd"),        # odd K (fp32 entries only): pad_left 7 in both roles
    (2, 129, 64, 15, 4, None, "data"),
    (2, 200, 64, 15, 4, [200, 61], 8),            # and another left pad
]


@functools.lru_cache(maxsize=None)
def _fwd_exact_case(B, T, Hh, K, G, flen, role):
    cg = Hh // G
    x, wg = ints("ex", (B, T, Hh)), ints("ew", (G, K, cg, cg))
    if role == "data":
        bias, pad, res = None, K - 1 - K // 2, 0
    else:
        bias, pad, res = ints("eb", (Hh,)), (K // 2 if role == "fwd" else role), 1
    y, pre = R.forward(x, wg, bias, flen, 0, pad, res)
    assert y.dtype == np.int64 and K * cg * 9 + 6 < 2 ** 24 and max(np.abs(pre).max(), np.abs(y).max()) < 2 ** 24      # the premise
    for a in (x, wg, y, pre):
        a.setflags(write=False)
    return x, wg, bias, pad, res, y, pre


# (the bf16 form needs (K cg) % 64 == 0: the K = 15 cases are for the fp32 entry alone)
@pytest.mark.parametrize("path,B,T,Hh,K,G,flen,role", [(p,) + c for c in FWD_EXACT for p in ("fp32", "bf16")
                                                       if p == "fp32" or (c[3] * (c[2] // c[4])) % 64 == 0])
def test_forward_and_data_pass_exact(env, path, B, T, Hh, K, G, flen, role):
    """y and the pre-activation equal the int64 reference bit for bit, with and without the pre-activation requested."""
    x, wg, bias, pad, res, y, pre = _fwd_exact_case(B, T, Hh, K, G, tuple(flen) if flen else None, role)
    for want_pre in (True, False):
        got_y, got_pre = run_forward(env, path, x, wg, bias, flen, 0, pad, res, want_pre)
        bad = np.argwhere(got_y != y)
        assert bad.size == 0, f"{len(bad)} wrong elements, first (b, t, channel) = {bad[0]}, last {bad[-1]}: {got_y[tuple(bad[0])]} != {y[tuple(bad[0])]}"
        if want_pre:
            assert np.array_equal(got_pre, pre)


# ---------------------------------------------------------------- exact: kernel gradient ----------
DW32_EXACT = [
    (2, 1, 64, 16, 4), (2, 12, 384, 128, 8), (3, 63, 128, 16, 4), (2, 64, 256, 16, 4), (2, 65, 64, 15, 4), (2, 127, 64, 128, 4),
    (2, 128, 128, 16, 4), (2, 129, 384, 128, 8), (3, 200, 128, 16, 2), (2, 200, 64, 15, 4),
]
# (B, T, H, K, G, S): S is what the slab rule gives at (B, H, K, G); the case asserts it
DW16_EXACT = [
    (2, 65, 64, 16, 4, 2),          # one sample per slab, one padded tile
    (3, 63, 64, 16, 4, 1),          # three samples in one accumulator, 1 padded row each
    (3, 1, 64, 16, 4, 1),           # ... and 63 padded rows each
    (4, 64, 64, 16, 4, 4),
    (8, 129, 64, 16, 4, 4),         # two samples per slab, Tk = 192
    (6, 200, 64, 16, 4, 2),         # three per slab, Tk = 256
    (2, 128, 128, 16, 4, 2),        # cg 32
    (4, 12, 384, 128, 8, 4),        # cg 48, T < K/2
    (4, 64, 768, 128, 16, 2),       # two per slab at the base model's width
    (2, 127, 1024, 128, 16, 1),     # cg 64: two samples in one accumulator
]


@functools.lru_cache(maxsize=None)
def _dw_exact_case(B, T, Hh, K, G):
    xz, dc = ints("dx", (B, T, Hh)), ints("dd", (B, T, Hh))
    xz[B - 1, T - T // 3:] = 0                    # a masked tail, as the training step hands it over
    ref = R.kernel_grad(xz, dc, K, G)
    assert ref.dtype == np.int64 and B * T * 9 < 2 ** 24 and np.abs(ref).max() < 2 ** 24
    return xz, dc, ref


def _explain_dw(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} wrong elements; groups {sorted(set(bad[:, 0]))[:8]}, taps {sorted(set(bad[:, 1]))[:16]}, first (g, k, ci, co) = {bad[0]}"


@pytest.mark.parametrize("B,T,Hh,K,G", DW32_EXACT)
def test_kernel_grad_exact(env, B, T, Hh, K, G):
    xz, dc, ref = _dw_exact_case(B, T, Hh, K, G)
    got = run_kernel_grad(env, "fp32", xz, dc, K, G)
    assert np.array_equal(got, ref), _explain_dw(got, ref)


@pytest.mark.parametrize("B,T,Hh,K,G,S", DW16_EXACT)
def test_kernel_grad_bf16_exact(env, B, T, Hh, K, G, S):
    xz, dc, ref = _dw_exact_case(B, T, Hh, K, G)
    got = run_kernel_grad(env, "bf16", xz, dc, K, G, expect_S=S)
    assert np.array_equal(got, ref), _explain_dw(got, ref)


@pytest.mark.parametrize("B,Hh,K,G,S", [(2, 64, 16, 4, 2), (3, 64, 16, 4, 1), (4, 64, 16, 4, 4), (8, 64, 16, 4, 4), (6, 64, 16, 4, 2),
                                        (4, 384, 128, 8, 4), (4, 768, 128, 16, 2), (2, 1024, 128, 16, 1), (32, 768, 128, 16, 2)])
def test_slab_rule(env, B, Hh, K, G, S):
    assert dw_query(env[0], B, 64, Hh, K, G)[1] == S


@pytest.mark.parametrize("G,K,cg", [(16, 128, 48), (4, 15, 16), (2, 16, 64), (3, 1, 32)])
def test_flip_regroup_exact(env, G, K, cg):
    g, k, ci, co = np.meshgrid(np.arange(G), np.arange(K), np.arange(cg), np.arange(cg), indexing="ij")
    wg = (g * 10 ** 6 + k * 10 ** 4 + ci * 100 + co).astype(np.float32)
    assert wg.max() < 2 ** 24
    got = run_flip(env, wg)
    assert np.array_equal(got, R.flip_regroup(wg))
    assert got[G - 1, 0, 1, 0] == (G - 1) * 10 ** 6 + (K - 1) * 10 ** 4 + 1      # [g][K-1-k][co][ci] <- [g][k][ci][co], spelled out


# ---------------------------------------------------------------- float tests ----------
FLOAT_SHAPES = [(2, 200, 768, 128, 16, None), (2, 300, 1024, 128, 16, (300, 257)), (4, 129, 384, 128, 8, None), (3, 65, 128, 16, 4, None)]


def _report(what, err, e32, bar):
    print(f"\n{what}: kernel err {err:.3e}, plain fp32 e32 {e32:.3e}, bar {bar:.3e}" + ("   [above 8 x e32]" if err > 8 * e32 else ""))


@functools.lru_cache(maxsize=None)
def _float_inputs(B, T, Hh, K, G, flen):
    cg = Hh // G
    x, dc = rnd("fx", (B, T, Hh)), rnd("fd", (B, T, Hh))
    wv, wgain, bias = rnd("fv", (K, cg, Hh), 0.3), (0.5 + rnd("fg", (K,), 0.3) ** 2).astype(np.float32), rnd("fb", (Hh,), 0.1)
    wg = R.regroup(R.effective_kernel(wv, wgain), G).astype(np.float32)         # the regrouped kernel is an INPUT of these tests
    return x, dc, wv, wgain, bias, wg


@functools.lru_cache(maxsize=None)
def _float_conv(B, T, Hh, K, G, flen, role, bf16):
    """conv + bias of the forward (role "fwd") / conv of dc with the flipped kernel (role "data"): fp64 and plain fp32."""
    x, dc, _, _, bias, wg = _float_inputs(B, T, Hh, K, G, flen)
    if role == "fwd":
        args = (x, wg, bias, flen, 0, K // 2, 0)
    else:
        args = (dc, R.flip_regroup(wg), None, None, 0, K - 1 - K // 2, 0)
    return R.forward(*args, bf16=bf16)[1], R.forward(*args, dtype=np.float32, bf16=bf16)[1]


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("path", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,Hh,K,G,flen", FLOAT_SHAPES)
def test_forward_float(env, path, B, T, Hh, K, G, flen, act):
    """Training forward y = xz + act(conv + bias) and its pre-activation; bar 3e-5 max(1, max|ref|).
    Measured on the MI355X, kernel err / e32, act 1 (act 2 within 5 %), y then the pre-activation:
      fp32  (2,200,768,128,16) 1.23e-6 / 1.71e-7, 1.79e-6 / 1.83e-7    (2,300,1024,128,16) 1.28e-6 / 2.11e-7, 2.07e-6 / 2.35e-7
            (4,129,384,128,8)  1.50e-6 / 1.93e-7, 2.12e-6 / 2.22e-7    (3,65,128,16,4)     2.14e-7 / 1.17e-7, 3.38e-7 / 1.81e-7
      bf16  (2,200,768,128,16) 5.65e-7 / 1.29e-7, 7.26e-7 / 1.54e-7    (2,300,1024,128,16) 5.38e-7 / 1.50e-7, 6.80e-7 / 1.64e-7
            (4,129,384,128,8)  6.32e-7 / 1.77e-7, 1.03e-6 / 1.64e-7    (3,65,128,16,4)     1.11e-7 / 8.24e-8, 1.30e-7 / 9.09e-8
    The fp32 kernel's pre-activation sits 9 to 10 x above e32 at K = 128 (one MFMA accumulator chain over all 6144 / 8192 terms),
    20 x below the bar; the bf16 GEMM form, which sums in 64-deep tiles, is at 4 to 6 x."""
    x, _, _, _, bias, wg = _float_inputs(B, T, Hh, K, G, flen)
    pre64, pre32 = _float_conv(B, T, Hh, K, G, flen, "fwd", path == "bf16")
    xz = R.mask_rows(x, flen)
    ref = xz + R.act_fn(pre64, act)
    e32 = H.max_err(xz + R.act_fn(pre32, act), ref)
    y, pre = run_forward(env, path, x, wg, bias, list(flen) if flen else None, act, K // 2, 1, True)
    assert np.isfinite(y).all() and np.isfinite(pre).all()
    _report(f"pos_conv forward {path} {(B, T, Hh, K, G)} act {act} y", H.max_err(y, ref), e32, 3e-5 * max(1.0, np.abs(ref).max()))
    _report("   pre-activation", H.max_err(pre, pre64), H.max_err(pre32, pre64), 3e-5 * max(1.0, np.abs(pre64).max()))
    assert H.max_err(pre, pre64) < 3e-5 * max(1.0, np.abs(pre64).max())
    assert H.max_err(y, ref) < 3e-5 * max(1.0, np.abs(ref).max())
    if path == "bf16":
        assert H.max_err(pre64, _float_conv(B, T, Hh, K, G, flen, "fwd", False)[0]) > 1e-4      # the operand rounding matters


@pytest.mark.parametrize("path", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,Hh,K,G,flen", FLOAT_SHAPES)
def test_data_pass_float(env, path, B, T, Hh, K, G, flen):
    """dxz = conv(dc, flipped kernel, pad_left = K-1-K/2), the flipped kernel from the flip entry; bar 3e-5 max(1, max|ref|).
    Measured on the MI355X, kernel err / e32, in the order of FLOAT_SHAPES:
      fp32  1.70e-6 / 1.83e-7, 2.14e-6 / 1.65e-7, 2.13e-6 / 2.56e-7, 4.31e-7 / 1.35e-7     (8 to 13 x e32 at K = 128, as the forward)
      bf16  6.11e-7 / 1.24e-7, 6.91e-7 / 1.46e-7, 6.56e-7 / 1.56e-7, 1.25e-7 / 6.01e-8"""
    _, dc, _, _, _, wg = _float_inputs(B, T, Hh, K, G, flen)
    ref, ref32 = _float_conv(B, T, Hh, K, G, flen, "data", path == "bf16")
    wg_t = run_flip(env, wg)
    assert np.array_equal(wg_t, R.flip_regroup(wg))
    got, _ = run_forward(env, path, dc, wg_t, None, None, 0, K - 1 - K // 2, 0, False)
    assert np.isfinite(got).all()
    _report(f"pos_conv data pass {path} {(B, T, Hh, K, G)}", H.max_err(got, ref), H.max_err(ref32, ref), 3e-5 * max(1.0, np.abs(ref).max()))
    assert H.max_err(got, ref) < 3e-5 * max(1.0, np.abs(ref).max())
    if path == "bf16":
        assert H.max_err(ref, _float_conv(B, T, Hh, K, G, flen, "data", False)[0]) > 1e-4


@pytest.mark.parametrize("path", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,Hh,K,G,flen", FLOAT_SHAPES)
def test_kernel_grad_float(env, path, B, T, Hh, K, G, flen):
    """dWg from the masked input and dc; bar 2e-5 max(1, max|ref|) (contraction length B T <= 600).
    Measured on the MI355X, kernel err / e32, in the order of FLOAT_SHAPES (max|ref| is 22 to 40, so the bars are 4e-4 to 8e-4):
      fp32  3.03e-5 / 9.87e-6, 4.53e-5 / 1.40e-5, 3.52e-5 / 1.19e-5, 1.39e-5 / 4.24e-6
      bf16  5.38e-6 / 3.93e-6, 1.24e-5 / 6.30e-6, 3.82e-6 / 4.45e-6, 3.07e-6 / 1.85e-6"""
    x, dc, _, _, _, _ = _float_inputs(B, T, Hh, K, G, flen)
    xz = R.mask_rows(x, flen)
    ref = R.kernel_grad(xz, dc, K, G, bf16=path == "bf16")
    e32 = H.max_err(R.kernel_grad(xz, dc, K, G, dtype=np.float32, bf16=path == "bf16"), ref)
    got = run_kernel_grad(env, path, xz, dc, K, G)
    assert np.isfinite(got).all()
    _report(f"pos_conv kernel gradient {path} {(B, T, Hh, K, G)}", H.max_err(got, ref), e32, 2e-5 * max(1.0, np.abs(ref).max()))
    assert H.max_err(got, ref) < 2e-5 * max(1.0, np.abs(ref).max())
    if path == "bf16":
        assert H.max_err(ref, R.kernel_grad(xz, dc, K, G)) > 1e-4


def _check_weight_norm_bwd(env, what, wv, wgain, dwg, G):
    dv64, dg64 = R.weight_norm_bwd(wv, wgain, dwg)
    dv32, dg32 = R.weight_norm_bwd(wv, wgain, dwg, dtype=np.float32)
    dv, dg = run_weight_norm_bwd(env, wv, wgain, dwg, G)
    assert np.isfinite(dv).all() and np.isfinite(dg).all()
    _report(f"weight_norm_bwd {what} d weight_v", H.max_err(dv, dv64), H.max_err(dv32, dv64), 1e-6 * max(1.0, np.abs(dv64).max()))
    _report(f"weight_norm_bwd {what} d weight_g", H.max_err(dg, dg64), H.max_err(dg32, dg64), 1e-6 * max(1.0, np.abs(dg64).max()))
    assert H.max_err(dv, dv64) < 1e-6 * max(1.0, np.abs(dv64).max())
    assert H.max_err(dg, dg64) < 1e-6 * max(1.0, np.abs(dg64).max())
    for k in range(wv.shape[0]):      # a tap is one block's whole problem: the same bar tap by tap, so that a large tap hides no small one
        assert H.max_err(dv[k], dv64[k]) < 1e-6 * max(1.0, np.abs(dv64[k]).max()), k


@pytest.mark.parametrize("B,T,Hh,K,G,flen", FLOAT_SHAPES)
def test_weight_norm_bwd_float(env, B, T, Hh, K, G, flen):
    """(d weight_v, d weight_g) from a seeded dW_eff; the kernel works in fp64: bar 1e-6 max(1, max|ref|).
    Measured on the MI355X, kernel err / e32 over the whole tensors, d weight_v then d weight_g, in the order of FLOAT_SHAPES:
      9.3e-10 / 3.9e-9, 5.7e-8 / 2.6e-7;  4.7e-10 / 2.3e-9, 5.5e-8 / 2.2e-7;  9.3e-10 / 4.1e-9, 4.7e-8 / 2.1e-7;  1.9e-9 / 7.0e-9, 4.7e-8 / 1.7e-7
    (the kernel's error is the final rounding to fp32)."""
    _, _, wv, wgain, _, _ = _float_inputs(B, T, Hh, K, G, flen)
    _check_weight_norm_bwd(env, str((Hh, K, G)), wv, wgain, rnd("fdw", (G, K, Hh // G, Hh // G)), G)


def test_weight_norm_bwd_layout(env):
    """H = 64, 4 groups, 3 taps, a gradient that is one element at a time: only the (g, k, ci, co) <-> (k, ci, g og + co) map matters."""
    Hh, G, K = 64, 4, 3
    cg = Hh // G
    wv, wgain = rnd("lv", (K, cg, Hh), 0.3), (0.5 + rnd("lg", (K,), 0.3) ** 2).astype(np.float32)
    g, k, ci, co = np.meshgrid(np.arange(G), np.arange(K), np.arange(cg), np.arange(cg), indexing="ij")
    _check_weight_norm_bwd(env, "layout", wv, wgain, (g * 4.0 + k * 1.0 + ci * 0.25 - co * 0.0625).astype(np.float32), G)
    one = np.zeros((G, K, cg, cg), np.float32)
    one[2, 1, 3, 5] = 1.0
    dv, _ = run_weight_norm_bwd(env, wv, wgain, one, G)
    ref, _ = R.weight_norm_bwd(wv, wgain, one)
    assert np.unravel_index(np.abs(dv).argmax(), dv.shape) == np.unravel_index(np.abs(ref).argmax(), ref.shape) == (1, 3, 2 * cg + 5)


def test_weight_norm_bwd_clamped_norm(env):
    """One tap with sum v^2 < 1e-12: the norm is the clamp's 1e-6 there, in the kernel as in the reference."""
    Hh, G, K = 64, 4, 3
    cg = Hh // G
    wv, wgain = rnd("cv", (K, cg, Hh), 0.3), (0.5 + rnd("cg", (K,), 0.3) ** 2).astype(np.float32)
    wv[1] *= np.float32(1e-8)
    assert 0 < (wv[1].astype(np.float64) ** 2).sum() < 1e-12
    _check_weight_norm_bwd(env, "clamp", wv, wgain, rnd("cdw", (G, K, cg, cg)), G)


# ---------------------------------------------------------------- composition ----------
@pytest.mark.parametrize("path", ["fp32", "bf16"])
def test_block_backward_composed_from_the_entries(env, path):
    """The entries chained as the training step chains them -- forward with the pre-activation, GELU' on the host in fp64, kernel
    gradient, weight-norm backward; flip, data pass, + dpos, row mask -- at (2, 129, 384, 128, 8), frame_len [129, 100].
    fp32: d weight_v, d weight_g and dx against torch fp64 autograd of the whole block.  bf16: against the reference's pieces on
    bf16-rounded operands, fed the dc the chain itself formed (its pre-activation is checked first): a dc recomputed from the
    reference's pre-activation differs in the last fp32 bits, which moves a few of its 99072 elements across a bf16 rounding
    boundary -- 2^-9 relative each, far above the accumulation-order bar and no property of the kernels.
    The weight gradients are linear images of dWg and take dWg's bar, 2e-5 max(1, max|ref|); y and dx take 3e-5.
    Measured on the MI355X, kernel err / e32, for y, dx, d weight_v, d weight_g:
      fp32  1.30e-6 / 2.2e-7, 1.14e-6 / 1.52e-7, 1.75e-7 / 1.06e-7, 2.60e-6 / 1.86e-6
      bf16  4.76e-7 / 1.2e-7, 3.40e-7 / 1.10e-7, 7.99e-8 / 5.48e-8, 4.64e-7 / 8.02e-7"""
    lib, torch, dev = env
    B, T, Hh, K, G, flen, act = 2, 129, 384, 128, 8, [129, 100], 1
    cg = Hh // G
    x, dy = rnd("kx", (B, T, Hh)), rnd("kdy", (B, T, Hh))
    wv, wgain, bias = rnd("kv", (K, cg, Hh), 0.3), (0.5 + rnd("kg", (K,), 0.3) ** 2).astype(np.float32), rnd("kb", (Hh,), 0.1)
    twg = nan_t(torch, dev, (G, K, cg, cg))
    N.check(lib.w2v2_op_weight_norm_regroup(N.ptr(dev_t(torch, dev, wv)), N.ptr(dev_t(torch, dev, wgain)), N.ptr(twg), K, cg, Hh, G, stream()))
    wg = twg.cpu().numpy()
    xz = R.mask_rows(x, flen)
    # ---- the chain
    y, pre = run_forward(env, path, x, wg, bias, flen, act, K // 2, 1, True)
    dc = (dy.astype(np.float64) * R.act_grad(pre.astype(np.float64), act)).astype(np.float32)
    dwg = run_kernel_grad(env, path, xz, dc, K, G)
    dv, dg = run_weight_norm_bwd(env, wv, wgain, dwg, G)
    dxz, _ = run_forward(env, path, dc, run_flip(env, wg), None, None, 0, K - 1 - K // 2, 0, False)
    dx = R.mask_rows(dxz + dy, flen)
    # ---- the reference
    if path == "fp32":
        tx, tv, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wv, wgain, bias))
        m = torch.ones(B, T, 1, dtype=torch.float64)
        for b, n in enumerate(flen):
            m[b, n:] = 0
        nrm = torch.sqrt(torch.clamp((tv * tv).sum(dim=(1, 2), keepdim=True), min=1e-12))
        c = torch.nn.functional.conv1d((tx * m).transpose(1, 2), (tv / nrm * tg.reshape(-1, 1, 1)).permute(2, 1, 0), tb, padding=K // 2,
                                    groups=G).transpose(1, 2)[:, :-1]
        ty = tx * m + torch.nn.functional.gelu(c)
        ty.backward(torch.from_numpy(dy.astype(np.float64)))
        ref_y, ref_dv, ref_dg, ref_dx = ty.detach().numpy(), tv.grad.numpy(), tg.grad.numpy(), tx.grad.numpy()
        wg64 = R.regroup(R.effective_kernel(wv, wgain), G)
        y32, pre32 = R.forward(x, wg64, bias, flen, act, K // 2, 1, dtype=np.float32)
        dc32 = dy * R.act_grad(pre32, act)
        dw32 = R.kernel_grad(xz, dc32, K, G, dtype=np.float32)
        dx32 = R.mask_rows(dy + R.conv(dc32, R.flip_regroup(wg64), K - 1 - K // 2, dtype=np.float32), flen)
    else:
        ref_y, ref_pre = R.forward(x, wg, bias, flen, act, K // 2, 1, bf16=True)
        y32 = R.forward(x, wg, bias, flen, act, K // 2, 1, dtype=np.float32, bf16=True)[0]
        assert H.max_err(pre, ref_pre) < 3e-5 * max(1.0, np.abs(ref_pre).max())
        ref_dw = R.kernel_grad(xz, dc, K, G, bf16=True)
        ref_dv, ref_dg = R.weight_norm_bwd(wv, wgain, ref_dw)
        ref_dx = R.mask_rows(dy + R.conv(dc, R.flip_regroup(wg), K - 1 - K // 2, bf16=True), flen)
        dw32 = R.kernel_grad(xz, dc, K, G, dtype=np.float32, bf16=True)
        dx32 = R.mask_rows(dy + R.conv(dc, R.flip_regroup(wg), K - 1 - K // 2, dtype=np.float32, bf16=True), flen)
    dv32, dg32 = R.weight_norm_bwd(wv, wgain, dw32, dtype=np.float32)
    bars = {"y": 3e-5, "dx": 3e-5, "d weight_v": 2e-5, "d weight_g": 2e-5}        # the weight gradients carry dWg's error: dWg's bar
    pairs = {"y": (y, ref_y, y32), "dx": (dx, ref_dx, dx32), "d weight_v": (dv, ref_dv, dv32), "d weight_g": (dg, ref_dg, dg32)}
    for name, (got, ref, f32) in pairs.items():
        assert np.isfinite(got).all()
        _report(f"composed {path} {name}", H.max_err(got, ref), H.max_err(f32, ref), bars[name] * max(1.0, np.abs(ref).max()))
    for name, (got, ref, _) in pairs.items():
        assert H.max_err(got, ref) < bars[name] * max(1.0, np.abs(ref).max()), name


# ---------------------------------------------------------------- rejections ----------
def test_rejections(env):
    """Each returns W2V2_EINVAL with its launcher's message, and leaves the NaN-filled outputs untouched."""
    lib, torch, dev = env

    def rejected(call, msg, *outs):
        assert call() == -1
        assert msg in lib.w2v2_last_error(), lib.w2v2_last_error()
        for o in outs:
            assert torch.isnan(o).all()

    # 24 channels per group on the fp32 entries
    B, T, Hh, K, G = 2, 64, 96, 16, 4
    cg = Hh // G
    x, wg, y, dwg = nan_t(torch, dev, (B, T, Hh)), nan_t(torch, dev, (G, K, cg, cg)), nan_t(torch, dev, (B, T, Hh)), nan_t(torch, dev, (G, K, cg, cg))
    rejected(lambda: lib.w2v2_op_pos_conv_ex(N.ptr(x), N.ptr(wg), None, None, N.ptr(y), None, B, T, Hh, K, G, 0, K // 2, 1, stream()),
             b"pos_conv: channels per group = 24", y)
    rejected(lambda: lib.w2v2_op_pos_conv_dw(N.ptr(x), N.ptr(x), N.ptr(dwg), B, T, Hh, K, G, stream()), b"pos_conv_dw: channels per group = 24", dwg)
    # pad_left = K
    B, T, Hh, K, G = 2, 64, 64, 16, 4
    cg = Hh // G
    x, wg, y = nan_t(torch, dev, (B, T, Hh)), nan_t(torch, dev, (G, K, cg, cg)), nan_t(torch, dev, (B, T, Hh))
    w16, pack, flen = nan16_t(torch, dev, G * K * cg * cg), nan16_t(torch, dev, lib.w2v2_op_pos_conv_bf16_pack_elems(B, T, Hh, K)), dev_t(torch, dev, [64, 61], np.int32)
    rejected(lambda: lib.w2v2_op_pos_conv_ex(N.ptr(x), N.ptr(wg), None, None, N.ptr(y), None, B, T, Hh, K, G, 0, K, 1, stream()),
             b"pos_conv: bad left pad", y)
    rejected(lambda: lib.w2v2_op_pos_conv_bf16(N.ptr(x), N.ptr(w16), None, None, N.ptr(y), None, N.ptr(pack), None, B, T, Hh, K, G, 0, K, 1,
                                               stream()), b"pos_conv_bf16: bad sizes", y)
    # the bf16 forward: a masked residual without its workspace; (K cg) % 64 != 0
    rejected(lambda: lib.w2v2_op_pos_conv_bf16(N.ptr(x), N.ptr(w16), None, N.ptr(flen), N.ptr(y), None, N.ptr(pack), None, B, T, Hh, K, G, 0,
                                               K // 2, 1, stream()), b"pos_conv_bf16: the masked residual needs", y)
    rejected(lambda: lib.w2v2_op_pos_conv_bf16(N.ptr(x), N.ptr(w16), None, None, N.ptr(y), None, N.ptr(pack), None, B, T, Hh, 15, G, 0, 7, 1,
                                               stream()), b"pos_conv_bf16: channels per group 16 / taps 15", y)
    # the bf16 kernel gradient: 65 samples; T % 64 != 0 without dc_pad
    for Bb, Tt in ((65, 64), (2, 65)):
        sizes, _ = dw_query(lib, Bb, Tt, Hh, K, G)
        xz, dwg = nan_t(torch, dev, (Bb, Tt, Hh)), nan_t(torch, dev, (G, K, cg, cg))
        pack32, slabs, red = (nan_t(torch, dev, (n,)) for n in sizes[:3])
        dc_pad = nan_t(torch, dev, (sizes[3],)) if Bb == 65 and sizes[3] else None
        rejected(lambda: lib.w2v2_op_pos_conv_dw_bf16(N.ptr(xz), N.ptr(xz), N.ptr(dwg), N.ptr(pack32), N.ptr(slabs), N.ptr(red), N.ptr(dc_pad),
                                                      Bb, Tt, Hh, K, G, stream()), b"pos_conv_dw_bf16: unsupported shape", dwg, slabs, pack32)
    assert lib.w2v2_pos_conv_dw_bf16_ws_floats(2, 64, 64, 16, 0, (C.c_int64 * 4)(), None) == -1
