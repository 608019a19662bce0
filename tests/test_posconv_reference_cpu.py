"""tests/posconv_reference.py against torch fp64 autograd of the whole positional-conv block and against brute-force loops.

The block, as the model defines it: weight norm per tap, zero-pad K/2 on both sides, grouped Conv1D (valid), drop the last frame
when K is even, activation, residual on the masked input.  Its gradients, assembled from the reference's pieces, must equal
autograd's; that pins "data gradient = conv with the flipped kernel at pad_left = K - 1 - K/2" without a GPU."""

import numpy as np
import pytest
import torch

import posconv_reference as R
from oracle import w2v2_oracle as O

# (B, T, H, K, groups, frame_len, act): odd and even K, a frame_len mask (with an empty sample), the three activations
SHAPES = [(2, 9, 8, 3, 2, [9, 5], 1), (2, 7, 16, 4, 4, [7, 4], 2), (3, 11, 12, 6, 3, [11, 0, 5], 0), (1, 6, 8, 5, 1, None, 1)]


def _inputs(B, T, H, K, G):
    rng = np.random.default_rng(1000 * T + K)
    cg = H // G
    return (rng.standard_normal((B, T, H)), rng.standard_normal((K, cg, H)) * 0.5, 0.5 + rng.random(K), rng.standard_normal(H) * 0.3,
            rng.standard_normal((B, T, H)))


def _torch_block(x, wv, wgain, bias, flen, K, G, act):
    """y of the block in torch fp64; x, wv, wgain, bias are leaf tensors."""
    B, T, H = x.shape
    m = torch.ones(B, T, 1, dtype=torch.float64)
    if flen is not None:
        for b, n in enumerate(flen):
            m[b, n:] = 0
    xz = x * m
    n = torch.sqrt(torch.clamp((wv * wv).sum(dim=(1, 2), keepdim=True), min=1e-12))
    kern = wv / n * wgain.reshape(-1, 1, 1)                                   # (K, cg, H)
    c = torch.nn.functional.conv1d(xz.transpose(1, 2), kern.permute(2, 1, 0), bias, padding=K // 2, groups=G).transpose(1, 2)
    if K % 2 == 0:
        c = c[:, :-1]
    a = c if act == 0 else torch.nn.functional.gelu(c, approximate="tanh" if act == 2 else "none")
    return xz + a, c


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, float(np.abs(b).max())))


@pytest.mark.parametrize("B,T,H,K,G,flen,act", SHAPES)
def test_reference_pieces_equal_autograd_of_the_block(B, T, H, K, G, flen, act):
    x, wv, wgain, bias, dy = _inputs(B, T, H, K, G)
    tx, tv, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wv, wgain, bias))
    ty, tc = _torch_block(tx, tv, tg, tb, flen, K, G, act)
    ty.backward(torch.from_numpy(dy))

    wg = R.regroup(R.effective_kernel(wv, wgain), G)
    y, pre = R.forward(x, wg, bias, flen, act, K // 2, 1)
    assert _rel(pre, tc.detach().numpy()) < 1e-10 and _rel(y, ty.detach().numpy()) < 1e-10
    dc = dy * R.act_grad(pre, act)
    assert _rel(dc.sum(axis=(0, 1)), tb.grad.numpy()) < 1e-10
    dv, dg = R.weight_norm_bwd(wv, wgain, R.kernel_grad(R.mask_rows(x, flen), dc, K, G))
    assert _rel(dv, tv.grad.numpy()) < 1e-10 and _rel(dg, tg.grad.numpy()) < 1e-10
    dxz, _ = R.forward(dc, R.flip_regroup(wg), None, None, 0, K - 1 - K // 2, 0)
    assert _rel(R.mask_rows(dy + dxz, flen), tx.grad.numpy()) < 1e-10
    # the other left pad is a different function for every K (for odd K the two pads coincide: then shift by one)
    wrong, _ = R.forward(dc, R.flip_regroup(wg), None, None, 0, (K // 2) if K % 2 == 0 else K // 2 - 1, 0)
    assert _rel(R.mask_rows(dy + wrong, flen), tx.grad.numpy()) > 1e-3


def test_reference_pieces_equal_brute_force_loops():
    B, T, H, K, G, flen, _ = SHAPES[0]
    cg = H // G
    x, wv, wgain, bias, dc = _inputs(B, T, H, K, G)
    n = np.array([max(sum(wv[k, i, o] ** 2 for i in range(cg) for o in range(H)), 1e-12) ** 0.5 for k in range(K)])
    wg = R.regroup(R.effective_kernel(wv, wgain), G)
    for pad in (K // 2, K - 1 - K // 2, 0):
        pre = np.zeros((B, T, H))
        for b in range(B):
            for t in range(T):
                for o in range(H):
                    g = o // cg
                    s = bias[o]
                    for k in range(K):
                        tt = t + k - pad
                        if 0 <= tt < min(T, flen[b]):
                            for ci in range(cg):
                                s += x[b, tt, g * cg + ci] * wgain[k] * wv[k, ci, o] / n[k]
                    pre[b, t, o] = s
        assert _rel(R.forward(x, wg, bias, flen, 0, pad, 0)[1], pre) < 1e-12
    xz = R.mask_rows(x, flen)
    dW = np.zeros((G, K, cg, cg))
    wt = np.zeros((G, K, cg, cg))
    for g in range(G):
        for k in range(K):
            for ci in range(cg):
                for co in range(cg):
                    wt[g, K - 1 - k, co, ci] = wg[g, k, ci, co]
                    dW[g, k, ci, co] = sum(xz[b, t + k - K // 2, g * cg + ci] * dc[b, t, g * cg + co]
                                           for b in range(B) for t in range(T) if 0 <= t + k - K // 2 < T)
    assert np.array_equal(R.flip_regroup(wg), wt)
    assert _rel(R.kernel_grad(xz, dc, K, G), dW) < 1e-12
    dv, dg = R.weight_norm_bwd(wv, wgain, dW)
    for k in range(K):
        dot = sum(dW[o // cg, k, ci, o % cg] * wv[k, ci, o] for ci in range(cg) for o in range(H))
        assert abs(dg[k] - dot / n[k]) < 1e-12
        for ci in range(cg):
            for o in range(H):
                assert abs(dv[k, ci, o] - wgain[k] / n[k] * (dW[o // cg, k, ci, o % cg] - dot * wv[k, ci, o] / n[k] ** 2)) < 1e-12


def test_integer_path_is_exact_and_the_switches_do_what_they_say():
    B, T, H, K, G = 2, 9, 8, 3, 2
    rng = np.random.default_rng(5)
    x, dc = rng.integers(-3, 4, (B, T, H)), rng.integers(-3, 4, (B, T, H))
    wg, bias = rng.integers(-3, 4, (G, K, H // G, H // G)), rng.integers(-3, 4, H)
    y, pre = R.forward(x, wg, bias, [9, 4], 0, 1, 1)
    yf, pref = R.forward(x.astype(np.float64), wg.astype(np.float64), bias.astype(np.float64), [9, 4], 0, 1, 1)
    assert y.dtype == np.int64 and pre.dtype == np.int64 and np.array_equal(y, yf) and np.array_equal(pre, pref)
    dw = R.kernel_grad(x, dc, K, G)
    assert dw.dtype == np.int64 and np.array_equal(dw, R.kernel_grad(x.astype(np.float64), dc.astype(np.float64), K, G))
    assert np.array_equal(R.kernel_grad(x, dc, K, G, bf16=True), dw)          # small integers are bf16 numbers
    # rounded operands: the same function of the rounded arrays, and a different one of the originals
    xf, df = rng.standard_normal((B, T, H)).astype(np.float32), rng.standard_normal((B, T, H)).astype(np.float32)
    a = R.kernel_grad(xf, df, K, G, bf16=True)
    assert np.array_equal(a, R.kernel_grad(O.round_bf16(xf), O.round_bf16(df), K, G)) and _rel(a, R.kernel_grad(xf, df, K, G)) > 1e-4
    wf = rng.standard_normal(wg.shape).astype(np.float32)
    a = R.forward(xf, wf, None, None, 1, 1, 1, bf16=True)[0]
    b = xf + R.forward(O.round_bf16(xf), O.round_bf16(wf), None, None, 1, 1, 0)[0]
    assert _rel(a, b) < 1e-15 and _rel(a, R.forward(xf, wf, None, None, 1, 1, 1)[0]) > 1e-4
    # fp32 evaluation: close to, and not the same as, the fp64 one
    e = _rel(R.forward(xf, wf, None, None, 2, 1, 1, dtype=np.float32)[0], R.forward(xf, wf, None, None, 2, 1, 1)[0])
    assert 0 < e < 1e-5
    # GELU' against a central difference
    c = np.linspace(-4, 4, 101)
    for act in (1, 2):
        num = (R.act_fn(c + 1e-6, act) - R.act_fn(c - 1e-6, act)) / 2e-6
        assert np.abs(R.act_grad(c, act) - num).max() < 1e-8
