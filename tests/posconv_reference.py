"""High-precision reference of the positional convolution block and of its gradients, piece by piece, written from the
formulas (PositionalConvEmbedding, encoder.py:153-181; Conv1DWithWeightNorm, tensorflow_addons.py:5-58):

    W_eff[k]  = g[k] v[k] / n[k],  n[k]^2 = max(sum v[k]^2, 1e-12)                      (weight norm, per tap)
    c[b,t,o]  = sum_{k,ci} xz[b, t + k - pad_left, G(o) cg + ci] W[G(o)][k][ci][o % cg] + bias[o]
    y         = [xz +] act(c)                                                           (xz: x, frames >= frame_len[b] zeroed)
    dWg[g][k][ci][co] = sum_{b,t} xz[b, t + k - K/2, g cg + ci] dc[b, t, g cg + co]     (kernel gradient)
    wg_t[g][K-1-k][co][ci] = wg[g][k][ci][co];  dxz = conv(dc, wg_t, pad_left = K-1-K/2)  (data gradient)
    dg[k] = <dW[k], v[k]> / n[k];  dv[k] = (g[k] / n[k]) (dW[k] - <dW[k], v[k]> v[k] / n[k]^2)

Layouts are the library's: activations (B, T, H); the regrouped kernel wg (groups, K, cg, cg) with cg = H / groups; weight_v
(K, cg, H), weight_g (K) or (K, 1, 1).

Arithmetic: fp64 by default.  `dtype=np.float32` evaluates the same formulas in plain fp32 (the tests' yardstick e32 for what
fp32 arithmetic costs at a shape).  `bf16=True` rounds the two operands of the contraction to bfloat16 first (nearest even,
`O.round_bf16`) and leaves everything else alone, which is what precision mode 1 computes up to the order of its fp32 sums.
Integer inputs (any numpy integer dtype) give exact int64 results.  The contractions run as matrix products of torch CPU tensors.
"""

import math

import numpy as np
import torch

from oracle import w2v2_oracle as O

INT_EXACT = 2 ** 53      # integer contractions run as fp64 matrix products: exact while every partial sum stays below this


def _is_int(*arrays):
    return all(np.issubdtype(np.asarray(a).dtype, np.integer) for a in arrays)


def _operands(a, b, dtype, bf16):
    """The two operands of a contraction in the working dtype, and whether the result is an exact integer."""
    exact = _is_int(a, b)
    a, b = np.asarray(a), np.asarray(b)
    if bf16:
        a, b = O.round_bf16(a.astype(np.float32)), O.round_bf16(b.astype(np.float32))
    work = np.float64 if exact else dtype
    return a.astype(work), b.astype(work), exact


def _mm(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


def _finish_int(r, bound):
    assert bound < INT_EXACT, "integer operands too large for the exact path"
    q = np.rint(r)
    assert np.array_equal(q, r)
    return q.astype(np.int64)


def _windows(x, K, pad_left, g, cg):
    """(B, T, K cg) view: row t of sample b holds frames t - pad_left .. t - pad_left + K - 1 of group g's channels (zero outside)."""
    B, T, _ = x.shape
    xp = np.zeros((B, T + K - 1, cg), x.dtype)
    xp[:, pad_left:pad_left + T] = x[:, :, g * cg:(g + 1) * cg]
    it = xp.itemsize
    return np.lib.stride_tricks.as_strided(xp, shape=(B, T, K * cg), strides=((T + K - 1) * cg * it, cg * it, it))


def mask_rows(x, frame_len):
    """x with the frames >= frame_len[b] of sample b zeroed (a copy)."""
    xz = np.array(x, copy=True)
    if frame_len is not None:
        for b, n in enumerate(frame_len):
            xz[b, int(n):] = 0
    return xz


def effective_kernel(weight_v, weight_g, dtype=np.float64):
    """(K, cg, H) kernel g v / n with n^2 = max(sum over the tap of v^2, 1e-12)."""
    v = np.asarray(weight_v, dtype)
    n = np.sqrt(np.maximum((v * v).sum(axis=(1, 2), keepdims=True), dtype(1e-12)))
    return v * (np.asarray(weight_g, dtype).reshape(-1, 1, 1) / n)


def regroup(kernel, groups):
    """(K, cg, H) -> wg (groups, K, cg, og): wg[g][k][ci][co] = kernel[k][ci][g og + co]."""
    K, cg, H = kernel.shape
    og = H // groups
    return np.ascontiguousarray(kernel.reshape(K, cg, groups, og).transpose(2, 0, 1, 3))


def ungroup(wg):
    """Inverse of regroup."""
    G, K, cg, og = wg.shape
    return np.ascontiguousarray(wg.transpose(1, 2, 0, 3).reshape(K, cg, G * og))


def flip_regroup(wg):
    """wg_t[g][K-1-k][co][ci] = wg[g][k][ci][co]."""
    return np.ascontiguousarray(wg[:, ::-1].transpose(0, 1, 3, 2))


def conv(xz, wg, pad_left, dtype=np.float64, bf16=False):
    """out[b, t, g cg + co] = sum_{k, ci} xz[b, t + k - pad_left, g cg + ci] wg[g][k][ci][co], zero outside [0, T)."""
    G, K, cg, og = wg.shape
    B, T, H = xz.shape
    assert H == G * cg and cg == og and 0 <= pad_left < K
    x, w, exact = _operands(xz, wg, dtype, bf16)
    out = np.empty((B, T, H), x.dtype)
    for g in range(G):
        win = _windows(x, K, pad_left, g, cg)
        wm = w[g].reshape(K * cg, og)
        for b in range(B):
            out[b, :, g * og:(g + 1) * og] = _mm(win[b], wm)
    if exact:
        return _finish_int(out, float(np.abs(x).max(initial=0)) * float(np.abs(w).max(initial=0)) * K * cg)
    return out


def act_fn(c, act):
    """0: identity; 1: x Phi(x) (exact GELU); 2: the tanh approximation."""
    if act == 0:
        return c
    t = torch.from_numpy(np.ascontiguousarray(c))
    if act == 1:
        return (0.5 * t * (1.0 + torch.erf(t * (1.0 / math.sqrt(2.0))))).numpy()
    u = math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)
    return (0.5 * t * (1.0 + torch.tanh(u))).numpy()


def act_grad(c, act):
    """d act(c) / dc."""
    if act == 0:
        return np.ones_like(c)
    t = torch.from_numpy(np.ascontiguousarray(c))
    if act == 1:
        return (0.5 * (1.0 + torch.erf(t * (1.0 / math.sqrt(2.0)))) + t * torch.exp(-0.5 * t * t) * (1.0 / math.sqrt(2.0 * math.pi))).numpy()
    k = math.sqrt(2.0 / math.pi)
    th = torch.tanh(k * (t + 0.044715 * t ** 3))
    return (0.5 * (1.0 + th) + 0.5 * t * (1.0 - th * th) * k * (1.0 + 3 * 0.044715 * t * t)).numpy()


def forward(x, wg, bias, frame_len, act, pad_left, add_residual, dtype=np.float64, bf16=False):
    """(y, pre): pre = conv(xz, wg, pad_left) + bias, y = [xz +] act(pre).  The residual is the unrounded masked input."""
    xz = mask_rows(x, frame_len)
    pre = conv(xz, wg, pad_left, dtype, bf16)
    exact = pre.dtype == np.int64
    if bias is not None:
        assert not exact or _is_int(bias)
        pre = pre + np.asarray(bias, pre.dtype)
    if exact:
        assert act == 0
        return (xz.astype(np.int64) + pre if add_residual else pre), pre
    y = act_fn(pre, act)
    return (xz.astype(pre.dtype) + y if add_residual else y), pre


def kernel_grad(xz, dc, K, groups, dtype=np.float64, bf16=False):
    """dWg[g][k][ci][co] = sum_{b, t} xz[b, t + k - K/2, g cg + ci] dc[b, t, g cg + co]  (xz already masked)."""
    B, T, H = xz.shape
    cg = H // groups
    x, d, exact = _operands(xz, dc, dtype, bf16)
    out = np.zeros((groups, K, cg, cg), x.dtype)
    for g in range(groups):
        win = _windows(x, K, K // 2, g, cg)
        for b in range(B):
            out[g] += _mm(win[b].T, d[b, :, g * cg:(g + 1) * cg]).reshape(K, cg, cg)
    if exact:
        return _finish_int(out, float(np.abs(x).max(initial=0)) * float(np.abs(d).max(initial=0)) * B * T)
    return out


def weight_norm_bwd(weight_v, weight_g, dwg, dtype=np.float64):
    """(d weight_v (K, cg, H), d weight_g (K)) from dwg (groups, K, cg, og), the gradient w.r.t. the regrouped effective kernel."""
    v = np.asarray(weight_v, dtype)
    g = np.asarray(weight_g, dtype).reshape(-1, 1, 1)
    dW = ungroup(np.asarray(dwg, dtype))
    n2 = np.maximum((v * v).sum(axis=(1, 2), keepdims=True), dtype(1e-12))
    n = np.sqrt(n2)
    dot = (dW * v).sum(axis=(1, 2), keepdims=True)
    return (g / n) * (dW - dot * v / n2), (dot / n).reshape(-1)
