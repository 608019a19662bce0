"""Every recorded row of tests/golden/attention_routes.json run once on the GPU through the op it names, at the row's own shape: the
launch counter of the recorded kernel (w2v2_op_attention_launches) rises by one and no other moves, and the output meets the bound
the suite already applies to that family against the fp64 formula -- the fp32 and split kernels test_ops_gpu.py's 2e-5, the bf16
kernel its 2e-2 (mean 2e-3) against bf16-rounded q d^-0.5, k, v; a training forward runs without dropout and is the same function,
held to the same bound; a backward is held to test_train_gpu.py's bounds on the gradient (5e-5 of its magnitude, bf16 kernels 1e-2,
mean 1e-3) against torch autograd in fp64.  A refused row returns the recorded message and launches nothing.

run_row uses only ops older than the route (tools/attention_route_record.py runs it on the commit before it)."""

import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import w2v2_oracle as O
from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_routes.json")
TABLE = json.load(open(GOLDEN))
KERNELS, ROWS = TABLE["kernels"], [r for r in TABLE["rows"] if r["op"] is not None]
SEED, STREAM = 991, 16


def qkv_of(row):
    a = row["args"]
    g = np.random.default_rng(len(row["name"]) + 7 * a["T"] + a["H"])
    return ((g.random((a["B"], a["T"], 3 * a["H"]), dtype=np.float32) * 2 - 1) * 2.0)


def segments(row):
    """(batch, first frame, frames) of every sequence that attends within itself"""
    a = row["args"]
    cu = a.get("cu_frames")
    return [(0, cu[i], cu[i + 1] - cu[i]) for i in range(len(cu) - 1)] if cu else [(b, 0, a["T"]) for b in range(a["B"])]


def run_row(lib, torch, dev, row, qkv, between=lambda: None):
    """(return code, output) of the row's own call; the thread's precision is the row's for the call alone.  A backward row runs the
    training forward first (its ctx and lse are inputs): `between` is called between the two."""
    a, s = row["args"], N.current_stream()
    B, T, Hh, heads = a["B"], a["T"], a["H"], a["heads"]
    tq = torch.from_numpy(qkv).to(dev)
    out = torch.full((B, T, Hh), float("nan"), device=dev)
    N.check(lib.w2v2_op_set_precision(a["mode"]))
    try:
        if row["op"] == "attention":
            rc = lib.w2v2_op_attention(N.ptr(tq), None, N.ptr(out), B, T, Hh, heads, s)
        elif row["op"] == "attention_packed":
            cu = (C.c_int32 * len(a["cu_frames"]))(*a["cu_frames"])
            rc = lib.w2v2_op_attention_packed(N.ptr(tq), len(a["cu_frames"]) - 1, cu, N.ptr(out), None, 0, None, Hh, heads, s)
        elif row["op"] == "attention_packed_bf16":
            cu = (C.c_int32 * len(a["cu_frames"]))(*a["cu_frames"])
            rc = lib.w2v2_op_attention_packed_bf16(N.ptr(tq), None, len(a["cu_frames"]) - 1, cu, N.ptr(out), None, Hh, heads, s)
        else:
            lse = torch.full((B, heads, T), float("nan"), device=dev)
            rc = lib.w2v2_op_attention_train(N.ptr(tq), None, N.ptr(out), N.ptr(lse), B, T, Hh, heads, 0.0, C.c_uint64(SEED), STREAM, s)
            if row["op"] == "attention_bwd":
                if rc != 0:      # no forward of this shape exists: the backward's own refusal is what the row records
                    out.zero_()
                    lse.zero_()
                between()
                g = np.random.default_rng(5).random((B, T, Hh), dtype=np.float32) * 2 - 1
                dqkv, ws = torch.full((B, T, 3 * Hh), float("nan"), device=dev), torch.empty((B, heads, T), device=dev)
                rc = lib.w2v2_op_attention_bwd(N.ptr(tq), None, N.ptr(out), N.ptr(lse), N.ptr(torch.from_numpy(g).to(dev)), N.ptr(dqkv), N.ptr(ws), B, T,
                                               Hh, heads, 0.0, C.c_uint64(SEED), STREAM, s)
                out = dqkv
        torch.cuda.synchronize()
    finally:
        N.check(lib.w2v2_op_set_precision(0))
    return rc, out



def reference(torch, row, qkv, bf16):
    """ctx (or, for a backward row, d qkv for the row's dctx) by the fp64 formula; bf16: on bf16-rounded q d^-0.5, k, v"""
    a = row["args"]
    Hh, heads = a["H"], a["heads"]
    d = Hh // heads
    x = qkv.copy()
    if bf16:
        x[:, :, :Hh] = O.round_bf16(x[:, :, :Hh] * np.float32(d ** -0.5)) * np.float32(d ** 0.5)     # (d = 64: the scale is a power of two)
        x[:, :, Hh:] = O.round_bf16(x[:, :, Hh:])
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(row["op"] == "attention_bwd")
    ctx = torch.zeros((a["B"], a["T"], Hh), dtype=torch.float64)
    parts = []
    for b, f0, nf in segments(row):
        q, k, v = [xt[b, f0:f0 + nf, i * Hh:(i + 1) * Hh].reshape(nf, heads, d).transpose(0, 1) for i in range(3)]
        parts.append((b, f0, nf, (torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2), -1) @ v).transpose(0, 1).reshape(nf, Hh)))
    if row["op"] != "attention_bwd":
        for b, f0, nf, c in parts:
            ctx[b, f0:f0 + nf] = c.detach()
        return ctx.numpy()
    g = torch.from_numpy((np.random.default_rng(5).random((a["B"], a["T"], Hh), dtype=np.float32) * 2 - 1).astype(np.float64))
    sum((c * g[b, f0:f0 + nf]).sum() for b, f0, nf, c in parts).backward()
    return xt.grad.numpy()


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


def launches(lib):
    c = (C.c_int64 * len(KERNELS))()
    N.check(lib.w2v2_op_attention_launches(c))
    return list(c)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row_reaches_the_recorded_kernel_within_its_family_bound(env, row):
    lib, torch, dev = env
    assert row["recorded"], "a row with an op carries what the commit before the route launched for it"
    qkv = qkv_of(row)
    start = {"c": launches(lib)}
    rc, out = run_row(lib, torch, dev, row, qkv, between=lambda: start.update(c=launches(lib)))
    rose = [b - a for a, b in zip(start["c"], launches(lib))]
    if row["refusal"]:
        assert rc != 0 and N.last_error() == row["recorded"] and not any(rose)
        return
    assert rc == 0, N.last_error()
    assert rose == [int(k == row["kernel"]) for k in KERNELS]
    bf16 = row["family"] == "bf16"
    got, ref = out.cpu().numpy().astype(np.float64), reference(torch, row, qkv, bf16)
    rows_of = np.zeros(got.shape[:2], bool)      # a packed op writes the utterances' rows only
    for b, f0, nf in segments(row):
        rows_of[b, f0:f0 + nf] = True
    assert np.isfinite(got[rows_of]).all()
    err = np.abs(got - ref)[rows_of]
    print(f"{row['name']}: max err {err.max():.3e}, mean err {err.mean():.3e}")
    if row["op"] == "attention_bwd":
        Hh = row["args"]["H"]
        for name, sl in (("dq", slice(0, Hh)), ("dk", slice(Hh, 2 * Hh)), ("dv", slice(2 * Hh, 3 * Hh))):
            e, scale = np.abs(got[:, :, sl] - ref[:, :, sl]), max(1.0, np.abs(ref[:, :, sl]).max())
            assert (e.max() < 1e-2 * scale and e.mean() < 1e-3 * scale) if bf16 else e.max() < 5e-5 * scale, f"{name}: {e.max():.3e}"
    elif bf16:
        assert err.max() < 2e-2 and err.mean() < 2e-3
    else:
        assert err.max() < 2e-5
