"""Every recorded row of tests/golden/gemm_bf16_routes.json run once on the GPU through the op it names: the launch counter of the
recorded kernel (w2v2_op_gemm_bf16_launches) rises by one and no other moves, and the output equals a fixed reference kernel's bit
for bit -- forward rows the guarded fp32 kernel's (w2v2_op_gemm_bf16 with A 4 bytes off a 16-byte boundary), weight-gradient rows
w2v2_op_gemm_bf16_at's, transposed-fp32 rows the guarded kernel's on a transposed copy; all on fp32 operands that hold exactly the
shadows' bf16 values.  A refused row returns the recorded message and launches nothing.

run_row and reference use only ops older than the router (tools/gemm_bf16_route_record.py runs them on the commit before it)."""

import ctypes as C
import json
import os

import pytest

from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bf16_routes.json")
ROWS = [r for r in json.load(open(GOLDEN)) if r["op"] is not None]
KERNELS = [None, "f32_guarded", "f32_vec", "a_shadow", "b_shadow", "dma_128x128", "dma_128x64", "at_f32_128x128", "at_f32_128x64", "tr_128x128",
           "sw_128x256", "swtr_128x256"]
NAN16 = 0x7FC0


def values(torch, dev, n, seed, scale=1.0):
    """n bf16-exact values"""
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(n, generator=g, device=dev) * scale).bfloat16()


def off16(torch, t):
    """a copy of the flat fp32 tensor t that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:] = t.reshape(-1)
    assert buf.data_ptr() % 16 == 0
    return buf[1:]


def operands(torch, dev, row):
    """The row's operands as bf16 values: forward (A flat with the row's strides, B (K, N), bias), weight gradient (X, dY by rows)."""
    a = row["args"]
    if row["op"] in ("gemm_bf16", "gemm_bf16_shadows"):
        na = (a["nbatch"] - 1) * a["strideA"] + (a["M"] - 1) * a["lda"] + a["K"]
        return dict(A=values(torch, dev, na, 1), B=values(torch, dev, a["K"] * a["N"], 2, 0.2).view(a["K"], a["N"]),
                    bias=values(torch, dev, a["N"], 3).float() if a["bias"] else None)
    if row["op"] == "gemm_bf16_at":
        return dict(X=values(torch, dev, a["nbatch"] * a["K"] * a["M"], 1).view(-1, a["M"]), dY=values(torch, dev, a["nbatch"] * a["K"] * a["N"], 2, 0.3).view(-1, a["N"]))
    return dict(X=values(torch, dev, a["rows"] * a["Kin"], 1).view(-1, a["Kin"]), dY=values(torch, dev, a["rows"] * a["Nout"], 2, 0.3).view(-1, a["Nout"]))


def guarded(lib, torch, A, lda, strideA, B, bias, M, N_, K, nbatch, act):
    """C = act(A B + bias) on the guarded fp32 kernel: A (flat fp32) is moved 4 bytes off a 16-byte boundary"""
    out, buf = torch.full((nbatch, M, N_), float("nan"), device=A.device), off16(torch, A)
    N.check(lib.w2v2_op_gemm_bf16(N.ptr(buf), lda, strideA, N.ptr(B), N_, N.ptr(out), N_, M * N_, N.ptr(bias), None, M, N_, K, nbatch, act,
                                  N.current_stream()), "w2v2_op_gemm_bf16")
    return out


def slab_rows(a):
    """weight_grad_bf16: (first row, rows) of every slab"""
    units = (a["rows"] + 63) // 64
    e = units - (a["per"] // 64) * a["S"] if a["variant"] in (2, 3) else 0
    out, start = [], 0
    for z in range(a["S"]):
        n = a["per"] + (64 if z < e else 0)
        out.append((start, max(0, min(n, a["rows"] - start))))
        start += n
    return out


def run_row(lib, torch, dev, row, ops):
    """(return code, output) of the row's own call"""
    a, s = row["args"], N.current_stream()
    if row["op"] == "gemm_bf16":
        A, B = ops["A"].float(), ops["B"].float()
        buf = off16(torch, A) if a["a_off"] else A
        out = torch.full((a["nbatch"], a["M"], a["N"]), float("nan"), device=dev)
        rc = lib.w2v2_op_gemm_bf16(N.ptr(buf), a["lda"], a["strideA"], N.ptr(B), a["N"], N.ptr(out), a["N"], a["M"] * a["N"], N.ptr(ops["bias"]),
                                   None, a["M"], a["N"], a["K"], a["nbatch"], a["act"], s)
    elif row["op"] == "gemm_bf16_shadows":
        B16 = ops["B"].t().contiguous()      # (N, K): the weight shadow's layout
        out = torch.full((a["nbatch"], a["M"], a["N"]), float("nan"), device=dev)
        rc = lib.w2v2_op_gemm_bf16_shadows(N.ptr(ops["A"]), a["lda"], a["strideA"], N.ptr(B16), N.ptr(out), None, a["N"], a["M"] * a["N"], N.ptr(ops["bias"]), None,
                                           a["M"], a["N"], a["K"], a["nbatch"], a["act"], a["variant"], s)
    elif row["op"] == "gemm_bf16_at":
        X, dY = ops["X"].float(), ops["dY"].float()
        out = torch.full((a["nbatch"], a["M"], a["N"]), float("nan"), device=dev)
        rc = lib.w2v2_op_gemm_bf16_at(N.ptr(X), a["M"], a["K"] * a["M"], N.ptr(dY), a["N"], a["K"] * a["N"], N.ptr(out), a["N"],
                                      a["M"] * a["N"], a["M"], a["N"], a["K"], a["nbatch"], s)
    else:
        # rows behind the last one: x16 holds a large finite value (the ragged form re-reads A's last row against B's zero row), dy16 the
        # promised zero row, then NaN
        alloc = max(a["rows"], a["per"] * a["S"]) + 1
        x16 = torch.full((a["x_off"] + alloc * a["Kin"],), 1000.0, device=dev).bfloat16()
        x16[a["x_off"]:a["x_off"] + a["rows"] * a["Kin"]] = ops["X"].reshape(-1)
        y16 = torch.full((alloc, a["Nout"]), NAN16, device=dev, dtype=torch.int16)
        y16[:a["rows"]] = ops["dY"].view(torch.int16)
        y16[a["rows"]] = 0
        out = torch.full((a["S"], a["Kin"], a["Nout"]), float("nan"), device=dev)
        rc = lib.w2v2_op_weight_grad_bf16(N.ptr(x16[a["x_off"]:]), N.ptr(y16), N.ptr(out), a["rows"], a["Kin"], a["Nout"], a["per"], a["S"], a["variant"], s)
    torch.cuda.synchronize()
    return rc, out


def reference(lib, torch, dev, row, ops):
    a = row["args"]
    if row["op"] in ("gemm_bf16", "gemm_bf16_shadows"):
        out = guarded(lib, torch, ops["A"].float(), a["lda"], a["strideA"], ops["B"].float(), ops["bias"], a["M"], a["N"], a["K"], a["nbatch"], a["act"])
    elif row["op"] == "gemm_bf16_at":
        X, dY, K = ops["X"].float(), ops["dY"].float(), a["K"]
        out = torch.cat([guarded(lib, torch, X[z * K:(z + 1) * K].t().contiguous(), K, 0, dY[z * K:(z + 1) * K].contiguous(), None, a["M"], a["N"], K, 1, 0)
                         for z in range(a["nbatch"])])
    else:
        outs = []
        for start, n in slab_rows(a):      # one slab per call, its rows padded with zeros to whole K tiles
            K = (n + 63) // 64 * 64
            X, dY = torch.zeros((K, a["Kin"]), device=dev), torch.zeros((K, a["Nout"]), device=dev)
            X[:n], dY[:n] = ops["X"][start:start + n].float(), ops["dY"][start:start + n].float()
            o = torch.full((1, a["Kin"], a["Nout"]), float("nan"), device=dev)
            N.check(lib.w2v2_op_gemm_bf16_at(N.ptr(X), a["Kin"], 0, N.ptr(dY), a["Nout"], 0, N.ptr(o), a["Nout"], 0, a["Kin"], a["Nout"], K, 1, N.current_stream()),
                    "w2v2_op_gemm_bf16_at")
            outs.append(o)
        out = torch.cat(outs)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


def launches(lib):
    c = (C.c_int64 * len(KERNELS))()
    N.check(lib.w2v2_op_gemm_bf16_launches(c))
    return list(c)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row_reaches_the_recorded_kernel_with_the_reference_bits(env, row):
    lib, torch, dev = env
    assert row["recorded"], "a row with an op carries what the commit before the router launched for it"
    ops = operands(torch, dev, row)
    before = launches(lib)
    rc, out = run_row(lib, torch, dev, row, ops)
    rose = [b - a for a, b in zip(before, launches(lib))]
    if row["refusal"]:
        assert rc != 0 and N.last_error() == row["recorded"] and not any(rose)
        return
    assert rc == 0, N.last_error()
    assert rose == [int(k == row["kernel"]) for k in KERNELS]
    ref = reference(lib, torch, dev, row, ops)
    assert torch.isfinite(ref).all()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
