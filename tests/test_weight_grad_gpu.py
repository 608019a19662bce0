"""One weight gradient per form of csrc/weight_grad_plan.h, run through w2v2_op_weight_grad at the smallest shapes that reach the form.

The operands are small integers (exact in bf16) and every partial sum stays below 2^24, so any kernel, slab order and fold gives the
exact integer dW = X^T dY and db = column sums of dY: the comparison is torch.equal against the int64 results, no tolerance.  The
memory behind the operands holds NaN patterns (except the promised zero row behind dY16) and every output and scratch is pre-filled
with NaN, so a row counted twice, a row dropped or a slab started at the wrong place changes an integer or leaves a NaN."""

import ctypes as C

import pytest

from wav2vec2 import _native as N
from test_weight_grad_plan_cpu import FIELDS, plan, problem

NAN16 = 0x7FC0
PAD_ROWS = 192      # NaN rows behind every operand: more than the rows a kernel's last K tiles reach past M
# name, precision, Kin, Nout, M, operands (A, dY, A16, dY16, zero row), the plan the case must reach
CASES = [
    ("uneven", 1, 128, 256, 419, (0, 1, 1, 1, 1), dict(form="uneven_128x256", S=2, Kp=192, kextra=1, validK=419, tail=None, bias="pass")),
    ("ragged_128x128", 1, 128, 128, 419, (0, 1, 1, 1, 1), dict(form="ragged_128x128", S=7, Kp=64, validK=419, tail=None, bias="pass")),
    ("divisor_shadows_shadow_tail", 1, 128, 128, 2368, (0, 1, 1, 1, 1), dict(form="div_shadows", S=18, Kp=128, R=64, tail="shadow", nslabs=19, bias="pass")),
    ("bf16_from_fp32_fused_bias_guarded_tail", 1, 128, 132, 1190, (1, 1, 0, 0, 0), dict(form="div_f32_reg", S=18, Kp=64, R=38, tail="copy", bias="fused")),
    ("fp32", 0, 96, 64, 1190, (1, 1, 0, 0, 0), dict(form="div_f32_copy", S=18, Kp=64, R=38, tail="copy", bias="pass")),
]


@pytest.fixture(scope="module")
def env():
    import torch
    torch.cuda.set_device(0)
    return N.load(), torch, torch.device("cuda:0")


def padded(torch, dev, t, dtype, zero_row=False):
    """t (rows, cols) followed by PAD_ROWS rows of NaN (the first of them zeros if promised), as `dtype`"""
    rows, cols = t.shape
    if dtype == torch.bfloat16:
        buf = torch.full((rows + PAD_ROWS, cols), NAN16, device=dev, dtype=torch.int16)
        buf[:rows] = t.to(torch.bfloat16).view(torch.int16)
    else:
        buf = torch.full((rows + PAD_ROWS, cols), float("nan"), device=dev)
        buf[:rows] = t.float()
    if zero_row:
        buf[rows] = 0
    assert buf.data_ptr() % 16 == 0
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_each_form_gives_the_exact_integer_gradient(env, case):
    lib, torch, dev = env
    name, precision, Kin, Nout, M, (hasA, hasdY, hasA16, hasdY16, zero_row), want = case
    r = torch.arange(M, device=dev, dtype=torch.int64)[:, None]
    X = (7 * r + 3 * torch.arange(Kin, device=dev)[None, :]) % 5 - 2
    dY = (11 * r + 5 * torch.arange(Nout, device=dev)[None, :]) % 3 - 1
    ref_dW, ref_db = (X.double().t() @ dY.double()).long(), dY.sum(0)      # (int64; the fp64 product holds these integers exactly: |sum| <= 2 M)
    assert 0 < int(ref_dW.abs().max()) <= 2 * M < 2 ** 24

    elems = Kin * Nout
    q = problem(M, Kin, Nout, precision, hasA, hasdY, hasA16, hasdY16, zero_row, dW=1, db=1, shared=34 * elems, cs=34 * Nout)
    p = plan(q)
    assert p["refusal"] is None and {k: p[k] for k in want} == want, p      # the case reaches the form it names
    assert p["S"] * p["Kp"] + 64 * p["kextra"] <= M + PAD_ROWS

    nan = float("nan")
    A = padded(torch, dev, X, torch.float32) if hasA else None
    dYf = padded(torch, dev, dY, torch.float32) if hasdY else None
    A16 = padded(torch, dev, X, torch.bfloat16) if hasA16 else None
    dY16 = padded(torch, dev, dY, torch.bfloat16, zero_row=bool(zero_row)) if hasdY16 else None
    dW, db = torch.full((Kin, Nout), nan, device=dev), torch.full((Nout,), nan, device=dev)
    slabs = torch.full((q["shared_slab_floats"],), nan, device=dev)
    at = torch.full((Kin * M,), nan, device=dev)
    cs_ws = torch.full((q["cs_floats"],), nan, device=dev)
    red_ws = torch.full(((M + 127) // 128 * Nout + 8,), nan, device=dev)
    N.check(lib.w2v2_op_set_precision(precision))
    try:
        rc = lib.w2v2_op_weight_grad((C.c_int64 * len(FIELDS))(*[int(q[f]) for f in FIELDS]), N.ptr(A), N.ptr(dYf), N.ptr(A16), N.ptr(dY16), N.ptr(dW), N.ptr(db),
                                     N.ptr(slabs), N.ptr(at), at.numel(), N.ptr(cs_ws), N.ptr(red_ws), red_ws.numel(), N.current_stream())
        torch.cuda.synchronize()
    finally:
        N.check(lib.w2v2_op_set_precision(0))
    assert rc == 0, N.last_error()
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    assert torch.equal(dW.double(), ref_dW.double()), int((dW.double() != ref_dW.double()).sum())
    assert torch.equal(db.double(), ref_db.double()), int((db.double() != ref_db.double()).sum())


@pytest.mark.gpu
def test_the_op_refuses_what_it_cannot_run(env):
    lib, torch, dev = env
    q = problem(419, 128, 256, 1, 0, 0, 1, 1, 1, shared=34 * 128 * 256)
    x16 = torch.zeros((420 + PAD_ROWS, 256), device=dev, dtype=torch.int16)
    dW = torch.zeros((128, 256), device=dev)

    def run(q, slabs=None):
        return lib.w2v2_op_weight_grad((C.c_int64 * len(FIELDS))(*[int(q[f]) for f in FIELDS]), None, None, N.ptr(x16), N.ptr(x16), N.ptr(dW), None, N.ptr(slabs),
                                       None, 0, None, None, 0, N.current_stream())

    # (the thread's precision is fp32 here: the problem says bf16)
    assert run(q) != 0 and "precision" in N.last_error()
    assert run(dict(q, precision=0, A=1)) != 0 and "flags disagree" in N.last_error()
    assert run(dict(q, precision=0)) != 0 and N.last_error() == "weight_grad: the fp32 operands are needed here (no bf16 shadows / shapes not whole 128-tiles)"
    N.check(lib.w2v2_op_set_precision(1))
    try:
        assert run(q) != 0 and N.last_error() == "op_weight_grad: this plan writes slabs"
    finally:
        N.check(lib.w2v2_op_set_precision(0))
    torch.cuda.synchronize()
