"""How the training step cuts a weight gradient into slabs (csrc/weight_grad_plan.h through w2v2_op_weight_grad_plan: host only, no GPU).

tests/golden/weight_grad_plans.json holds one row per form and per boundary of a rule: the problem, and what the commit BEFORE the plan
became a pure function did with it.  "recorded" rows carry the weight-gradient kernel's name and grid z (= S) from a kernel trace of
that commit's backward with one site trainable (tools/weight_grad_plan_record.py); "derived" rows name the lines of that commit's
weight_grad their expectation was read from.  The sweep below holds the properties any plan must have, over every shape the models and
the benchmark can pose; tests/test_weight_grad_gpu.py runs one plan per form."""

import ctypes as C
import json
import os

import pytest

from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_grad_plans.json")
ROWS = json.load(open(GOLDEN))
FIELDS = ["M", "Kin", "Nout", "precision", "A", "dY", "A16", "dY16", "dy16_zero_row", "want_dW", "want_db", "unpack", "shared_slab_floats",
          "site_slab_floats", "cs_floats", "dw_blocks", "dw_uneven"]
OUT = ["refusal", "form", "kernel", "kq", "cap", "S", "Kp", "kextra", "validK", "b_zero_row", "Mq", "R", "tail", "nslabs", "dst", "fold", "bias", "max_slabs"]
REFUSALS = [None, "fp32_operands", "slab_scratch", "bias_needs_dy"]
FORMS = ["bias_only", "uneven_128x256", "ragged_128x128", "div_shadows", "div_f32_reg", "div_f32_copy"]
TAILS = [None, "shadow", "copy"]
DSTS = [None, "dW", "slabs"]
BIAS = [None, "fused", "pass"]
KERNELS = [None, "f32_guarded", "f32_vec", "a_shadow", "b_shadow", "dma_128x128", "dma_128x64", "at_f32_128x128", "at_f32_128x64", "tr_128x128",
           "sw_128x256", "swtr_128x256"]      # as w2v2_op_gemm_bf16_route numbers them
NAMES = dict(refusal=REFUSALS, form=FORMS, kernel=KERNELS, tail=TAILS, dst=DSTS, bias=BIAS)
ROUTE_FIELDS = ["M", "N", "K", "nbatch", "lda", "ldb", "strideA", "strideB", "ldb16", "A", "B", "A16", "B16", "B16p", "C", "C16", "transA", "zmod", "colsum",
                "overlapA", "validK", "kextra", "b_zero_row", "force_kernel"]
ABSENT, ALIGNED = 0, 2


def plan(q):
    out = (C.c_int64 * len(OUT))()
    N.check(N.load().w2v2_op_weight_grad_plan((C.c_int64 * len(FIELDS))(*[int(q[f]) for f in FIELDS]), out), "w2v2_op_weight_grad_plan")
    return {k: (NAMES[k][v] if k in NAMES else v) for k, v in zip(OUT, out)}


def problem(M, Kin, Nout, precision=1, A=0, dY=0, A16=0, dY16=0, zero_row=0, dW=1, db=0, unpack=0, shared=0, site=0, cs=None, blocks=512, uneven=1):
    return dict(M=M, Kin=Kin, Nout=Nout, precision=precision, A=A, dY=dY, A16=A16, dY16=dY16, dy16_zero_row=zero_row, want_dW=dW, want_db=db, unpack=unpack,
                shared_slab_floats=shared, site_slab_floats=site, cs_floats=34 * max(Kin, Nout) if cs is None else cs, dw_blocks=blocks, dw_uneven=uneven)


def slab_rows(q, p):
    """(first row, rows) of every slab and of the tail, as the kernels the plan names read them"""
    out, start = [], 0
    for z in range(p["S"]):
        n = p["Kp"] + (64 if z < p["kextra"] else 0)
        out.append((start, min(n, p["Mq"] - start)))
        start += n
    if p["R"]:
        out.append((p["Mq"], p["R"]))
    return out


def gemm_route(q, p):
    """what gemm_bf16_route says to the slab GEMM the plan implies (16-byte aligned operands)"""
    shadows = p["form"] in ("uneven_128x256", "ragged_128x128", "div_shadows")
    g = dict(M=q["Kin"], N=q["Nout"], K=p["Kp"], nbatch=p["S"], lda=q["Kin"], ldb=q["Nout"], strideA=p["Kp"] * q["Kin"], strideB=p["Kp"] * q["Nout"], ldb16=0,
             A=ALIGNED if q["A"] else ABSENT, B=ALIGNED if q["dY"] else ABSENT, A16=ALIGNED if shadows else ABSENT, B16=ABSENT, B16p=ALIGNED if shadows else ABSENT,
             C=1, C16=0, transA=1, zmod=0, colsum=int(p["bias"] == "fused"), overlapA=0, validK=p["validK"], kextra=p["kextra"], b_zero_row=p["b_zero_row"],
             force_kernel=0)
    out = (C.c_int32 * 5)()
    N.check(N.load().w2v2_op_gemm_bf16_route((C.c_int64 * len(ROUTE_FIELDS))(*[int(g[f]) for f in ROUTE_FIELDS]), out), "w2v2_op_gemm_bf16_route")
    return dict(kernel=KERNELS[out[0]], krag=out[1], refused=out[2] != 0)


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_plan_matches_the_table(row):
    p = plan(row["problem"])
    assert {k: p[k] for k in row["plan"]} == row["plan"], p
    if row["recorded"] is None:
        assert row["derived"], "a row without a recording says which lines its expectation was read from"
    else:      # the weight-gradient kernel of the trace and its grid z
        assert row["recorded"]["grid_z"] == p["S"]
        want = {"swtr_128x256": "gemm_bf16_sw_kernel<false, true, 0, true>", "tr_128x128": "gemm_bf16_tr_kernel<2, 4, 2>",
                "at_f32_128x128": "gemm_bf16_kernel<7, 128, 128, 2, 2, 2>", "at_f32_128x64": "gemm_bf16_kernel<7, 128, 64, 2, 2, 2>"}[p["kernel"]]
        assert row["recorded"]["kernel"].replace("w2v2::", "").startswith(want)


def test_table_reaches_every_form_tail_and_refusal():
    plans = [plan(r["problem"]) for r in ROWS]
    assert {p["refusal"] for p in plans} == set(REFUSALS)
    ok = [p for p in plans if p["refusal"] is None]
    assert {p["form"] for p in ok} == set(FORMS) and {p["bias"] for p in ok} == set(BIAS) and {p["dst"] for p in ok} == set(DSTS)
    # the eight (form, tail) launch sequences that exist
    assert {(p["form"], p["tail"]) for p in ok if p["form"] != "bias_only"} == {
        ("uneven_128x256", None), ("ragged_128x128", None), ("div_shadows", None), ("div_shadows", "shadow"), ("div_f32_reg", None), ("div_f32_reg", "copy"),
        ("div_f32_copy", None), ("div_f32_copy", "copy")}


def test_benchmark_shapes():
    for name, S, Kp, kextra in (("bench_base_ffn_up", 7, 3456, 6), ("bench_large_ffn_up", 4, 5952, 3), ("fingerprint_225", 1, 256, 0),
                                ("fingerprint_675", 3, 192, 2)):
        p = plan(by_name(name)["problem"])
        assert (p["form"], p["S"], p["Kp"], p["kextra"]) == ("uneven_128x256", S, Kp, kextra), name


def test_boundaries_flip_where_the_table_says():
    un = by_name("uneven_419_zero_row")["problem"]
    # three K tiles per slab (the last may be short): 2 units -> the divisor rule or the ragged form, 3 -> one uneven slab, 6 -> two
    assert [plan(dict(un, M=m))["form"] for m in (64, 65, 128, 129, 192)] == ["div_shadows", "ragged_128x128", "div_shadows", "uneven_128x256", "uneven_128x256"]
    assert [plan(dict(un, M=m))["S"] for m in (129, 320, 321, 384)] == [1, 1, 2, 2]
    assert plan(dict(un, dy16_zero_row=0))["form"] == "ragged_128x128" and plan(dict(un, dw_uneven=0))["form"] == "ragged_128x128"
    assert plan(dict(un, Nout=128))["form"] == "ragged_128x128" and plan(dict(un, Kin=64, A=1, dY=1))["form"] == "div_f32_reg"
    # cap from the block slots: 72 wide tiles x 7 = 504 <= 512 < 72 x 8; from the scratch: cap + 2 slabs of the shared one, cap + 1 of a site's
    base = by_name("bench_base_ffn_up")["problem"]
    assert [plan(dict(base, dw_blocks=b))["cap"] for b in (503, 504, 575, 576)] == [6, 7, 7, 8]
    e = base["Kin"] * base["Nout"]
    assert [plan(dict(base, shared_slab_floats=n * e))["cap"] for n in (9, 8, 8 - 1)] == [7, 6, 5]
    assert [plan(dict(base, site_slab_floats=n * e + 1))["cap"] for n in (8, 7, 6)] == [7, 6, 5]
    # the divisor rule: a prime unit count gives one unit away; 2 d >= cap stops the search
    dv = by_name("div_shadows_2368")["problem"]
    assert [(plan(dict(dv, M=64 * u))["S"], plan(dict(dv, M=64 * u))["R"]) for u in (36, 37, 38, 41)] == [(18, 0), (18, 64), (19, 0), (20, 64)]
    # the fused bias needs nslabs + 1 rows of column sums
    fb = by_name("div_f32_reg_1190_fused")["problem"]
    assert [plan(dict(fb, cs_floats=n * fb["Nout"]))["bias"] for n in (20, 19)] == ["fused", "pass"]


def test_scratch_sizes_follow_the_plan():
    """wg_max_slabs (out[17]) is what the training step sizes a site's scratch with: the sizes in bytes are the ones it always had."""
    for (Kin, Nout), want in (((3072, 768), 16), ((768, 768), 33), ((768, 2304), 20), ((4096, 1024), 9), ((1024, 1024), 33), ((128, 64), 33)):
        assert plan(problem(64, Kin, Nout, A=1, dY=1, shared=33 * Kin * Nout))["max_slabs"] == want == min(32, -(-2048 * 128 * 128 // (Kin * Nout))) + 1


DIMS = [(64, 128, 32), (768, 3072, 512), (1024, 4096, 512), (100, 300, 512), (132, 516, 36), (640, 2560, 512)]      # H, F, last conv width
ROWS_M = list(range(1, 1400)) + [2053, 23984, 24576]
# (precision, A, dY, A16, dY16, zero row): what the call sites pass -- fp32 and bf16x3 take fp32 operands; mode bf16 takes them, or both
# shadows (with the zero row behind the step's own dY shadows, and without), or shadows beside the fp32 tensors
OPERANDS = [(0, 1, 1, 0, 0, 0), (2, 1, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0), (1, 0, 0, 1, 1, 1), (1, 0, 0, 1, 1, 0), (1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 0, 0)]


def check_plan(q, p, routes):
    M, Kin, Nout, e = q["M"], q["Kin"], q["Nout"], q["Kin"] * q["Nout"]
    tag = (q, p)
    if not (q["A"] and q["dY"]) and (q["precision"] != 1 or Kin % 128 or Nout % 128):      # shadows alone serve whole 128-tiles in mode bf16 only
        assert p["refusal"] == "fp32_operands", tag
        return
    assert p["refusal"] is None, tag
    rows = slab_rows(q, p)
    assert len(rows) == p["nslabs"] and all(n > 0 for _, n in rows), tag                               # no slab is empty
    assert rows[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(rows, rows[1:])) and rows[-1][0] + rows[-1][1] == M, tag      # [0, M) exactly once
    assert p["Kp"] % p["kq"] == 0 and p["Mq"] + p["R"] == M and p["S"] <= p["cap"] <= 32, tag
    if p["form"] == "uneven_128x256":      # only the last K tile of the last slab may be short, and then the zero row stands behind it
        span = p["S"] * p["Kp"] + 64 * p["kextra"]
        assert 0 <= span - M < 64 and p["b_zero_row"] == (span != M) and (not p["b_zero_row"] or q["dy16_zero_row"]) and p["kextra"] < p["S"], tag
        assert p["validK"] == (M if span != M else 0) and p["Kp"] >= 192 and Kin % 128 == 0 and Nout % 256 == 0, tag
    if p["form"] == "ragged_128x128":
        assert p["validK"] == M and 0 < p["S"] * p["Kp"] - M < p["Kp"], tag
    assert p["fold"] == (p["nslabs"] > 1 or bool(q["unpack"])) and p["dst"] == ("slabs" if p["fold"] else "dW"), tag
    if p["fold"]:
        assert (p["nslabs"] + 1) * e <= (q["site_slab_floats"] or q["shared_slab_floats"]), tag
    assert p["nslabs"] <= p["max_slabs"], tag
    assert (p["kernel"] is not None) == (p["S"] > 0 and p["form"] != "div_f32_copy"), tag
    if p["kernel"]:
        key = (Kin, Nout, p["Kp"], p["S"], p["kextra"], p["validK"], p["b_zero_row"], p["bias"] == "fused", q["A"], q["dY"], p["form"])
        if key not in routes:
            routes[key] = gemm_route(q, p)
        rt = routes[key]
        assert not rt["refused"] and rt["kernel"] == p["kernel"], (tag, rt)
        assert rt["krag"] == (M % 64 if p["b_zero_row"] else 0), (tag, rt)


def test_every_shape_of_the_models_gets_a_sound_plan():
    routes, seen = {}, set()
    for H, F, Cw in DIMS:
        shared = 33 * max(F * H, 3 * H * H)
        sites = [(F, H, True), (H, F, True), (H, H, True), (H, 3 * H, True), (H, 32, False), (Cw, H, False)]
        for Kin, Nout, layer_site in sites:
            own = plan(problem(64, Kin, Nout, A=1, dY=1, shared=shared))["max_slabs"] + 1
            for site in ((0, own * Kin * Nout) if layer_site else (0,)):
                for prec, A, dY, A16, dY16, zr in OPERANDS:
                    for M in ROWS_M:
                        q = problem(M, Kin, Nout, prec, A, dY, A16, dY16, zr, db=int(bool(dY)), unpack=int(Nout == 3 * H and site != 0), shared=shared, site=site)
                        p = plan(q)
                        check_plan(q, p, routes)
                        if p["refusal"] is None:
                            seen.add((p["form"], p["tail"]))
    assert len(seen) == 8 and ("div_shadows", "shadow") in seen, seen      # (640, 2560) reaches the shadow tail: Nout % 256 != 0 on the divisor rule
