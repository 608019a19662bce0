"""Which kernels an fp32 GEMM reaches (csrc/gemm_f32_route.h through w2v2_op_gemm_f32_route: host only, no GPU).

tests/golden/gemm_f32_routes.json holds, per shape, the launch counters RECORDED on the GPU on the commit before the router
became a pure function: the increase of the four ring counters (w2v2_op_gemm_ring_launches) and of the gemm family's kernel-launch
counter.  The route of every row must imply exactly those.  Five counters do not tell the double-buffered instances apart, nor
reach the per-batch-B form (strideB != 0, not callable through w2v2_op_gemm): rows marked "derived" also carry the kernel names, read
from that commit's code, not recorded."""

import ctypes as C
import json
import os

import pytest

from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_f32_routes.json")
ROWS = json.load(open(GOLDEN))
KERNELS = [None, "ring_256x128", "ring_128x128", "ring_64x64", "ring_64x64_quarters", "db_256x128x16", "db_128x128x32", "db_64x64x32",
           "staged_128x128"]
ONE, SPLIT_K, ORDER_SPLIT, ROW_SPLIT = range(4)


def route(row, ab_aligned=1, c_aligned=1, **over):
    r = dict(row, **over)
    out = (C.c_int32 * 8)()
    N.check(N.load().w2v2_op_gemm_f32_route(r["M"], r["N"], r["K"], r["nbatch"], r["lda"], r["ldb"], r["ldc"], r["strideA"], r["strideB"], r["act"],
                                           int(r["bias"]), int(r["residual"]), ab_aligned, c_aligned, r["variant"], out), "w2v2_op_gemm_f32_route")
    kind, k0, k1, S, main_tiles, main_rows, persist, launches = out
    return dict(kind=kind, kernels=[KERNELS[k] for k in (k0, k1) if k], S=S, main_tiles=main_tiles, main_rows=main_rows, persist=persist,
                launches=launches)


def implied(rt):
    """(ring counter increases, kernel launches) a route stands for: each ring kernel adds 1 to its counter; one launch, or two for
    either split, or the split-K GEMM plus its fold."""
    ring = [0, 0, 0, 0]
    for k in rt["kernels"]:
        if k.startswith("ring"):
            ring[KERNELS.index(k) - 1] += 1
    assert len(rt["kernels"]) == (1 if rt["kind"] in (ONE, SPLIT_K) else 2)
    return ring, 1 if rt["kind"] == ONE else 2


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_route_matches_the_recorded_launches(row):
    rt = route(row)
    ring, launches = implied(rt)
    assert launches == rt["launches"]
    if row["recorded"] is not None:
        assert (ring, launches) == (row["recorded"]["ring"], row["recorded"]["launches"]), rt
    else:
        assert row["derived"], "a row without a recording must say where its expectation comes from"
    if row["derived"]:
        assert rt["kernels"] == row["kernels"], rt
    # by shape, and as variant 2, the ring kernels run the persistent grid; variant 1 one tile per block; no ring kernel, no flag
    assert rt["persist"] == int(any(k.startswith("ring") for k in rt["kernels"]) and row["variant"] in (-1, 2))


def test_table_reaches_every_kernel_and_kind():
    seen, kinds = set(), set()
    for row in ROWS:
        rt = route(row)
        seen.update(rt["kernels"])
        kinds.add(rt["kind"])
    assert seen == set(KERNELS[1:]) and kinds == {ONE, SPLIT_K, ORDER_SPLIT, ROW_SPLIT}


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


def test_split_parameters():
    assert route(by_name("splitk_s4"))["S"] == 4 and route(by_name("splitk_s2_upper_bound"))["S"] == 2
    assert route(by_name("above_splitk_bound"))["kind"] == ONE
    rt = route(by_name("order_split"))
    assert (rt["kind"], rt["main_tiles"], rt["kernels"]) == (ORDER_SPLIT, 512, ["ring_128x128", "ring_64x64_quarters"])
    rt = route(by_name("tail_quarter_full_exactly"))
    assert (rt["kind"], rt["main_tiles"]) == (ORDER_SPLIT, 1024)
    rt = route(by_name("row_split"))
    assert (rt["kind"], rt["main_rows"], rt["kernels"]) == (ROW_SPLIT, 8192, ["ring_128x128", "ring_64x64"])
    for name in ("tail_just_over_a_quarter", "half_full_last_round", "one_below_wide", "wide_refused_by_padding", "ring128_384_tiles"):
        assert route(by_name(name))["kernels"] == ["ring_128x128"], name
    assert route(by_name("wide"))["kernels"] == ["ring_256x128"]
    assert route(by_name("small_383_tiles"))["kernels"] == ["ring_64x64"]


def test_alignment_facts():
    """A or B off 16 bytes: the register-staged kernel, whatever the shape.  C, bias or residual off 16 bytes: no split-K (the fold
    stores 16 bytes at a time); the problem then counts as small."""
    for row in ROWS:
        assert route(row, ab_aligned=0)["kernels"] == ["staged_128x128"]
    rt = route(by_name("splitk_s4"), c_aligned=0)
    assert (rt["kind"], rt["kernels"]) == (ONE, ["ring_64x64"])
    assert route(by_name("splitk_s4"), ldc=66)["kind"] == ONE


def test_per_batch_b_never_takes_a_ring_kernel():
    for row in ROWS:
        if row["nbatch"] == 1:
            continue
        rt = route(row, strideB=row["K"] * row["ldb"])
        assert not any(k.startswith("ring") for k in rt["kernels"]), (row["name"], rt)
