"""Which kernel a bf16 GEMM reaches (csrc/gemm_bf16_route.h through w2v2_op_gemm_bf16_route: host only, no GPU).

tests/golden/gemm_bf16_routes.json holds one row per rule of the router and per boundary of a rule: the op call that poses the
problem, the problem as the router sees it, and what the commit BEFORE the router became a pure function did with it -- "recorded" is
the kernel's name in a kernel trace of that commit (tools/gemm_bf16_route_record.py), or the message it refused the call with.  Rows
no op can pose (one shadow only, the positional conv's two-level batch, column sums, overlapping transposed rows) are "derived": they
name the lines of that commit's launch_gemm_bf16_x their expectation was read from.  tests/test_gemm_bf16_route_gpu.py runs the
recorded rows."""

import ctypes as C
import json
import os

import pytest

from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bf16_routes.json")
ROWS = json.load(open(GOLDEN))
FIELDS = ["M", "N", "K", "nbatch", "lda", "ldb", "strideA", "strideB", "ldb16", "A", "B", "A16", "B16", "B16p", "C", "C16", "transA", "zmod", "colsum",
          "overlapA", "validK", "kextra", "b_zero_row", "force_kernel"]
KERNELS = [None, "f32_guarded", "f32_vec", "a_shadow", "b_shadow", "dma_128x128", "dma_128x64", "at_f32_128x128", "at_f32_128x64", "tr_128x128",
           "sw_128x256", "swtr_128x256"]
REFUSALS = [None, "kextra_on_tr", "validk", "kextra_zero_row", "at_f32", "shadow_only"]
# the name each kernel has in a kernel trace (the 128 x 256 kernels: any epilogue form of the forward one, the one transposed instance)
TRACE_NAME = {"f32_guarded": "gemm_bf16_kernel<0, 128, 128, 2, 2, 2>", "f32_vec": "gemm_bf16_kernel<1, 128, 128, 2, 2, 2>",
              "a_shadow": "gemm_bf16_kernel<2, 128, 128, 2, 2, 2>", "b_shadow": "gemm_bf16_kernel<3, 128, 128, 2, 2, 2>",
              "dma_128x128": "gemm_bf16_kernel<5, 128, 128, 2, 4, 2>", "dma_128x64": "gemm_bf16_kernel<5, 128, 64, 2, 2, 2>",
              "at_f32_128x128": "gemm_bf16_kernel<7, 128, 128, 2, 2, 2>", "at_f32_128x64": "gemm_bf16_kernel<7, 128, 64, 2, 2, 2>",
              "tr_128x128": "gemm_bf16_tr_kernel<2, 4, 2>", "sw_128x256": "gemm_bf16_sw_kernel<false, true, ", "swtr_128x256": "gemm_bf16_sw_kernel<false, true, 0, true>"}
ABSENT, PRESENT, ALIGNED = range(3)


def route(row, **over):
    p = dict(row["problem"], **over)
    out = (C.c_int32 * 5)()
    N.check(N.load().w2v2_op_gemm_bf16_route((C.c_int64 * len(FIELDS))(*[int(p[f]) for f in FIELDS]), out), "w2v2_op_gemm_bf16_route")
    return dict(kernel=KERNELS[out[0]], krag=out[1], refusal=REFUSALS[out[2]], a_bytes=out[3], b_bytes=out[4])


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_route_matches_the_table(row):
    rt = route(row)
    assert (rt["kernel"], rt["krag"], rt["refusal"]) == (row["kernel"], row["krag"], row["refusal"]), rt
    assert (rt["kernel"] is None) == (rt["refusal"] is not None)
    if row["recorded"] is None:
        assert row["op"] is None and row["derived"], "a row without a recording says which lines its expectation was read from"
    elif row["refusal"]:
        assert row["recorded"].startswith("gemm_bf16: ")
    else:
        name = row["recorded"].replace("w2v2::", "")
        assert name.startswith(TRACE_NAME[row["kernel"]]) and (row["kernel"] != "sw_128x256" or name.endswith(", false>")), name
    if rt["kernel"]:      # shadows are read as 2 bytes per element, fp32 operands as 4
        a16 = rt["kernel"] in ("a_shadow", "dma_128x128", "dma_128x64", "tr_128x128", "sw_128x256", "swtr_128x256")
        b16 = rt["kernel"] in ("b_shadow", "dma_128x128", "dma_128x64", "tr_128x128", "sw_128x256", "swtr_128x256")
        assert (rt["a_bytes"], rt["b_bytes"]) == (2 if a16 else 4, 2 if b16 else 4)


def test_table_reaches_every_kernel_and_refusal():
    routes = [route(r) for r in ROWS]
    assert {rt["kernel"] for rt in routes} == set(KERNELS) and {rt["refusal"] for rt in routes} == set(REFUSALS)


def test_boundaries_flip_where_the_table_says():
    sw, T = by_name("sw_256_tiles"), 128 * 86
    assert (sw["problem"]["M"], sw["problem"]["N"], sw["problem"]["K"]) == (T, 768, 768)
    # 256 tiles of 128 x 256: M = 128 x 85 + 1 is the 86th tile row
    assert route(sw, M=128 * 85 + 1)["kernel"] == "sw_128x256" and route(sw, M=128 * 85)["kernel"] == "dma_128x128"
    assert by_name("dma_255_tiles")["problem"]["M"] == 128 * 85
    # N K >= 768 x 768 for a single batch; any weight with two batches
    assert route(sw, K=704)["kernel"] == "dma_128x128" and route(sw, K=704, M=T // 2, nbatch=2, strideA=T // 2 * 704)["kernel"] == "sw_128x256"
    assert route(sw, K=704, N=1024)["kernel"] == "sw_128x256"      # 704 x 1024 >= 768 x 768
    # at least three K tiles, whole 256-column tiles
    assert route(sw, K=192, nbatch=2)["kernel"] == "sw_128x256" and route(sw, K=128, nbatch=2)["kernel"] == "dma_128x128"
    assert route(sw, N=1024)["kernel"] == "sw_128x256" and route(sw, N=1024 + 64)["kernel"] == "dma_128x128"
    # narrow outputs, both 128 x 64 kernels
    for name, wide, narrow in (("dma_n64", "dma_128x128", "dma_128x64"), ("at_n64", "at_f32_128x128", "at_f32_128x64")):
        assert route(by_name(name))["kernel"] == narrow and route(by_name(name), N=68, ldb=68)["kernel"] == wide
    # the weight gradient: N % 256, K >= 192, and which ragged row counts the 128 x 256 form takes
    wg = by_name("swtr_whole")
    assert route(wg, N=128, ldb=128)["kernel"] == "tr_128x128" and route(wg, K=128, strideA=128 * 128, strideB=128 * 256)["kernel"] == "tr_128x128"
    assert route(wg, M=64)["refusal"] == "at_f32"      # no whole 128 x 128 tile: not the shadow form, and no fp32 operands here
    rag = by_name("swtr_ragged_zero_row")
    assert [route(rag, validK=v)["krag"] for v in (193, 255)] == [1, 63] and route(rag, validK=256)["krag"] == 0
    assert route(rag, validK=192)["kernel"] == "tr_128x128"            # a whole K tile missing: not the ragged form
    assert route(rag, b_zero_row=0)["kernel"] == "tr_128x128"
    assert route(by_name("swtr_kextra"))["kernel"] == "swtr_128x256" and route(by_name("kextra_on_tr_n128"))["refusal"] == "kextra_on_tr"


def test_force_kernel_overrides_the_size_rules_only():
    sw, small = by_name("sw_256_tiles"), by_name("force2_below_threshold")
    assert route(sw, force_kernel=1)["kernel"] == "dma_128x128" and route(small, force_kernel=0)["kernel"] == "dma_128x128"
    assert route(small, force_kernel=2)["kernel"] == "sw_128x256"
    # 2 does not override the shape, nor the two-level batch
    assert route(by_name("dma_n320"), force_kernel=2)["kernel"] == "dma_128x128" and route(by_name("dma_k128"), force_kernel=2)["kernel"] == "dma_128x128"
    assert route(by_name("zmod_on_sw_shape"), force_kernel=2)["kernel"] == "dma_128x128"
    # the weight gradient takes the 128 x 256 form by shape alone: 1 keeps it off, 0 and 2 are the same
    wg = by_name("swtr_whole")
    assert [route(wg, force_kernel=f)["kernel"] for f in (0, 1, 2)] == ["swtr_128x256", "tr_128x128", "swtr_128x256"]
    assert route(by_name("tr_n128"), force_kernel=2)["kernel"] == "tr_128x128"
    # nothing else reads it
    for name in ("f32_vec", "f32_k72", "a_shadow_only", "b_shadow_only", "at_n256", "at_n64", "dma_n64"):
        assert len({route(by_name(name), force_kernel=f)["kernel"] for f in (0, 1, 2)}) == 1, name


def test_every_refusal_row_is_refused():
    refused = [r for r in ROWS if r["refusal"]]
    assert {r["refusal"] for r in refused} == set(REFUSALS[1:])
    for r in refused:
        rt = route(r)
        assert rt["kernel"] is None and rt["refusal"] == r["refusal"], r["name"]


def test_a_shadow_that_cannot_be_streamed_falls_to_the_next_source():
    """A16 or B16 off 16 bytes (or with rows that break 16-byte pieces) counts as not given: with both fp32 operands behind them
    the sources fall 5 -> 3 | 2 -> 1 -> 0, without them the call is refused."""
    both = dict(by_name("a_shadow_only")["problem"], B16=ALIGNED, ldb16=128)
    row = {"problem": both}
    assert route(row)["kernel"] == "dma_128x128"
    assert route(row, A16=PRESENT)["kernel"] == "b_shadow" and route(row, B16=PRESENT)["kernel"] == "a_shadow"
    assert route(row, A16=PRESENT, B16=PRESENT)["kernel"] == "f32_vec"
    assert route(row, A16=PRESENT, B16=PRESENT, A=PRESENT)["kernel"] == "f32_guarded"
    assert route(row, lda=132)["kernel"] == "b_shadow" and route(row, ldb16=132)["kernel"] == "a_shadow"      # rows of 264 bytes
    assert route(row, A16=PRESENT, A=PRESENT)["kernel"] == "f32_guarded"      # B's shadow needs 16-byte loads of A beside it
    assert route(row, A16=PRESENT, A=ABSENT)["refusal"] == "shadow_only" and route(row, B16=PRESENT, B=ABSENT)["refusal"] == "shadow_only"
    # the weight gradient: a shadow off 16 bytes leaves the fp32 form, which the fp32 operands must then satisfy
    wg = dict(by_name("swtr_whole")["problem"], A=ALIGNED, B=ALIGNED)
    assert route({"problem": wg})["kernel"] == "swtr_128x256"
    for f in ("A16", "B16p"):
        assert route({"problem": wg}, **{f: PRESENT})["kernel"] == "at_f32_128x128"
    assert route({"problem": wg}, A16=PRESENT, B=PRESENT)["refusal"] == "at_f32"
