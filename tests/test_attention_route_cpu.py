"""Which attention kernel a problem reaches (csrc/attention_route.h through w2v2_op_attention_route: host only, no GPU).

tests/golden/attention_routes.json holds one row per mode x head size x dense / packed x pass, per rule of the route and per
boundary of a rule: the op call that poses the problem, the problem as the route sees it, and what the commit BEFORE the route
existed did with it -- "recorded" is the kernel's name in a kernel trace of that commit (tools/attention_route_record.py; a
backward row: its kernels joined with " + "), or the message it refused the call with.  Rows no op can pose (a bf16 shadow or planes
wanted, unaligned buffers, the plan of a model whose head size is not 64, W2V2_SPLIT_ATTN off) are "derived": they name the lines of
that commit their expectation was read from.  tests/test_attention_route_gpu.py runs the recorded rows."""

import ctypes as C
import json
import os

import pytest

from wav2vec2 import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_routes.json")
TABLE = json.load(open(GOLDEN))
KERNELS, REFUSALS, ROWS = TABLE["kernels"], TABLE["refusals"], TABLE["rows"]
FAMILIES = [None, "f32", "split", "bf16"]
FIELDS = ["pass", "precision", "B", "T", "H", "heads", "packed", "split_allowed", "io_aligned", "want_f32", "want_b16", "want_planes"]
INFER, TRAIN, BWD = range(3)


def trace_names(kernel):
    """the name(s) a kernel id has in a kernel trace"""
    part = kernel.split("_")
    if part[0] == "f32":
        dh = next(p for p in part if p[0] == "d")[1:]
        if part[1] == "bwd":
            return [f"attn_dvec_kernel<{dh}>", f"attention_bwd_dq_kernel<{dh}>", f"attention_bwd_dkv_kernel<{dh}>"]
        waves = "8" if part[1] == "packed" else part[-1][1:]
        return [f"attention_kernel<{dh}, {waves}, {'true' if part[1] == 'train' else 'false'}, {'true' if part[1] == 'packed' else 'false'}>"]
    if part[0] == "split":
        return [f"attention_split_kernel<{1 if part[-1] == 'f16x2' else 0}, {'true' if part[1] == 'packed' else 'false'}>"]
    return {"bf16": ["attention_bf16_pipe_kernel<false, false, false>"], "bf16_packed": ["attention_bf16_pipe_kernel<false, false, true>"],
            "bf16_train": ["attention_bf16_pipe_kernel<true, false, false>"],      # (the table's training rows run without dropout)
            "bf16_bwd": ["attention_bf16_bwd_dq_kernel<false>", "attention_bf16_bwd_dkv_kernel<false>"]}[kernel]


def route(row, **over):
    p = dict(row["problem"], **over)
    out = (C.c_int32 * 10)()
    N.check(N.load().w2v2_op_attention_route((C.c_int32 * len(FIELDS))(*[int(p[f]) for f in FIELDS]), out), "w2v2_op_attention_route")
    return dict(kernel=KERNELS[out[0]], refusal=REFUSALS[out[1]], family=FAMILIES[out[2]], fmt=out[3], dh=out[4], waves=out[5], rows=out[6],
                lse_log2=bool(out[7]), writes_b16=bool(out[8]), writes_planes=bool(out[9]))


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_route_matches_the_table(row):
    rt, p = route(row), row["problem"]
    assert (rt["kernel"], rt["refusal"], rt["family"], rt["waves"], rt["rows"]) == (row["kernel"], row["refusal"], row["family"], row["waves"], row["rows"]), rt
    assert (rt["kernel"] is None) == (rt["refusal"] is not None) and rt["dh"] == p["H"] // p["heads"]
    if row["recorded"] is None:
        assert row["op"] is None and row["derived"], "a row without a recording says which lines its expectation was read from"
    elif row["refusal"]:
        who = {INFER: "attention_packed: " if p["packed"] else "attention: ", TRAIN: "attention_train: ", BWD: "attention_bwd: "}[p["pass"]]
        assert row["recorded"].startswith(who) and (row["refusal"] != "head_size" or f"head size {rt['dh']} unsupported" in row["recorded"])
    else:
        assert [n.replace("w2v2::", "") for n in row["recorded"].split(" + ")] == trace_names(row["kernel"])
    if rt["kernel"]:
        assert rt["rows"] == 32 * rt["waves"]
        assert rt["fmt"] == ({2: 0, 3: 1}[p["precision"]] if rt["family"] == "split" else -1)
        assert rt["writes_b16"] == (rt["family"] == "bf16") and rt["writes_planes"] == (rt["family"] == "split")
        assert rt["lse_log2"] == (rt["family"] == "bf16" and p["pass"] != INFER)


def test_table_reaches_every_kernel_and_refusal():
    routes = [route(r) for r in ROWS]
    assert {rt["kernel"] for rt in routes} == set(KERNELS) and {rt["refusal"] for rt in routes} == set(REFUSALS)
    # ... and covers modes 0-3 x head sizes 32 / 64 / 128 x dense / packed x the three passes (packed: inference only)
    seen = {(r["problem"]["pass"], r["problem"]["precision"], r["problem"]["H"] // r["problem"]["heads"], r["problem"]["packed"]) for r in ROWS}
    assert {(ps, m, dh, pk) for ps in range(3) for m in range(4) for dh in (32, 64, 128) for pk in ((0, 1) if ps == INFER else (0,))} <= seen


def test_wave_counts_flip_where_the_cost_model_says():
    """fp32 inference, dense: blocks of 32 nw queries per (batch, head), 256 CUs (two blocks each at 4 waves, head size < 128), cost =
    rounds x waves in flight x (9 at 12 waves, else 10), candidates 12, 8, 4, the first strict minimum wins."""
    w12 = by_name("waves12_d64")      # 172 (batch, head) pairs of 257 queries: one 12-wave round against two of 8 or 4 waves
    assert [route(w12, T=t)["waves"] for t in (257, 384, 385)] == [12, 12, 8]      # 385: two 12-wave blocks per pair, two rounds; 8 and 4 tie at 160, 8 comes first
    assert route(w12, B=64)["waves"] == 12 and route(w12, B=65)["waves"] == 4      # 260 pairs: two 12-wave rounds (216), three of 8 waves (240), two of 4 (160)
    w4 = by_name("waves4_d64")        # 260 pairs of 64 queries: one round at two blocks per CU against two
    assert route(w4, B=64)["waves"] == 8 and route(w4)["waves"] == 4               # 256 pairs: one round each, 80 = 80, 8 comes first
    assert route(w4, H=512)["waves"] == 4                                          # head size 128: one block per CU at 4 waves, two rounds either way: 80 against 160
    assert route(by_name("waves8_d128_on_a_tie"), B=128)["waves"] == 4             # 256 blocks of 4 waves: one round, 40 against 80
    for r in ROWS:                    # no head-size-128 route has 12 waves; packed, split and bf16 routes do not depend on the shape
        if r["kernel"] and r["problem"]["H"] // r["problem"]["heads"] == 128:
            assert route(r, B=43, T=257)["waves"] != 12
    for name, waves in (("packed_fp32_d64", 8), ("packed_bf16x3_d64", 8), ("packed_bf16_d64", 4), ("infer_bf16_d64", 4), ("infer_f16x2_d64", 8)):
        assert {route(by_name(name), B=b, T=t)["waves"] for b, t in ((1, 1), (43, 257), (65, 64), (32, 768))} == {waves}


def test_training_takes_twelve_waves_from_384_frames_on():
    row = by_name("train_T384")
    assert [route(row, T=t)["kernel"] for t in (383, 384, 385, 2000)] == ["f32_train_d64_w4"] + ["f32_train_d64_w12"] * 3
    assert route(row, H=32)["kernel"] == "f32_train_d32_w4" and route(row, B=64)["kernel"] == "f32_train_d64_w12"      # T alone decides
    assert route(row, **{"pass": BWD})["kernel"] == "f32_bwd_d64"


def test_the_family_follows_mode_head_size_and_alignment():
    dense = by_name("infer_bf16x3_d64")
    assert route(dense)["family"] == "split"
    for over in (dict(io_aligned=0), dict(split_allowed=0), dict(precision=0), dict(H=256, heads=2), dict(H=64, heads=2)):
        assert route(dense, **over)["family"] == "f32", over
    assert route(dense, precision=1)["family"] == "bf16" and route(dense, precision=1, io_aligned=0)["family"] == "bf16"
    # the split family serves inference only; the bf16 family every pass, with or without a shadow asked for
    for ps in (TRAIN, BWD):
        assert route(dense, **{"pass": ps})["family"] == "f32" and route(dense, precision=1, **{"pass": ps})["family"] == "bf16"
    assert route(dense, precision=1, want_b16=1)["kernel"] == "bf16" and route(dense, precision=1, want_f32=0, want_b16=1)["kernel"] == "bf16"
    # a form the family cannot write is refused, whatever else is asked for
    assert route(dense, want_b16=1)["refusal"] == "shadow" and route(dense, precision=0, want_planes=1)["refusal"] == "planes"
    assert route(dense, want_planes=1)["kernel"] == "split_bf16x3" and route(dense, precision=3, want_planes=1, packed=1)["kernel"] == "split_packed_f16x2"
    # the shadow is looked at before the head size, the head size last (the order of the launchers before the route)
    assert route(by_name("refuse_d96"), want_b16=1)["refusal"] == "shadow" and route(by_name("refuse_d96"), want_planes=1)["refusal"] == "planes"
    # head size 128 exists in inference only
    d128 = by_name("infer_fp32_d128")
    assert route(d128)["kernel"] and route(d128, packed=1)["kernel"] and route(d128, **{"pass": TRAIN})["refusal"] == "head_size"


def test_every_refusal_row_is_refused():
    refused = [r for r in ROWS if r["refusal"]]
    assert {r["refusal"] for r in refused} == set(REFUSALS[1:])
    for r in refused:
        rt = route(r)
        assert rt["kernel"] is None and rt["refusal"] == r["refusal"] and rt["waves"] == 0, r["name"]
