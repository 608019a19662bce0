#!/usr/bin/env python
"""Which kernel each row of tests/golden/gemm_bf16_routes.json launches, by its name in a kernel trace -- needs no launch counter,
so it also runs on a commit older than w2v2_op_gemm_bf16_launches (the table's "recorded" column was taken that way):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_bf16_route_record.py run DIR
    python tools/gemm_bf16_route_record.py join DIR          -> DIR/recorded.json  {row: kernel name | refusal message}
`run` launches every row once, in table order, through tests/test_gemm_bf16_route_gpu.py's run_row, and only then the reference
kernels; it also writes whether each row's output carries the reference's bits.  `join` reads the trace: the first gemm_bf16 kernels
of the process are the accepted rows', in order."""
import csv, glob, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gsoc-wav2vec2_amd"), os.path.join(ROOT, "tests")]
mode, out_dir = sys.argv[1], sys.argv[2]

if mode == "run":
    import torch
    from wav2vec2 import _native as N
    import test_gemm_bf16_route_gpu as T
    lib, dev = N.load(), torch.device("cuda:0")
    done = []
    for row in T.ROWS:
        ops = T.operands(torch, dev, row)
        rc, out = T.run_row(lib, torch, dev, row, ops)
        done.append((row, ops, out, {"name": row["name"], "rc": rc, "error": N.last_error() if rc else None}))
    for row, ops, out, rec in done:
        if rec["rc"] == 0:
            ref = T.reference(lib, torch, dev, row, ops)
            rec["finite"] = bool(torch.isfinite(ref).all())
            rec["bits_equal"] = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
            if not rec["bits_equal"]:
                rec["differing"] = int((out.view(torch.int32) != ref.view(torch.int32)).sum())
                rec["max_abs_diff"] = float((out - ref).abs().max())
        print(json.dumps(rec), flush=True)
    json.dump([d[3] for d in done], open(os.path.join(out_dir, "rows.json"), "w"), indent=1)
else:
    rows = json.load(open(os.path.join(out_dir, "rows.json")))
    trace = []
    for f in glob.glob(os.path.join(out_dir, "**", "*_kernel_trace.csv"), recursive=True):
        trace += list(csv.DictReader(open(f)))
    trace.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [re.sub(r"^void ", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).split("(")[0] for r in trace if "gemm_bf16" in r["Kernel_Name"]]
    accepted = [r for r in rows if r["rc"] == 0]
    assert len(names) >= len(accepted), (len(names), len(accepted))
    recorded = {r["name"]: r["error"] for r in rows if r["rc"] != 0}
    recorded.update({r["name"]: k for r, k in zip(accepted, names)})
    json.dump(recorded, open(os.path.join(out_dir, "recorded.json"), "w"), indent=1)
    for r in rows:
        print(f"{r['name']:28s} {recorded[r['name']]}  {'' if r['rc'] else 'bits == reference: ' + str(r['bits_equal'])}")
