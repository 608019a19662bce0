#!/usr/bin/env python
"""Which kernel each row of tests/golden/attention_routes.json launches, by its name in a kernel trace -- needs no launch counter, so
it also runs on a commit older than w2v2_op_attention_launches (the table's "recorded" column was taken that way):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/attention_route_record.py run DIR
    python tools/attention_route_record.py join DIR          -> DIR/recorded.json  {row: kernel name(s) | refusal message}
`run` launches every row with an op once, in table order, through tests/test_attention_route_gpu.py's run_row (ops older than the
route only).  `join` reads the trace: the attention kernels of the process are the accepted rows', in order -- one per forward row;
a backward row ran its training forward first, which is skipped, and owns the kernels from its first backward kernel up to and
including the dK / dV kernel (joined with " + ")."""
import csv, glob, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsoc-wav2vec2_amd"), os.path.join(ROOT, "tests")]
mode, out_dir = sys.argv[1], sys.argv[2]

if mode == "run":
    import torch
    from wav2vec2 import _native as N
    import test_attention_route_gpu as T
    lib, dev, done = N.load(), torch.device("cuda:0"), []
    for row in T.ROWS:
        rc, _ = T.run_row(lib, torch, dev, row, T.qkv_of(row))
        done.append({"name": row["name"], "op": row["op"], "rc": rc, "error": N.last_error() if rc else None})
        print(json.dumps(done[-1]), flush=True)
    json.dump(done, open(os.path.join(out_dir, "rows.json"), "w"), indent=1)
else:
    rows = json.load(open(os.path.join(out_dir, "rows.json")))
    trace = []
    for f in glob.glob(os.path.join(out_dir, "**", "*_kernel_trace.csv"), recursive=True):
        trace += list(csv.DictReader(open(f)))
    trace.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [re.sub(r"^void ", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).split("(")[0] for r in trace]
    names = [n for n in names if "attention" in n or "attn" in n]
    recorded, i = {}, 0
    for r in rows:
        if r["rc"] != 0:
            recorded[r["name"]] = r["error"]      # (a refused backward's forward was refused too: the same head sizes)
            continue
        if r["op"] == "attention_bwd":
            while "bwd" not in names[i] and "dvec" not in names[i]:
                i += 1      # its training forward
            j = i
            while "dkv" not in names[j]:
                j += 1
            recorded[r["name"]] = " + ".join(names[i:j + 1])
            i = j + 1
        else:
            recorded[r["name"]] = names[i]
            i += 1
    assert i == len(names), (i, len(names))
    json.dump(recorded, open(os.path.join(out_dir, "recorded.json"), "w"), indent=1)
    for r in rows:
        print(f"{r['name']:32s} {recorded[r['name']]}")
