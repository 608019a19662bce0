#!/usr/bin/env python
"""What the training step launches for the rows of tests/golden/weight_grad_plans.json that carry a "record" spec, by the weight-gradient
kernel's name and grid in a kernel trace -- needs no plan op, so it also runs on a commit older than w2v2_op_weight_grad_plan (the
table's "recorded" column was taken that way).  One process per row, in a run that collects nothing else:
    for ROW in $(python tools/weight_grad_plan_record.py rows); do
        rocprofv3 --kernel-trace --output-format csv -d DIR/$ROW -- python tools/weight_grad_plan_record.py run DIR $ROW; done
    python tools/weight_grad_plan_record.py join DIR          -> DIR/recorded.json  {row: {"kernel": name, "grid_z": slabs}}
`run` builds a one-layer model of the row's dims, makes the row's site the only trainable variable and runs one training forward and
backward in mode bf16 over B x L samples (B T = the row's M).  `join` reads each trace: the first weight-gradient GEMM (a transposed
form of the bf16 GEMM kernels) is the site's -- the packed q|k|v gradient, which the step computes whatever is trainable, comes after it."""
import csv, glob, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gsoc-wav2vec2_amd"), os.path.join(ROOT, "tests")]
ROWS = [r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "weight_grad_plans.json"))) if r.get("record")]
SITES = {"ffn_up": "feed_forward/intermediate_dense/kernel", "ffn_down": "feed_forward/output_dense/kernel", "out_proj": "attention/out_proj/kernel"}
WGRAD = re.compile(r"gemm_bf16_sw_kernel<false, true, 0, true>|gemm_bf16_tr_kernel<|gemm_bf16_kernel<7, ")
mode = sys.argv[1]

if mode == "rows":
    print(" ".join(r["name"] for r in ROWS))
elif mode == "run":
    import numpy as np
    import torch
    import wav2vec2
    from wav2vec2 import variables as V
    from wav2vec2.training import Trainer
    row = next(r for r in ROWS if r["name"] == sys.argv[3])
    a, q = row["record"], row["problem"]
    small = dict(filter_sizes=[64] * 7, num_conv_pos_embeddings=32, num_conv_pos_embedding_groups=4) if a["H"] < 512 else {}
    cfg = wav2vec2.Wav2Vec2Config(hidden_size=a["H"], num_heads=a["heads"], num_layers=1, intermediate_size=a["F"], **small)
    assert a["B"] * cfg.num_frames(a["L"]) == q["M"] and {"ffn_up": (a["H"], a["F"]), "ffn_down": (a["F"], a["H"]), "out_proj": (a["H"], a["H"])}[a["site"]] == (q["Kin"], q["Nout"])
    torch.cuda.set_device(0)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(a["B"], a["L"]))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    m.set_precision("bf16")
    m.set_trainable("", False)
    m.set_trainable("encoder/layers/0/" + SITES[a["site"]], True)
    tr = Trainer(m, None, seed=0, dropout=0.1, apply_spec_augment=False)
    wave = V.hash_normal("weight_grad_plan_record", a["B"] * a["L"], 8).reshape(a["B"], a["L"])
    logits = tr.forward(wave, sd_keep=np.ones(1, dtype=np.float32), step_seed=1)
    tr.backward(torch.sin(logits))
    torch.cuda.synchronize()
    g = tr.gradient("encoder/layers/0/" + SITES[a["site"]])
    print(json.dumps({"name": row["name"], "finite": bool(np.isfinite(g).all()), "max_abs": float(np.abs(g).max())}), flush=True)
else:
    recorded = {}
    for row in ROWS:
        trace = []
        for f in glob.glob(os.path.join(sys.argv[2], row["name"], "**", "*_kernel_trace.csv"), recursive=True):
            trace += list(csv.DictReader(open(f)))
        trace.sort(key=lambda r: int(r["Start_Timestamp"]))
        hits = [r for r in trace if WGRAD.search(r["Kernel_Name"])]
        if not hits:
            print(f"{row['name']:28s} no weight-gradient kernel in the trace")
            continue
        k = hits[0]
        name = re.sub(r"^void ", "", k["Kernel_Name"].replace("(anonymous namespace)::", "")).split("(")[0]
        recorded[row["name"]] = {"kernel": name, "grid_z": int(k["Grid_Size_Z"]) // int(k["Workgroup_Size_Z"]),
                                 "grid_xy": int(k["Grid_Size_X"]) // int(k["Workgroup_Size_X"]) * (int(k["Grid_Size_Y"]) // int(k["Workgroup_Size_Y"]))}
        print(f"{row['name']:28s} {name}  z = {recorded[row['name']]['grid_z']}  x y = {recorded[row['name']]['grid_xy']}  ({len(hits)} weight-gradient GEMMs in the trace)")
    json.dump(recorded, open(os.path.join(sys.argv[2], "recorded.json"), "w"), indent=1)
