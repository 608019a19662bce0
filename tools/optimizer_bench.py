#!/usr/bin/env python
"""Time of the optimizer calls on wav2vec2-base with the stage-2 trainable set (the conv stack frozen: the
90.2 M elements `Trainer.reduce_ranges` documents).  Reports one JSON line.

One short forward + backward creates the gradient buffer; then, arms interleaved in one loop so that they share the clock and
the neighbours, HIP events around each call, median / min / max of --steps:
  adam_step        w2v2_adam_step: the default Trainer's update (Adam + the w2v2_finalize that re-derives the packed tensors)
  norm_adamw_step  w2v2_grad_norm + w2v2_adamw_step: the update with clipping / decay / skip
  grad_norm        w2v2_grad_norm alone (grad_sumsq + grad_norm_finish)
  accumulate_*     one w2v2_grad_accumulate per mode
Each with the bytes it must move (fp32 streams of the trainable elements: Adam 7, the norm 1, store 2, add / finish 3) and the
resulting GB/s; `of_step` is the share of the bf16 fine-tune step of the README (--step-ms, default 31.0).

    python tools/optimizer_bench.py [--steps 30] [--warmup 5] [--step-ms 31.0]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))


def stats(t, digits=4):
    t = sorted(t)
    return {"ms": round(float(np.median(t)), digits), "min": round(t[0], digits), "max": round(t[-1], digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=31.0)
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    torch.cuda.set_device(0)
    cfg = wav2vec2.Wav2Vec2Config()
    B, L = 2, 16000
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(B, L))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    m.freeze_feature_extractor()
    tr = wav2vec2.Trainer(m, wav2vec2.CTCLoss(cfg, (B, L), division_factor=B), dropout=0.0, apply_spec_augment=False)
    x = V.hash_normal("optimizer_bench/wave", B * L, 3).reshape(B, L)
    labels = np.array([[5, 6, 7, 0], [9, 9, 0, 0]], np.int32)
    logits = tr.forward(x, step_seed=1)
    _, dlog = tr.loss.per_sample(labels, logits, with_grad=True)
    tr.backward(dlog)
    elems = sum(n for runs in tr.reduce_ranges() for _, n in runs)
    lib, h = m._lib, m._handle
    lr, b1, b2, eps = 1e-6, 0.9, 0.999, 1e-7
    it = [0]

    def adam():
        it[0] += 1
        N.check(lib.w2v2_adam_step(h, lr, b1, b2, eps, it[0], N.current_stream()), "w2v2_adam_step")

    def norm():
        N.check(lib.w2v2_grad_norm(h, 1.0, 1, N.current_stream()), "w2v2_grad_norm")

    def norm_adamw():
        it[0] += 1
        norm()
        N.check(lib.w2v2_adamw_step(h, lr, b1, b2, eps, 0.01, it[0], N.current_stream()), "w2v2_adamw_step")

    def accumulate(mode):
        return lambda: N.check(lib.w2v2_grad_accumulate(h, mode, N.current_stream()), "w2v2_grad_accumulate")

    # (streams of 4 bytes per trainable element; accumulate FINISH last: it changes the gradient the other arms read)
    arms = [("adam_step", adam, 7), ("norm_adamw_step", norm_adamw, 8), ("grad_norm", norm, 1), ("accumulate_store", accumulate(0), 2),
            ("accumulate_add", accumulate(1), 3), ("accumulate_finish", accumulate(2), 3)]
    times = {name: [] for name, _, _ in arms}
    for step in range(args.warmup + args.steps):
        ev = []
        for name, fn, _ in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.append((name, a, b))
        torch.cuda.synchronize()
        if step >= args.warmup:
            for name, a, b in ev:
                times[name].append(a.elapsed_time(b))
        tr.grad_buffer().mul_(0.25)       # (FINISH doubled it, twice with ADD: keep the gradient finite over the run)
    res = {"model": "wav2vec2-base, stage 2", "trainable_elements": int(elems), "steps": args.steps, "step_ms": args.step_ms}
    for name, _, streams in arms:
        s = stats(times[name])
        nbytes = 4.0 * streams * elems
        s.update(MB=round(nbytes * 1e-6, 1), gbps=round(nbytes / s["ms"] * 1e-6, 1), of_step=round(s["ms"] / args.step_ms, 4))
        res[name] = s
    norm_s, scale, skipped_last, skipped_total = tr._optimizer_stats()
    res["last_norm"], res["last_scale"], res["skipped_total"] = norm_s, scale, int(skipped_total)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
