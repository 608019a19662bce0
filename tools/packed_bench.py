#!/usr/bin/env python
"""Throughput of three ways to run one set of differently sized utterances through the base Wav2Vec2ForCTC (seeded weights), in
one precision mode (--precision fp32 | bf16 | bf16x3 | f16x2, default fp32; the mode holds for all three forms; "bf16" sets the
option "bf16_packed", which the packed form needs in that mode -- b1 and padded run the dense bf16 forward either way):

  packed  one predict_packed call (w2v2_forward_packed): each utterance exact, no padded frame computed;
  b1      a B = 1 loop: exact, one forward per utterance (a new length re-sizes the workspace, as for any caller);
  padded  one batch zero-padded to the longest utterance (the reference notebooks' protocol): padding enters base checkpoints'
          GroupNorm statistics, and every padded frame costs full compute.

The lengths are drawn once from a seed, uniform in [--min-s, --max-s] seconds (default 64 utterances of 1.5-35 s, roughly
LibriSpeech test-clean's range).  Prints one JSON line: audio-s/s per form, ms per pass, and the padded batch's padding fraction.
--families adds one more packed pass under the model's profiler and its time per kernel family ("packed_families_ms").

    python tools/packed_bench.py [--n 64] [--steps 3] [--warmup 1] [--forms packed,b1,padded] [--precision fp32] [--families]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", default="packed,b1,padded")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16x3", "f16x2"])
    ap.add_argument("--families", action="store_true")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import variables as V
    torch.cuda.set_device(0)
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    m.set_precision(args.precision)
    if args.precision == "bf16":
        m.set_option("bf16_packed", True)
    rng = np.random.default_rng(args.seed)
    lens = rng.integers(int(args.min_s * SR), int(args.max_s * SR) + 1, size=args.n)
    waves = [torch.randn(int(n), device="cuda") for n in lens]
    audio_s = float(lens.sum()) / SR
    Lmax = int(lens.max())

    def run_packed():
        m.predict_packed(waves)

    def run_b1():
        for w in waves:
            m(w[None])

    padded = None

    def run_padded():
        m(padded)

    forms = {"packed": run_packed, "b1": run_b1, "padded": run_padded}
    res = {"precision": args.precision, "n": args.n, "audio_s": round(audio_s, 2), "min_len": int(lens.min()), "max_len": Lmax,
           "padding_fraction": round(1.0 - float(lens.sum()) / (args.n * Lmax), 4),
           "frames": int(sum(m.num_frames(int(n)) for n in lens)), "padded_frames": args.n * m.num_frames(Lmax)}
    for name in args.forms.split(","):
        if name == "padded":
            padded = torch.zeros(args.n, Lmax, device="cuda")
            for i, w in enumerate(waves):
                padded[i, :w.shape[0]] = w
        fn = forms[name]
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        best, med = min(times), float(np.median(times))
        res[name] = {"ms_median": round(med * 1e3, 2), "ms_min": round(best * 1e3, 2), "audio_s_per_s": round(audio_s / med, 1)}
        if name == "padded":
            padded = None
            torch.cuda.empty_cache()
    if args.families and "packed" in res:
        m.profile(True)
        m.profile_reset()
        run_packed()
        torch.cuda.synchronize()
        res["packed_families_ms"] = {k: round(v["ms"], 3) for k, v in m.profile_read().items() if v["launches"]}
        m.profile(False)
    if "packed" in res and "padded" in res:
        res["packed_over_padded"] = round(res["packed"]["audio_s_per_s"] / res["padded"]["audio_s_per_s"], 3)
    if "packed" in res and "b1" in res:
        res["packed_over_b1"] = round(res["packed"]["audio_s_per_s"] / res["b1"]["audio_s_per_s"], 3)
    if args.precision == "f16x2":
        res["range_overflow"] = m.range_overflow()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
