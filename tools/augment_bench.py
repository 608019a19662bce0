#!/usr/bin/env python
"""Time of the augmentation kernels on seeded noise.  Reports one JSON line.

The batch is the training benchmark's: --batch utterances (default 32) of --samples samples (default 246000).  Cases:
  fir_<K>       one w2v2_fir call, every utterance with its own K-tap filter (K = 4000, 8000, 16000), direct path at tap K / 100,
                without and with match_power (HIP events; median, min and max of --steps).  `tflops` counts 2 len K flops per
                utterance over the median; `of_peak` is its share of the 157.3 TF fp32 matrix peak
  mix           one w2v2_mix call on the same batch, noise recordings of 10 s; `gbps` counts the five passes it makes (the signal
                and the noise read twice, the output written once) over the median
  augment       Augment(rirs of 8000 taps, noises) on the batch from Python, everything included

    python tools/augment_bench.py [--batch 32] [--samples 246000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))

PEAK_TF = 157.3         # fp32 matrix peak


def stats(t, digits=3):
    t = sorted(t)
    return {"ms": round(float(np.median(t)), digits), "min": round(t[0], digits), "max": round(t[-1], digits)}


def events(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=246000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--taps", type=int, nargs="*", default=[4000, 8000, 16000])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from wav2vec2 import _native as N
    from wav2vec2.audio import Augment
    torch.cuda.set_device(0)
    lib = N.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    B, n = args.batch, args.samples
    x = torch.randn(B * n, device="cuda", generator=gen)
    y = torch.empty_like(x)
    gain = torch.empty(B, device="cuda")
    lens = np.full(B, n, np.int64)
    in0 = (np.arange(B) * n).astype(np.int64)
    res = {"batch": B, "samples": n, "steps": args.steps, "peak_tf": PEAK_TF}
    for K in args.taps:
        decay = torch.exp(-torch.arange(K, device="cuda") / (K / 7.0))
        taps = torch.randn(B * K, device="cuda", generator=gen) * decay.repeat(B)
        taps0 = (np.arange(B) * K).astype(np.int64)
        ntaps = np.full(B, K, np.int32)
        delay = np.full(B, K // 100, np.int32)
        one = {"gflop": round(2e-9 * B * n * K, 1)}
        for key, match in (("kernel", 0), ("kernel_match_power", 1)):
            def call():
                N.check(lib.w2v2_fir(N.ptr(x), B, N.ptr(in0), N.ptr(lens), N.ptr(taps), N.ptr(taps0), N.ptr(ntaps), N.ptr(delay),
                                     N.ptr(y), N.ptr(in0), match, N.ptr(gain), N.current_stream()), "w2v2_fir")
            one[key] = events(torch, call, args.steps, args.warmup)
        one["tflops"] = round(2e-9 * B * n * K / one["kernel"]["ms"], 2)
        one["of_peak"] = round(one["tflops"] / PEAK_TF, 4)
        res[f"fir_{K}"] = one
    m = 160000
    noise = torch.randn(B * m, device="cuda", generator=gen)
    noise0, noise_len = (np.arange(B) * m).astype(np.int64), np.full(B, m, np.int64)
    offset = np.random.default_rng(args.seed).integers(0, m, size=B).astype(np.int64)
    scale = np.full(B, 10.0 ** (-10.0 / 20.0), np.float64)

    def mix():
        N.check(lib.w2v2_mix(N.ptr(x), B, N.ptr(in0), N.ptr(lens), N.ptr(noise), N.ptr(noise0), N.ptr(noise_len), N.ptr(offset),
                             N.ptr(scale), N.ptr(y), N.ptr(in0), N.ptr(gain), N.current_stream()), "w2v2_mix")

    k = events(torch, mix, args.steps, args.warmup)
    res["mix"] = {"kernel": k, "gbps": round(5 * 4.0 * B * n / k["ms"] * 1e-6, 1)}

    rng = np.random.default_rng(args.seed)
    rirs = [rng.standard_normal(8000) * np.exp(-np.arange(8000) / 1200.0) for _ in range(8)]
    aug = Augment(rirs=rirs, noises=[rng.standard_normal(m).astype(np.float32) for _ in range(4)], seed=args.seed)
    waves = list(torch.split(x, [n] * B))
    t = []
    for i in range(args.warmup + max(3, args.steps // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug(waves)
        torch.cuda.synchronize()
        if i >= args.warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    res["augment"] = {"call": stats(t, 2), "taps": [int(v) for v in aug.rirs.lengths]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
