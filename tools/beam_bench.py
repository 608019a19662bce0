#!/usr/bin/env python
"""Time of the CTC prefix beam search (w2v2_ctc_beam_search) on tools/packed_bench.py's utterance set: 64 seeded lengths of 1.5-35 s
through the base Wav2Vec2ForCTC (seeded weights, fp32) as one predict_packed call, decoded at beam widths 1, 16 and 64 without a
language model and at width 16 with a 3-gram table (counted on seeded id sequences).  Reports, as one JSON line, per configuration:

  kernel_ms     one w2v2_ctc_beam_search call on the packed views (HIP events around the call; median, min and max of --steps)
  us_per_step   kernel_ms over the frame count of the longest utterance (the sweep is sequential in frames)
  call_ms       one beam_search() call from Python (checks, output allocation, the kernels, the copies back, the Hypothesis lists)
  ref_ms        the fp64 numpy reference (tests/beam_reference.py) on the first --ref-n utterances, on the host, and whether its
                transcripts equal the kernel's (ref_equal; utterances whose smallest decision margin is below the rounding bound
                are left out of that comparison and counted in ref_fragile)
and once: packed_ms, the packed fp32 forward of the set measured in the same run -- the yardstick: the decoder at width 16 should
cost less than the forward it follows (over_packed = kernel_ms / packed_ms).

    python tools/beam_bench.py [--n 64] [--steps 10] [--warmup 2] [--nbest 1] [--ref-n 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nbest", type=int, default=1)
    ap.add_argument("--ref-n", type=int, default=2, help="utterances the host reference is timed on (0: skip); seconds each")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import CharNgramLM, beam_search
    torch.cuda.set_device(0)
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    rng = np.random.default_rng(args.seed)                       # the packed_bench set
    lens = rng.integers(int(args.min_s * SR), int(args.max_s * SR) + 1, size=args.n)
    waves = [torch.randn(int(n), device="cuda") for n in lens]

    logits = m.predict_packed(waves)
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        logits = m.predict_packed(waves)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    packed_ms = float(np.median(t)) * 1e3

    vs, blank = cfg.vocab_size, cfg.pad_id
    lrng = np.random.default_rng(args.seed + 2)
    letters = [v for v in range(vs) if v != blank]
    lm3 = CharNgramLM.from_ids([lrng.choice(letters, size=200).tolist() for _ in range(50)], vs, blank, order=3, add_k=0.5,
                               alpha=0.5, beta=0.1)

    base, row0, fl = _logits_base(logits, None)
    n, max_len, tot = len(fl), max(fl), sum(fl)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    nbest = args.nbest
    labels = torch.empty((n, nbest, max_len), dtype=torch.int32, device="cuda")
    length = torch.empty((n, nbest), dtype=torch.int32, device="cuda")
    score = torch.empty((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.empty((n, nbest), dtype=torch.float64, device="cuda")
    lib = N.load()
    res = {"n": n, "audio_s": round(float(lens.sum()) / SR, 2), "frames": tot, "max_frames": max_len, "vocab": vs, "nbest": nbest,
           "packed_ms": round(packed_ms, 2), "packed_ms_spread": [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)], "configs": []}

    for W, lm in [(1, None), (16, None), (64, None), (16, lm3)]:
        if nbest > W:
            continue
        table = lm.device_table(base.device) if lm is not None else None

        def kernel():
            N.check(lib.w2v2_ctc_beam_search(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, nbest, N.ptr(table),
                                             lm.order if lm else 1, lm.alpha if lm else 0.0, lm.beta if lm else 0.0, max_len,
                                             N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))

        for _ in range(args.warmup):
            kernel()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            kernel()
            b.record()
        torch.cuda.synchronize()
        kt = sorted(a.elapsed_time(b) for a, b in ev)
        kernel_ms = float(np.median(kt))
        ct = []
        for _ in range(max(3, args.steps // 3)):
            t0 = time.perf_counter()
            hyps = beam_search(logits, beam_width=W, nbest=nbest, blank=blank, lm=lm)
            ct.append(time.perf_counter() - t0)
        c = {"beam_width": W, "lm_order": lm.order if lm else 0, "kernel_ms": round(kernel_ms, 3), "kernel_ms_min": round(kt[0], 3),
             "kernel_ms_max": round(kt[-1], 3), "us_per_step": round(kernel_ms * 1e3 / max_len, 3),
             "call_ms": round(float(np.median(ct)) * 1e3, 3), "over_packed": round(kernel_ms / packed_ms, 4),
             "mean_len": round(float(np.mean([len(h[0].ids) for h in hyps if h])), 1)}
        if args.ref_n:
            import beam_reference as BR
            hosts = [l.cpu().numpy() for l in logits[:args.ref_n]]
            t0 = time.perf_counter()
            refs = [BR.search(h, W, nbest, blank, None if lm is None else lm.table, lm.order if lm else 1, lm.alpha if lm else 0.0,
                              lm.beta if lm else 0.0) for h in hosts]
            c["ref_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            c["ref_n"] = len(hosts)
            firm = [i for i, (r, h) in enumerate(zip(refs, hosts)) if r.margin >= BR.tau(h.shape[0], r.kmax)]
            c["ref_fragile"] = len(hosts) - len(firm)
            c["ref_equal"] = all([x.ids for x in hyps[i]] == [k for k, _, _ in refs[i].hyps] for i in firm)
        res["configs"].append(c)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
