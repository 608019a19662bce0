#!/usr/bin/env python
"""Time of the CTC phrase search (w2v2_ctc_spot) in its two uses.

A term list over an archive: tools/packed_bench.py's utterance set (64 seeded lengths of 1.5-35 s through the base Wav2Vec2ForCTC,
seeded weights, fp32, one predict_packed call) searched for 1 000 seeded phrases of 3-20 labels, every phrase in every recording:
64 000 pairs in ONE call on the packed views.  One phrase over one long recording: a synthetic hour (180 000 frames of seeded
logits, vocabulary 32) searched whole -- one wave walks it -- and as overlapping pieces (--chunk / --overlap), one wave each.
Reports, as one JSON line (and as a table with --out FILE.md):

  packed_ms        the packed fp32 forward of the set, measured in the same run, for scale
  list_ms          one w2v2_ctc_spot call over every pair (HIP events; median, min and max of --steps; labels on the device)
  list_ns_step     list_ms over the pairs' frame steps (sum over the pairs of the recording's frames)
  hour_ms          one call, one pair, 180 000 frames; hour_ns_step: per frame
  hour_chunked_ms  one call over the pieces of the same pair; find_ms / find_chunked_ms: find_phrases from Python (tables, the
                   kernels, the copy back, the merge of the pieces' hits), wall clock
  hits             stored hits of the list search, and whether the chunked hour found what the whole one did

    python tools/spot_bench.py [--n 64] [--phrases 1000] [--steps 10] [--warmup 2] [--chunk 2048] [--overlap 256] [--out profiles/spot.md]
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


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return float(np.median(t)), t[0], t[-1]


def wall(torch, fn, reps):
    fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, out


def spot_call(torch, N, base, row0, frames, utt, labs, blank, thr, max_hits):
    """the arguments of one w2v2_ctc_spot call, everything in place; returns (callable, count tensor)"""
    V, m = int(base.shape[1]), len(labs)
    row0_h, frames_h, utt_h = np.asarray(row0, np.int64), np.asarray(frames, np.int32), np.asarray(utt, np.int32)
    nlab = np.asarray([len(l) for l in labs], np.int32)
    label0 = np.concatenate(([0], np.cumsum(nlab[:-1], dtype=np.int64))).astype(np.int64)
    lab_dev = torch.from_numpy(np.concatenate([np.asarray(l, np.int32) for l in labs] + [np.zeros(1, np.int32)])).cuda()
    thr_h = np.asarray(thr, np.float64)
    score = torch.empty((m, max_hits), dtype=torch.float64, device="cuda")
    begin = torch.empty((m, max_hits), dtype=torch.int32, device="cuda")
    end = torch.empty((m, max_hits), dtype=torch.int32, device="cuda")
    count = torch.empty(m, dtype=torch.int32, device="cuda")
    lib = N.load()
    keep = (row0_h, frames_h, utt_h, nlab, label0, lab_dev, thr_h, score, begin, end)

    def call():
        N.check(lib.w2v2_ctc_spot(N.ptr(base), V, len(frames_h), N.ptr(row0_h), N.ptr(frames_h), m, N.ptr(utt_h), N.ptr(lab_dev),
                                  N.ptr(label0), N.ptr(nlab), blank, -1, N.ptr(thr_h), max_hits, N.ptr(score), N.ptr(begin), N.ptr(end),
                                  N.ptr(count), None, None, None, N.current_stream()), "w2v2_ctc_spot")
        return keep

    return call, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-hits", type=int, default=8)
    ap.add_argument("--hour-frames", type=int, default=180000)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--overlap", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the result as a markdown table to this file")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.spotting import chunk_plan, find_phrases
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
    base, row0, fl = _logits_base(logits, None)
    n = len(fl)
    prng = np.random.default_rng(args.seed + 1)
    pool = [v for v in range(vs) if v != blank]
    phrases = [prng.choice(pool, int(prng.integers(3, 21))).astype(np.int32) for _ in range(args.phrases)]
    utt = [i for i in range(n) for _ in phrases]
    labs = [p for _ in range(n) for p in phrases]
    thr = [-1.0 * len(p) for p in labs]
    call, count = spot_call(torch, N, base, row0, fl, utt, labs, blank, thr, args.max_hits)
    list_ms, list_min, list_max = timed(torch, call, args.steps, args.warmup)
    steps_total = float(sum(fl)) * len(phrases)
    cnt = count.cpu().numpy()
    res = {"n": n, "audio_s": round(float(lens.sum()) / SR, 2), "frames": int(sum(fl)), "max_frames": max(fl), "vocab": vs,
           "phrases": len(phrases), "pairs": len(utt), "labels_mean": round(float(np.mean([len(p) for p in phrases])), 1),
           "frame_steps": steps_total, "packed_ms": round(packed_ms, 2), "list_ms": round(list_ms, 3), "list_ms_min": round(list_min, 3),
           "list_ms_max": round(list_max, 3), "list_ns_step": round(list_ms * 1e6 / steps_total, 4),
           "over_packed": round(list_ms / packed_ms, 4), "hits": int(np.minimum(cnt, args.max_hits).sum()), "bad_pairs": int((cnt < 0).sum())}

    # one phrase over one synthetic hour
    T, Vh = args.hour_frames, 32
    g = torch.Generator(device="cuda").manual_seed(args.seed + 2)
    hour = torch.randn((T, Vh), device="cuda", generator=g) * 3.0
    hour[:, 0] += 4.0                                            # the blank leads most frames, as in speech
    phrase = np.asarray(np.random.default_rng(args.seed + 3).choice(np.arange(1, Vh), 10, replace=False), np.int32)
    at = torch.arange(500, T - 20, 997, device="cuda")           # the phrase planted every 997 frames, one frame per label
    for k, v in enumerate(phrase):
        hour[at + k, int(v)] += 12.0
    whole, _ = spot_call(torch, N, hour, [0], [T], [0], [phrase], 0, [-10.0], 256)
    hour_ms, hour_min, hour_max = timed(torch, whole, args.steps, args.warmup)
    plan = chunk_plan(T, args.chunk, args.overlap)
    pieces, _ = spot_call(torch, N, hour, [s for s, _ in plan], [f for _, f in plan], list(range(len(plan))), [phrase] * len(plan), 0,
                          [-10.0] * len(plan), 256)
    chunk_ms, chunk_min, chunk_max = timed(torch, pieces, args.steps, args.warmup)
    find_ms, a = wall(torch, lambda: find_phrases([hour], [phrase], min_score=-10.0, max_hits=256), max(3, args.steps // 3))
    chunked = dict(chunk_frames=args.chunk, overlap_frames=args.overlap)
    findc_ms, b = wall(torch, lambda: find_phrases([hour], [phrase], min_score=-10.0, max_hits=256, **chunked), max(3, args.steps // 3))
    res["hour"] = {"frames": T, "vocab": Vh, "labels": int(phrase.size), "hour_ms": round(hour_ms, 3), "hour_ms_min": round(hour_min, 3),
                   "hour_ms_max": round(hour_max, 3), "hour_ns_step": round(hour_ms * 1e6 / T, 2), "chunk": args.chunk,
                   "overlap": args.overlap, "pieces": len(plan), "hour_chunked_ms": round(chunk_ms, 3),
                   "hour_chunked_ms_min": round(chunk_min, 3), "hour_chunked_ms_max": round(chunk_max, 3),
                   "find_ms": round(find_ms, 3), "find_chunked_ms": round(findc_ms, 3), "planted": int(at.numel()), "hits_whole": len(a[0]), "hits_chunked": len(b[0]),
                   "same_hits": [h[:4] for h in a[0]] == [h[:4] for h in b[0]]}
    print(json.dumps(res))
    if args.out:
        h = res["hour"]
        rows = [("packed fp32 forward of the set (for scale)", f"{res['packed_ms']} ms"),
                (f"term list: {res['pairs']} pairs ({n} recordings x {res['phrases']} phrases of 3-20 labels), one call",
                 f"{res['list_ms']} ms (min {res['list_ms_min']}, max {res['list_ms_max']})"),
                ("... per frame step of a pair", f"{res['list_ns_step']} ns"),
                ("... over the forward", f"{res['over_packed']}"),
                (f"one phrase ({h['labels']} labels) over {h['frames']} frames, whole (one wave)",
                 f"{h['hour_ms']} ms (min {h['hour_ms_min']}, max {h['hour_ms_max']})"),
                ("... per frame step", f"{h['hour_ns_step']} ns"),
                (f"... as {h['pieces']} pieces (chunk {h['chunk']}, overlap {h['overlap']})",
                 f"{h['hour_chunked_ms']} ms (min {h['hour_chunked_ms_min']}, max {h['hour_chunked_ms_max']})"),
                ("find_phrases from Python, whole / chunked (wall clock)", f"{h['find_ms']} / {h['find_chunked_ms']} ms"),
                (f"hits whole / chunked ({h['planted']} planted), equal", f"{h['hits_whole']} / {h['hits_chunked']}, {h['same_hits']}")]
        with open(args.out, "w") as f:
            f.write("# CTC phrase search (w2v2_ctc_spot): measured times\n\n")
            f.write(f"`python tools/spot_bench.py --out {os.path.basename(args.out)}` on one MI355X; {res['n']} recordings, "
                    f"{res['audio_s']} s of audio, {res['frames']} frames, vocabulary {res['vocab']}; HIP events, median of "
                    f"{args.steps} calls.\n\n| what | time |\n|---|---|\n")
            for k, v in rows:
                f.write(f"| {k} | {v} |\n")
            f.write("\n```json\n" + json.dumps(res) + "\n```\n")


if __name__ == "__main__":
    main()
