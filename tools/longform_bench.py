#!/usr/bin/env python
"""Time of the long-recording path on one seeded recording of --seconds (default 3600 s), base Wav2Vec2ForCTC with
seeded weights, fp32.  Reports one JSON line.

Part one, the forward:
  long_ms       predict_long(recording): 20 s windows with 2 s margins, gathered and normalised on the device, in packed calls of
                at most 1200 s of stream (median, min and max of --steps)
  packed_ms     the closest thing the library had before: the same audio cut on the host into 20 s utterances (no overlap, so
                window / (window - 2 margin) = 1.25 x less work) through predict_packed in calls of 1200 s
Part two, the decoding, on seeded peaky logits of the recording's frame count with a planted pause about every 8 s
(tests/longform_reference.py: peaky_logits):
  cuts_ms       one w2v2_ctc_pause_cuts call over the whole recording (HIP events), and the pauses it finds
  whole_ms      w2v2_ctc_beam_search over the recording as ONE utterance (what a caller without this layer would run): one block
  segments_ms   the same search over decode_long's segments in one call, one block each
  decode_ms     decode_long() from Python, everything included (cuts, choice, search, the copies back)

    python tools/longform_bench.py [--seconds 3600] [--steps 3] [--warmup 1] [--beam-width 16] [--skip-forward] [--skip-whole]
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


def wall(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(float(np.median(t)), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--window-s", type=float, default=20.0)
    ap.add_argument("--margin-s", type=float, default=2.0)
    ap.add_argument("--max-stream-s", type=float, default=1200.0)
    ap.add_argument("--beam-width", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-whole", action="store_true", help="skip the search over the recording as one utterance (seconds)")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.decoding import beam_search
    from wav2vec2.longform import choose_cuts, decode_long, group_windows, pause_cuts, seconds_to_samples, window_plan
    import longform_reference as R
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    cfg = wav2vec2.Wav2Vec2Config()
    L = int(args.seconds * SR)
    T = cfg.num_frames(L)
    res = {"audio_s": args.seconds, "frames": T, "window_s": args.window_s, "margin_s": args.margin_s,
           "max_stream_s": args.max_stream_s}

    if not args.skip_forward:
        m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
        m.set_weights(V.seeded_weights(cfg, seed=1))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(args.seed)
        wave = torch.randn(L, device="cuda", generator=gen)
        window, margin = seconds_to_samples(args.window_s, args.margin_s, cfg)
        plan = window_plan(L, window, margin, cfg)
        res["windows"] = len(plan)
        res["long_calls"] = len(group_windows(plan, int(args.max_stream_s * SR), cfg))
        res["long"] = wall(lambda: m.predict_long(wave, args.window_s, args.margin_s, True, args.max_stream_s), args.steps,
                           args.warmup, sync)
        # the parent's closest equivalent: 20 s utterances, normalised per utterance by torch on the device, packed calls of 1200 s
        pieces = [wave[a:a + window] for a in range(0, L, window) if L - a >= 400]
        per_call = max(1, int(args.max_stream_s * SR) // window)

        def packed():
            out = []
            for i in range(0, len(pieces), per_call):
                group = [(p - p.mean()) / torch.sqrt(p.var(unbiased=False) + 1e-5) for p in pieces[i:i + per_call]]
                out.append(m.predict_packed(group))
            return out

        res["packed_utterances"] = len(pieces)
        res["packed"] = wall(packed, args.steps, args.warmup, sync)
        res["long_over_packed"] = round(res["long"]["ms"] / res["packed"]["ms"], 3)
        del m, wave, pieces

    # ---- decoding on planted logits ----
    vs, blank, delim, min_pause = cfg.vocab_size, cfg.pad_id, 4, 10
    rng = np.random.default_rng(args.seed + 1)
    x, _ = R.peaky_logits(rng, T, vs, blank, delim, min_pause, n_pauses=max(2, int(args.seconds / 8.0)),
                          letters=[v for v in range(5, vs)])
    logits = torch.from_numpy(x).cuda()
    lib = N.load()
    max_cuts = T // (min_pause + 1) + 1
    cut = torch.empty((1, max_cuts), dtype=torch.int32, device="cuda")
    pause = torch.empty((1, max_cuts), dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    row0_h, frames_h = np.zeros(1, np.int64), np.array([T], np.int32)

    def cuts_kernel():
        N.check(lib.w2v2_ctc_pause_cuts(N.ptr(logits), vs, 1, N.ptr(row0_h), N.ptr(frames_h), blank, delim, 2.0, min_pause, max_cuts,
                                        N.ptr(cut), N.ptr(pause), N.ptr(count), N.current_stream()))

    def events(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        sync()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        sync()
        t = sorted(a.elapsed_time(b) for a, b in ev)
        return {"ms": round(float(np.median(t)), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}

    res["cuts"] = events(cuts_kernel, max(args.steps, 5), args.warmup)
    found = pause_cuts([logits], blank=blank, delimiter_id=delim, margin=2.0, min_pause=min_pause)[0]
    chosen = choose_cuts(found.cuts, found.pauses, T)
    b = [0] + chosen + [T]
    sizes = [e - s for s, e in zip(b, b[1:])]
    res["pauses"] = found.count
    res["segments"] = len(sizes)
    res["segment_frames"] = [int(min(sizes)), int(np.median(sizes)), int(max(sizes))]
    segs = list(torch.split(logits, sizes))
    W = args.beam_width
    res["beam_width"] = W
    res["segments_search"] = wall(lambda: beam_search(segs, beam_width=W, blank=blank), args.steps, args.warmup, sync)
    res["decode_long"] = wall(lambda: decode_long(logits, None, beam_width=W, blank=blank, delimiter_id=delim, min_pause=min_pause),
                              args.steps, args.warmup, sync)
    if not args.skip_whole:
        res["whole_search"] = wall(lambda: beam_search([logits], beam_width=W, blank=blank), max(1, args.steps - 1), 1, sync)
        res["whole_over_segments"] = round(res["whole_search"]["ms"] / res["segments_search"]["ms"], 2)
        whole = beam_search([logits], beam_width=W, blank=blank)[0][0].ids
        pieces = beam_search(segs, beam_width=W, blank=blank)
        res["same_transcript"] = list(whole) == [i for h in pieces for i in h[0].ids]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
