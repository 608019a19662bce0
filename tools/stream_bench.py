#!/usr/bin/env python
"""Cost of streaming transcription, one GPU process, one JSON line.  The utterance set is tools/beam_bench.py's: 64
seeded lengths of 1.5-35 s through the base Wav2Vec2ForCTC (seeded weights, fp32) as one predict_packed call.

  unchanged   (i) w2v2_ctc_beam_search on that set at widths 1, 16, 64 and 16 with a 3-gram table, in this build and -- with
              --parent-lib, a libw2v2.so built from the parent commit and loaded beside this one -- in the parent's, the two
              alternating call by call (HIP events around each call).  Per configuration: the median of each, `parent_spread_ms` =
              the parent's own max - min over its calls, and `within` = |median - parent median| <= parent_spread_ms.
  chunked     (ii) the same set through BeamStream (64 streams, width 16, no model): one advance() of everything, and advance()
              calls of 50, 200 and 400 frames per stream, without results until a last call that returns them.  Host clock around
              each call (advance ends in a device-to-host copy): `one_call_ms` against `sum_ms`, the sum over the calls, with their
              number.  What resuming costs; not a gate.
  session     (iii) Wav2Vec2ForCTC.stream with 1, 8 and 64 streams, every stream fed --session-s seconds of noise in chunks of one
              second at the default window and margin.  Host clock around each feed(): median and worst over all feeds, the same
              over the feeds that ran a window (`busy_`), and `audio_s_per_s` = all audio fed / all time spent in feed().

    python tools/stream_bench.py [--steps 20] [--warmup 3] [--parent-lib lib/libw2v2_parent.so] [--session-s 30]
"""
import argparse
import ctypes
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="a libw2v2.so built from the parent commit")
    ap.add_argument("--session-s", type=float, default=30.0)
    ap.add_argument("--session-streams", default="1,8,64")
    args = ap.parse_args()
    if args.parent_lib and not os.path.exists(args.parent_lib):
        ap.error(f"--parent-lib {args.parent_lib} does not exist")

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import BeamStream, CharNgramLM, beam_search
    from wav2vec2.processor import Wav2Vec2Processor
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench: no HIP device; nothing is measured without one")
    torch.cuda.set_device(0)
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    rng = np.random.default_rng(args.seed)                       # the packed_bench / beam_bench set
    lens = rng.integers(int(args.min_s * SR), int(args.max_s * SR) + 1, size=args.n)
    waves = [torch.randn(int(n), device="cuda") for n in lens]
    logits = m.predict_packed(waves)
    torch.cuda.synchronize()
    vs, blank = cfg.vocab_size, cfg.pad_id
    lrng = np.random.default_rng(args.seed + 2)
    letters = [v for v in range(vs) if v != blank]
    lm3 = CharNgramLM.from_ids([lrng.choice(letters, size=200).tolist() for _ in range(50)], vs, blank, order=3, add_k=0.5,
                               alpha=0.5, beta=0.1)
    base, row0, fl = _logits_base(logits, None)
    n, max_len = len(fl), max(fl)
    res = {"n": n, "audio_s": round(float(lens.sum()) / SR, 2), "frames": sum(fl), "max_frames": max_len}

    # ---- (i) the unchanged search, this build and the parent's, alternating ----
    libs = {"this": N.load()}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        rt, at = N.PROTOTYPES["w2v2_ctc_beam_search"]
        parent.w2v2_ctc_beam_search.restype, parent.w2v2_ctc_beam_search.argtypes = rt, at
        parent.w2v2_version.restype = ctypes.c_char_p
        libs["parent"] = parent
        res["parent_version"] = parent.w2v2_version().decode()
    res["version"] = libs["this"].w2v2_version().decode()
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    out = {k: (torch.empty((n, 1, max_len), dtype=torch.int32, device="cuda"), torch.empty((n, 1), dtype=torch.int32, device="cuda"),
               torch.empty((n, 1), dtype=torch.float64, device="cuda"), torch.empty((n, 1), dtype=torch.float64, device="cuda")) for k in libs}
    res["unchanged"] = []
    for W, lm in [(1, None), (16, None), (64, None), (16, lm3)]:
        table = lm.device_table(base.device) if lm is not None else None

        def kernel(k):
            labels, length, score, total = out[k]
            rc = libs[k].w2v2_ctc_beam_search(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, 1, N.ptr(table),
                                              lm.order if lm else 1, lm.alpha if lm else 0.0, lm.beta if lm else 0.0, max_len,
                                              N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream())
            if rc:
                raise RuntimeError(f"w2v2_ctc_beam_search ({k}) failed: {rc}")

        for _ in range(args.warmup):
            for k in libs:
                kernel(k)
        torch.cuda.synchronize()
        ev = {k: [] for k in libs}
        for _ in range(args.steps):
            for k in libs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                kernel(k)
                b.record()
                ev[k].append((a, b))
        torch.cuda.synchronize()
        ms = {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
        c = {"beam_width": W, "lm_order": lm.order if lm else 0, "this_ms": round(float(np.median(ms["this"])), 3),
             "this_min_max_ms": [round(ms["this"][0], 3), round(ms["this"][-1], 3)]}
        if "parent" in libs:
            spread = ms["parent"][-1] - ms["parent"][0]
            c.update(parent_ms=round(float(np.median(ms["parent"])), 3), parent_min_max_ms=[round(ms["parent"][0], 3), round(ms["parent"][-1], 3)],
                     parent_spread_ms=round(spread, 3),
                     within=bool(abs(float(np.median(ms["this"])) - float(np.median(ms["parent"]))) <= spread),
                     same_bits=all(bool(torch.equal(x, y)) for x, y in zip(out["this"][:2], out["parent"][:2]))
                     and bool(torch.equal(out["this"][2].view(torch.int64), out["parent"][2].view(torch.int64))))
        res["unchanged"].append(c)

    # ---- (ii) chunked against whole ----
    W = 16
    ct = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = beam_search(logits, beam_width=W, nbest=1, blank=blank)
        ct.append(time.perf_counter() - t0)
    res["chunked"] = {"beam_width": W, "beam_search_call_ms": round(float(np.median(ct)) * 1e3, 3), "runs": []}
    for chunk in (None, 50, 200, 400):
        reps = []
        for _ in range(3):
            s = BeamStream(n, vs, beam_width=W, nbest=1, blank=blank, initial_frames=2048)
            pos, times = [0] * n, []
            while any(p < T for p, T in zip(pos, fl)):
                parts = []
                for i, l in enumerate(logits):
                    c = fl[i] if chunk is None else chunk
                    parts.append(l[pos[i]:pos[i] + c] if pos[i] < fl[i] else None)
                    pos[i] = min(fl[i], pos[i] + c)
                last = chunk is None or not any(p < T for p, T in zip(pos, fl))
                t0 = time.perf_counter()
                steps = s.advance(parts, results=last)
                times.append(time.perf_counter() - t0)
            reps.append((sum(times), len(times)))
            same = all([h.ids for h in st.hypotheses] == [h.ids for h in w] for st, w in zip(steps, want))
        best = sorted(reps)[len(reps) // 2]
        key = "one_call_ms" if chunk is None else "sum_ms"
        res["chunked"]["runs"].append({"chunk_frames": chunk or max_len, key: round(best[0] * 1e3, 3), "calls": best[1], "equal_offline": same})

    # ---- (iii) a session ----
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(ROOT, "tests", "golden", "vocab.json"))
    res["session"] = []
    for ns in [int(v) for v in args.session_streams.split(",")]:
        srng = np.random.default_rng(args.seed + 7)
        audio = [torch.from_numpy(srng.standard_normal(int(args.session_s * SR)).astype(np.float32)).cuda() for _ in range(ns)]
        runs = []
        for rep in range(2):                                     # the first pass warms every shape up
            s = m.stream(tok, n_streams=ns)
            times, busy = [], []
            for a in range(0, int(args.session_s * SR), SR):
                done = list(s.done_windows)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.feed([w[a:a + SR] for w in audio])
                dt = time.perf_counter() - t0
                times.append(dt)
                if s.done_windows != done:
                    busy.append(dt)
            t0 = time.perf_counter()
            s.finish()
            runs.append((times, busy, time.perf_counter() - t0))
        times, busy, fin = runs[-1]
        res["session"].append({"streams": ns, "feeds": len(times), "feed_median_ms": round(float(np.median(times)) * 1e3, 3),
                               "feed_worst_ms": round(max(times) * 1e3, 3), "busy_feeds": len(busy),
                               "busy_median_ms": round(float(np.median(busy)) * 1e3, 3) if busy else None,
                               "finish_ms": round(fin * 1e3, 3),
                               "audio_s_per_s": round(ns * args.session_s / sum(times), 1),
                               "window_s": s.window / SR, "margin_s": s.margin / SR})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
