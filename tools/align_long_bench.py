#!/usr/bin/env python
"""Time of the forced alignment of one whole recording (w2v2_ctc_align_long) over a grid of tile geometries.

One synthetic hour of read speech: 180 000 frames, V = 32, 54 000 labels (15 per second).  The logits are peaky around a seeded
frame path (every label at least one frame, a blank behind it, the other frames dealt out at random), so the best path is known:
it is the planted one, and every timed geometry is checked against it.  Per geometry (strips of --strips pairs x panels of
--panels frames) one JSON line:

  launches        kernels enqueued by the call: lse, init, one per anti-diagonal of tiles, finish
  workspace       bytes of library scratch (w2v2_ctc_align_long_workspace)
  ms              one w2v2_ctc_align_long call (HIP events around the call; labels already on the device), median and min
  us_per_step     ms / ((panels + strips) * panel_frames): the time per sequential step of the diagonal schedule, next to the
                  0.415 us per step of the one-block aligner (profiles/align.md)
  path_ok         the path equals the planted one
  star_*          the star row (w2v2_ctc_align_long_star): star_same_labels_ms is the star entry point on the very
                  same star-free labels (star_same_labels_path_ok: it finds the planted path too); star_ms on the transcript in which
                  every --star-every-th word (a word: 5 labels) is replaced by one star

and at the end the geometry with the smallest median and the hour's budget: the forward that produces the logits of the hour
takes 0.57 s.

    python tools/align_long_bench.py [--frames 180000] [--labels 54000] [--strips 1024,2048,8192] [--panels 512,1024,2048]
                                     [--steps 3] [--warmup 1] [--default] [--star-every 20] [--star-score -0.5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))

ONE_BLOCK_US_PER_STEP = 0.415       # profiles/align.md
FORWARD_S_PER_HOUR = 0.57


def planted(rng, T, U, V, blank):
    """(logits (T, V) fp32, labels (U), path (T)): label k holds 1 + a_k frames, then 1 + b_k blanks"""
    labels = rng.integers(1, V, size=U)
    labels[labels == blank] = (blank + 1) % V
    extra = rng.multinomial(T - 2 * U, np.full(2 * U, 1.0 / (2 * U))) + 1
    tokens = np.empty(2 * U, np.int64)
    tokens[0::2] = labels
    tokens[1::2] = blank
    path = np.repeat(tokens, extra)
    assert path.size == T
    x = rng.standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), path] += 12.0
    return x, labels.astype(np.int32), path.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=180000)
    ap.add_argument("--labels", type=int, default=54000)
    ap.add_argument("--vocab", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--strips", default="1024,2048,8192")
    ap.add_argument("--panels", default="512,1024,2048")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--default", action="store_true", help="time the library's default geometry (0, 0) as well")
    ap.add_argument("--star-every", type=int, default=20, help="every this many words one becomes a star (0: no star row)")
    ap.add_argument("--star-score", type=float, default=-0.5)
    args = ap.parse_args()

    import torch
    from wav2vec2 import _native as N
    torch.cuda.set_device(0)
    T, U, V, blank = args.frames, args.labels, args.vocab, 0
    x, labels, path = planted(np.random.default_rng(args.seed), T, U, V, blank)
    base = torch.from_numpy(x).cuda()
    lab_dev = torch.from_numpy(labels).cuda()
    want = torch.from_numpy(path).cuda()
    row0, label0 = np.zeros(1, np.int64), np.zeros(1, np.int64)
    frames_h, nlab_h = np.asarray([T], np.int32), np.asarray([U], np.int32)
    tok = torch.empty(T, dtype=torch.int32, device="cuda")
    li = torch.empty_like(tok)
    flp = torch.empty(T, dtype=torch.float32, device="cuda")
    sc = torch.empty(1, dtype=torch.float64, device="cuda")
    lib = N.load()
    if args.star_every:
        WORD = 5
        slabels = np.concatenate([np.asarray([V], np.int32) if (w // WORD) % args.star_every == args.star_every - 1 else labels[w:w + WORD]
                                  for w in range(0, U, WORD)])
        slab_dev = torch.from_numpy(slabels).cuda()
        snlab_h = np.asarray([slabels.size], np.int32)

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in ev)

    grid = [(int(s), int(p)) for s in args.strips.split(",") for p in args.panels.split(",")]
    if args.default:
        grid.append((0, 0))
    rows = []
    for sp, pf in grid:
        def call():
            N.check(lib.w2v2_ctc_align_long(N.ptr(base), V, 1, N.ptr(row0), N.ptr(frames_h), N.ptr(lab_dev), N.ptr(label0),
                                            N.ptr(nlab_h), blank, N.ptr(tok), N.ptr(li), N.ptr(flp), N.ptr(sc), sp, pf, 0,
                                            N.current_stream()), "w2v2_ctc_align_long")

        def star_call(ld, nl):
            N.check(lib.w2v2_ctc_align_long_star(N.ptr(base), V, 1, N.ptr(row0), N.ptr(frames_h), N.ptr(ld), N.ptr(label0), N.ptr(nl),
                                                 blank, args.star_score, N.ptr(tok), N.ptr(li), N.ptr(flp), N.ptr(sc), sp, pf, 0,
                                                 N.current_stream()), "w2v2_ctc_align_long_star")

        star = {}
        if args.star_every:
            st = timed(lambda: star_call(slab_dev, snlab_h))
            star_frames = int((tok == V).sum().item())
            tok.fill_(-7)
            ss = timed(lambda: star_call(lab_dev, nlab_h))
            star = {"stars": int((slabels == V).sum()), "star_frames": star_frames, "star_ms": round(float(np.median(st)), 2),
                    "star_ms_min": round(st[0], 2), "star_same_labels_ms": round(float(np.median(ss)), 2),
                    "star_same_labels_ms_min": round(ss[0], 2), "star_same_labels_path_ok": bool(torch.equal(tok, want))}
        tok.fill_(-7)
        ms = timed(call)
        res = {"strip_pairs": sp, "panel_frames": pf,
               "workspace": int(lib.w2v2_ctc_align_long_workspace(1, N.ptr(frames_h), N.ptr(nlab_h), sp, pf)),
               "ms": round(float(np.median(ms)), 2), "ms_min": round(ms[0], 2), "path_ok": bool(torch.equal(tok, want)),
               "score": float(sc.cpu()[0])}
        if sp:
            strips, panels = -(-(U + 1) // sp), -(-(T - 1) // pf)
            res.update(strips=strips, panels=panels, launches=strips + panels - 1 + 3,
                       us_per_step=round(res["ms"] * 1e3 / ((panels + strips) * pf), 3))
        res.update(star)
        rows.append(res)
        print(json.dumps(res), flush=True)
    best = min((r for r in rows if r["strip_pairs"]), key=lambda r: r["ms"])
    print(json.dumps({"frames": T, "labels": U, "vocab": V, "best_strip_pairs": best["strip_pairs"],
                      "best_panel_frames": best["panel_frames"], "best_ms": best["ms"],
                      "one_block_us_per_step": ONE_BLOCK_US_PER_STEP, "forward_ms_per_hour": FORWARD_S_PER_HOUR * 1e3,
                      "under_the_forward": best["ms"] < FORWARD_S_PER_HOUR * 1e3 * T / 180000.0,
                      "all_paths_ok": all(r["path_ok"] for r in rows)}))


if __name__ == "__main__":
    main()
