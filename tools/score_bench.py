#!/usr/bin/env python
"""Time of the exact CTC scoring (w2v2_ctc_score) on tools/packed_bench.py's utterance set: 64 seeded lengths of 1.5-35 s through the
base Wav2Vec2ForCTC (seeded weights, fp32) as one predict_packed call, decoded at beam width 16 with nbest 16, and all 64 x 16 =
1024 (utterance, hypothesis) pairs scored in ONE call on the packed views.  Reports, as one JSON line:

  packed_ms     the packed fp32 forward of the set, measured in the same run
  beam_ms       one w2v2_ctc_beam_search call at width 16 / nbest 16 (HIP events; median of --steps)
  score_ms      one w2v2_ctc_score call over every pair (HIP events; median, min and max of --steps; labels already on the device)
  rescore_ms    one rescore() call from Python (label upload, the kernels, the copy back, the new Hypothesis lists)
  over_beam     score_ms / beam_ms: the scorer is meant to cost less than the search it follows
  gap           the largest and the mean of (exact - beam score) over the pairs: what the beam's lower bound leaves out
and, on the pairs the only other route can take (w2v2_ctc_loss holds at most 319 labels per row):
  loss_route    pairs, gather_ms (each pair's utterance copied into a padded (pairs, Tmax, V) batch on the device), loss_ms (one
                w2v2_ctc_loss call with a null gradient), route_ms (both), score_subset_ms (w2v2_ctc_score on the same pairs) and
                max_diff (largest |exact - (-nll)| over them; the loss is fp32)

    python tools/score_bench.py [--n 64] [--steps 10] [--warmup 2] [--width 16] [--nbest 16]
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
LOSS_MAX_LABELS = 319


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--nbest", type=int, default=16)
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import beam_search, rescore
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

    vs, blank, W, nbest = cfg.vocab_size, cfg.pad_id, args.width, args.nbest
    base, row0, fl = _logits_base(logits, None)
    n, max_len = len(fl), max(fl)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    lib = N.load()
    labels = torch.empty((n, nbest, max_len), dtype=torch.int32, device="cuda")
    length = torch.empty((n, nbest), dtype=torch.int32, device="cuda")
    score = torch.empty((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.empty((n, nbest), dtype=torch.float64, device="cuda")

    def beam():
        N.check(lib.w2v2_ctc_beam_search(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, nbest, None, 1, 0.0, 0.0, max_len,
                                         N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))

    beam_ms, _, _ = timed(torch, beam, args.steps, args.warmup)
    hyps = beam_search(logits, beam_width=W, nbest=nbest, blank=blank)
    pairs = [(i, h) for i, hs in enumerate(hyps) for h in hs]
    utt = np.asarray([i for i, _ in pairs], np.int32)
    nlab = np.asarray([len(h.ids) for _, h in pairs], np.int32)
    label0 = np.concatenate(([0], np.cumsum(nlab[:-1], dtype=np.int64))).astype(np.int64)
    flat = np.concatenate([np.asarray(h.ids, np.int32) for _, h in pairs] + [np.zeros(1, np.int32)])
    lab_dev = torch.from_numpy(flat).cuda()
    logp = torch.empty(len(pairs), dtype=torch.float64, device="cuda")

    def scorer(sel=None, out=logp):
        u, l0, nl = (utt, label0, nlab) if sel is None else (utt[sel], label0[sel], nlab[sel])
        N.check(lib.w2v2_ctc_score(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), len(u), N.ptr(u), N.ptr(lab_dev), N.ptr(l0),
                                   N.ptr(nl), blank, N.ptr(out), N.current_stream()))

    score_ms, score_min, score_max = timed(torch, scorer, args.steps, args.warmup)
    exact = logp.cpu().numpy()
    gap = exact - np.asarray([h.score for _, h in pairs])
    ct = []
    for _ in range(max(3, args.steps // 3)):
        t0 = time.perf_counter()
        rescore(logits, hyps, blank=blank)
        ct.append(time.perf_counter() - t0)
    res = {"n": n, "audio_s": round(float(lens.sum()) / SR, 2), "frames": int(sum(fl)), "max_frames": max_len, "vocab": vs, "beam_width": W,
           "nbest": nbest, "pairs": len(pairs), "labels_mean": round(float(nlab.mean()), 1), "labels_max": int(nlab.max()),
           "packed_ms": round(packed_ms, 2), "beam_ms": round(beam_ms, 3), "score_ms": round(score_ms, 3),
           "score_ms_min": round(score_min, 3), "score_ms_max": round(score_max, 3), "rescore_ms": round(float(np.median(ct)) * 1e3, 3),
           "over_beam": round(score_ms / beam_ms, 4), "over_packed": round(score_ms / packed_ms, 4),
           "gap": {"max": round(float(gap.max()), 4), "mean": round(float(gap.mean()), 4), "min": float(gap.min())}}

    # the only other route: a padded, replicated (pairs, Tmax, V) batch through w2v2_ctc_loss, for the pairs of at most 319 labels
    sel = np.flatnonzero(nlab <= LOSS_MAX_LABELS)
    if sel.size:
        B, Tm, Um = int(sel.size), int(max(fl[i] for i in utt[sel])), max(int(nlab[sel].max()), 1)
        lab_pad = np.full((B, Um), blank, np.int32)
        for r, j in enumerate(sel):
            lab_pad[r, :nlab[j]] = flat[label0[j]:label0[j] + nlab[j]]
        lab_pad_dev = torch.from_numpy(lab_pad).cuda()
        label_len = torch.from_numpy(nlab[sel].astype(np.int32)).cuda()
        logit_len = torch.from_numpy(np.asarray([fl[i] for i in utt[sel]], np.int32)).cuda()
        batch = torch.zeros((B, Tm, vs), dtype=torch.float32, device="cuda")
        nll = torch.empty(B, dtype=torch.float32, device="cuda")
        src = [logits[int(i)] for i in utt[sel]]

        def gather():
            for r, s in enumerate(src):
                batch[r, :s.shape[0]].copy_(s)

        def loss():
            N.check(lib.w2v2_ctc_loss(N.ptr(batch), B, Tm, vs, N.ptr(lab_pad_dev), Um, N.ptr(label_len), N.ptr(logit_len), blank,
                                      N.ptr(nll), None, N.current_stream()))

        def route():
            gather()
            loss()

        gather_ms, _, _ = timed(torch, gather, args.steps, args.warmup)
        loss_ms, _, _ = timed(torch, loss, args.steps, args.warmup)
        route_ms, _, _ = timed(torch, route, args.steps, args.warmup)
        sub = torch.empty(B, dtype=torch.float64, device="cuda")
        sub_ms, _, _ = timed(torch, lambda: scorer(sel, sub), args.steps, args.warmup)
        diff = np.abs(sub.cpu().numpy() + nll.cpu().numpy().astype(np.float64))
        res["loss_route"] = {"pairs": B, "max_frames": Tm, "max_labels": Um, "batch_mib": round(B * Tm * vs * 4 / 2 ** 20, 1),
                             "gather_ms": round(gather_ms, 3), "loss_ms": round(loss_ms, 3), "route_ms": round(route_ms, 3),
                             "score_subset_ms": round(sub_ms, 3), "over_route": round(sub_ms / route_ms, 4),
                             "max_diff": float(diff[np.isfinite(diff)].max()) if np.isfinite(diff).any() else None}
    else:
        res["loss_route"] = {"pairs": 0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
