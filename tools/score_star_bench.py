#!/usr/bin/env python
"""Time of the star entry points of the exact CTC scorer and its gradient (w2v2_ctc_score_star, w2v2_ctc_score_grad_star; DESIGN.md
§24) next to the star-free ones, on tools/score_bench.py's 1024 (utterance, hypothesis) pairs: 64 seeded lengths of 1.5-35 s through
the base Wav2Vec2ForCTC (seeded weights, fp32) as one predict_packed call, decoded at beam width 16 with nbest 16.  The four arms run
on the SAME star-free labels, one after the other within a round, --rounds rounds, the order rotating from round to round; a fifth
and sixth arm run the star entry points on labels with every --every-th label replaced by the star.  Reports, as one JSON line, per
arm the median, minimum and maximum of the rounds' medians (HIP events; labels already on the device), the ratios star / star-free,
the pairs per thread layout (P), and whether the star entry points gave the star-free bits.  --layouts adds the four arms on one synthetic set per thread layout (32 pairs
of 200, 400, 800 and 2049 labels on 2U + 50 frames: 1, 2, 4 and 8 pairs per thread), which the beam lists do not separate.

    python tools/score_star_bench.py [--n 64] [--steps 10] [--warmup 2] [--rounds 5] [--every 10] [--layouts]
"""
import argparse
import json
import os
import sys

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
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--nbest", type=int, default=16)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--star-score", type=float, default=-0.5)
    ap.add_argument("--layouts", action="store_true", help="also time each thread layout alone on a synthetic set")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import beam_search
    torch.cuda.set_device(0)
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    rng = np.random.default_rng(args.seed)                       # the packed_bench set
    lens = rng.integers(int(args.min_s * SR), int(args.max_s * SR) + 1, size=args.n)
    waves = [torch.randn(int(n), device="cuda") for n in lens]
    logits = m.predict_packed(waves)
    vs, blank, ss = cfg.vocab_size, cfg.pad_id, float(args.star_score)
    base, row0, fl = _logits_base(logits, None)
    n = len(fl)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    lib = N.load()
    hyps = beam_search(logits, beam_width=args.width, nbest=args.nbest, blank=blank)
    pairs = [(i, h) for i, hs in enumerate(hyps) for h in hs]
    utt = np.asarray([i for i, _ in pairs], np.int32)
    nlab = np.asarray([len(h.ids) for _, h in pairs], np.int32)
    label0 = np.concatenate(([0], np.cumsum(nlab[:-1], dtype=np.int64))).astype(np.int64)
    flat = np.concatenate([np.asarray(h.ids, np.int32) for _, h in pairs] + [np.zeros(1, np.int32)])
    planted = flat.copy()
    for l0, nl in zip(label0, nlab):                             # every --every-th label of a pair becomes the star (never two in a row)
        planted[l0 + args.every // 2:l0 + nl:max(2, args.every)] = vs
    lab_dev, planted_dev = torch.from_numpy(flat).cuda(), torch.from_numpy(planted).cuda()
    mp = len(pairs)
    coef = torch.from_numpy(rng.standard_normal(mp)).cuda()
    out = {k: torch.empty(mp, dtype=torch.float64, device="cuda") for k in ("score", "score_star", "grad", "grad_star", "planted")}
    g0, g1 = torch.zeros_like(base), torch.zeros_like(base)
    common = (N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), mp, N.ptr(utt))
    stream = N.current_stream()

    def score():
        N.check(lib.w2v2_ctc_score(*common, N.ptr(lab_dev), N.ptr(label0), N.ptr(nlab), blank, N.ptr(out["score"]), stream))

    def score_star(lab=lab_dev, key="score_star"):
        N.check(lib.w2v2_ctc_score_star(*common, N.ptr(lab), N.ptr(label0), N.ptr(nlab), blank, ss, N.ptr(out[key]), stream))

    def grad():
        N.check(lib.w2v2_ctc_score_grad(*common, N.ptr(lab_dev), N.ptr(label0), N.ptr(nlab), blank, N.ptr(coef), N.ptr(out["grad"]),
                                        N.ptr(g0), 0, stream))

    def grad_star(lab=lab_dev, key="grad_star"):
        N.check(lib.w2v2_ctc_score_grad_star(*common, N.ptr(lab), N.ptr(label0), N.ptr(nlab), blank, ss, N.ptr(coef), N.ptr(out[key]),
                                             N.ptr(g1), 0, stream))

    arms = {"score": score, "score_star": score_star, "grad": grad, "grad_star": grad_star,
            "score_star_planted": lambda: score_star(planted_dev, "planted"), "grad_star_planted": lambda: grad_star(planted_dev, "planted")}
    times = {k: [] for k in arms}
    names = list(arms)
    for r in range(args.rounds):                                 # the order rotates: no arm always follows the same one
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(timed(torch, arms[k], args.steps, args.warmup))
    grad()
    grad_star()
    torch.cuda.synchronize()
    same = bool((out["score"].view(torch.int64) == out["score_star"].view(torch.int64)).all()
                and (out["grad"].view(torch.int64) == out["grad_star"].view(torch.int64)).all()
                and (out["score"].view(torch.int64) == out["grad"].view(torch.int64)).all()
                and (g0.view(torch.int32) == g1.view(torch.int32)).all())
    P = np.where(nlab + 1 <= 256, 1, np.where(nlab + 1 <= 512, 2, np.where(nlab + 1 <= 1024, 4, 8)))
    res = {"n": n, "frames": int(sum(fl)), "vocab": vs, "pairs": mp, "labels_mean": round(float(nlab.mean()), 1), "labels_max": int(nlab.max()),
           "pairs_per_layout": {str(p): int((P == p).sum()) for p in (1, 2, 4, 8)}, "stars_planted": int((planted == vs).sum()),
           "rounds": args.rounds, "steps": args.steps, "star_free_bits": same}
    for k, t in times.items():
        res[k + "_ms"] = {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    res["score_star_over_score"] = round(float(np.median(times["score_star"]) / np.median(times["score"])), 4)
    res["grad_star_over_grad"] = round(float(np.median(times["grad_star"]) / np.median(times["grad"])), 4)
    if args.layouts:
        del g0, g1
        res["layouts"] = {str(p): layout_arm(torch, N, lib, p, U, ss, args) for p, U in ((1, 200), (2, 400), (4, 800), (8, 2049))}
    print(json.dumps(res))


def layout_arm(torch, N, lib, P, U, ss, args, pairs=32, V=32):
    """the four arms on a synthetic set of ONE thread layout: ``pairs`` utterances of 2U + 50 frames of N(0, 2) logits, one star-free
    pair of U labels each (a tenth of them repeats)"""
    rng = np.random.default_rng(100 + P)
    T = 2 * U + 50
    base = (torch.randn((pairs * T, V), device="cuda", generator=torch.Generator("cuda").manual_seed(P)) * 2).contiguous()
    lab = rng.integers(1, V, size=(pairs, U)).astype(np.int32)
    rep = rng.random((pairs, U)) < 0.1
    for k in range(1, U):
        lab[rep[:, k], k] = lab[rep[:, k], k - 1]
    lab_dev = torch.from_numpy(np.concatenate([lab.reshape(-1), np.zeros(1, np.int32)])).cuda()
    row0 = (np.arange(pairs, dtype=np.int64) * T)
    frames, utt, nlab = np.full(pairs, T, np.int32), np.arange(pairs, dtype=np.int32), np.full(pairs, U, np.int32)
    label0 = (np.arange(pairs, dtype=np.int64) * U)
    coef = torch.from_numpy(rng.standard_normal(pairs)).cuda()
    out = [torch.empty(pairs, dtype=torch.float64, device="cuda") for _ in range(4)]
    g = [torch.zeros_like(base), torch.zeros_like(base)]
    common = (N.ptr(base), V, pairs, N.ptr(row0), N.ptr(frames), pairs, N.ptr(utt), N.ptr(lab_dev), N.ptr(label0), N.ptr(nlab), 0)
    stream = N.current_stream()
    arms = {"score": lambda: N.check(lib.w2v2_ctc_score(*common, N.ptr(out[0]), stream)),
            "score_star": lambda: N.check(lib.w2v2_ctc_score_star(*common, ss, N.ptr(out[1]), stream)),
            "grad": lambda: N.check(lib.w2v2_ctc_score_grad(*common, N.ptr(coef), N.ptr(out[2]), N.ptr(g[0]), 0, stream)),
            "grad_star": lambda: N.check(lib.w2v2_ctc_score_grad_star(*common, ss, N.ptr(coef), N.ptr(out[3]), N.ptr(g[1]), 0, stream))}
    names, times = list(arms), {k: [] for k in arms}
    for r in range(args.rounds):
        for k in names[r % 4:] + names[:r % 4]:
            times[k].append(timed(torch, arms[k], max(3, args.steps // 2), 1))
    torch.cuda.synchronize()
    same = bool(all((o.view(torch.int64) == out[0].view(torch.int64)).all() for o in out[1:]) and (g[0].view(torch.int32) == g[1].view(torch.int32)).all())
    res = {"labels": U, "frames": T, "pairs": pairs, "star_free_bits": same}
    for k, t in times.items():
        res[k + "_ms"] = {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    res["score_star_over_score"] = round(float(np.median(times["score_star"]) / np.median(times["score"])), 4)
    res["grad_star_over_grad"] = round(float(np.median(times["grad_star"]) / np.median(times["grad"])), 4)
    return res


if __name__ == "__main__":
    main()
