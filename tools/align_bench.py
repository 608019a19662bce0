#!/usr/bin/env python
"""Time of the CTC forced alignment (w2v2_ctc_align) on tools/packed_bench.py's utterance set: 64 seeded lengths of 1.5-35 s through
the base Wav2Vec2ForCTC (seeded weights, fp32) as one predict_packed call, each utterance aligned to a seeded synthetic
transcript of about --labels-per-s labels per second of audio, with a share --repeat of letters equal to the one before
(doubled letters; each costs the path one more frame).  Reports, as one JSON line:

  kernel_ms     one w2v2_ctc_align call on the packed views (HIP events around the call; labels already on the device)
  us_per_step   kernel_ms over the frame count of the longest utterance (the sweep is sequential in frames)
  call_ms       one forced_align() call from Python (label checks, label upload, the kernels, the score copy back)
  ref_ms        the fp64 numpy reference (tests/align_reference.py) over the same set, on the host
  packed_ms     the packed fp32 forward of the set, for scale
  star_*        the star row (w2v2_ctc_align_star): star_same_labels_kernel_ms is the star entry point on the very
                same star-free labels; star_kernel_ms on the transcripts in which every --star-every-th word (a word: 5 labels)
                is replaced by one star

    python tools/align_bench.py [--n 64] [--steps 20] [--warmup 3] [--labels-per-s 15] [--repeat 0.03] [--ref-n 64]
                                [--star-every 20] [--star-score -0.5]
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


def transcript(rng, U, V, blank, repeat):
    out = []
    letters = [v for v in range(V) if v != blank]
    for _ in range(U):
        if out and rng.random() < repeat:
            out.append(out[-1])
        else:
            out.append(int(rng.choice([v for v in letters if not out or v != out[-1]])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--labels-per-s", type=float, default=15.0)
    ap.add_argument("--repeat", type=float, default=0.03)
    ap.add_argument("--ref-n", type=int, default=64, help="utterances the host reference is timed on (0: skip)")
    ap.add_argument("--star-every", type=int, default=20, help="every this many words one becomes a star (0: no star row)")
    ap.add_argument("--star-score", type=float, default=-0.5)
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base, forced_align
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
    for _ in range(3):
        t0 = time.perf_counter()
        logits = m.predict_packed(waves)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    packed_ms = float(np.median(t)) * 1e3

    trng = np.random.default_rng(args.seed + 1)
    frames = [int(l.shape[0]) for l in logits]
    labels = []
    for n, T in zip(lens, frames):
        U = int(round(args.labels_per_s * n / SR))
        lab = transcript(trng, U, cfg.vocab_size, cfg.pad_id, args.repeat)
        while len(lab) + int(sum(a == b for a, b in zip(lab[1:], lab[:-1]))) > T:
            lab = lab[:-1]
        labels.append(lab)

    # the C ABI alone on the packed views, labels resident
    base, row0, fl = _logits_base(logits, None)
    n = len(frames)
    flat = np.concatenate([np.asarray(l, np.int32) for l in labels])
    lab_dev = torch.from_numpy(flat).cuda()
    label0 = np.cumsum([0] + [len(l) for l in labels[:-1]]).astype(np.int64)
    nlab = np.asarray([len(l) for l in labels], np.int32)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    tot = sum(frames)
    tok = torch.empty(tot, dtype=torch.int32, device="cuda")
    li = torch.empty_like(tok)
    flp = torch.empty(tot, dtype=torch.float32, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    lib = N.load()

    def kernel():
        N.check(lib.w2v2_ctc_align(N.ptr(base), cfg.vocab_size, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(lab_dev), N.ptr(label0),
                                   N.ptr(nlab), cfg.pad_id, N.ptr(tok), N.ptr(li), N.ptr(flp), N.ptr(sc), N.current_stream()))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in ev)

    kt = timed(kernel)
    kernel_ms = float(np.median(kt))

    # the star row: the star entry point on the same labels, and on transcripts with every star_every-th word a star
    star = {}
    if args.star_every:
        WORD = 5
        slabels = []
        for l in labels:
            out = []
            for w in range(0, len(l), WORD):
                out.extend([cfg.vocab_size] if (w // WORD) % args.star_every == args.star_every - 1 else l[w:w + WORD])
            slabels.append(out)
        sflat = np.concatenate([np.asarray(l, np.int32) for l in slabels])
        slab_dev = torch.from_numpy(sflat).cuda()
        slabel0 = np.cumsum([0] + [len(l) for l in slabels[:-1]]).astype(np.int64)
        snlab = np.asarray([len(l) for l in slabels], np.int32)

        def star_kernel(ld, l0, nl):
            N.check(lib.w2v2_ctc_align_star(N.ptr(base), cfg.vocab_size, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(ld), N.ptr(l0), N.ptr(nl),
                                            cfg.pad_id, args.star_score, N.ptr(tok), N.ptr(li), N.ptr(flp), N.ptr(sc), N.current_stream()))

        st = timed(lambda: star_kernel(slab_dev, slabel0, snlab))
        star_frames = int((tok == cfg.vocab_size).sum().item())
        ss = timed(lambda: star_kernel(lab_dev, label0, nlab))
        star = {"stars": int((sflat == cfg.vocab_size).sum()), "star_labels": int(snlab.sum()), "star_frames": star_frames,
                "star_kernel_ms": round(float(np.median(st)), 3), "star_kernel_ms_min": round(st[0], 3),
                "star_same_labels_kernel_ms": round(float(np.median(ss)), 3), "star_same_labels_kernel_ms_min": round(ss[0], 3)}
        kernel()                                                 # (tok below: the star-free paths)

    ct = []
    for _ in range(max(3, args.steps // 4)):
        t0 = time.perf_counter()
        forced_align(logits, labels, blank=cfg.pad_id)
        ct.append(time.perf_counter() - t0)
    call_ms = float(np.median(ct)) * 1e3

    res = {"n": n, "audio_s": round(float(lens.sum()) / SR, 2), "frames": tot, "max_frames": max(frames),
           "labels": int(nlab.sum()), "max_labels": int(nlab.max()),
           "repeats": int(sum(sum(a == b for a, b in zip(l[1:], l[:-1])) for l in labels)),
           "kernel_ms": round(kernel_ms, 3), "kernel_ms_min": round(kt[0], 3),
           "us_per_step": round(kernel_ms * 1e3 / max(frames), 3), "call_ms": round(call_ms, 3),
           "packed_ms": round(packed_ms, 2), "align_over_packed": round(kernel_ms / packed_ms, 4), "target_ms": 2.0}
    res.update(star)
    if args.ref_n:
        import align_reference as AR
        hosts = [l.cpu().numpy() for l in logits[:args.ref_n]]
        t0 = time.perf_counter()
        refs = [AR.viterbi(h, l, cfg.pad_id) for h, l in zip(hosts, labels)]
        res["ref_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["ref_n"] = len(hosts)
        got = tok.cpu().numpy()
        o, same = 0, True
        for h, r in zip(hosts, refs):
            same &= bool(np.array_equal(got[o:o + h.shape[0]], r[0]))
            o += h.shape[0]
        res["paths_equal_reference"] = same
    print(json.dumps(res))


if __name__ == "__main__":
    main()
