#!/usr/bin/env python
"""Time of the edit distance kernel (w2v2_edit_distance) on two seeded cases, no model download:

  wer   2939 word-level pairs with LibriSpeech-like lengths (test-clean has 2939 utterances): a reference of 3-80 words
        (mean about 20) over a 8000-word vocabulary, the hypothesis a copy with about 8 % of the words substituted, deleted or
        inserted -- what wav2vec2.metrics.wer does to a corpus.
  mbr   64 utterances x 64 hypotheses at character level, about 300 characters each, every hypothesis a 3 % mutation of its
        utterance's text; all 64 x 63 / 2 pairs of all utterances in one call -- what wav2vec2.metrics.mbr_select does.

Per case, as one JSON object: kernel_ms (HIP events around one w2v2_edit_distance call, tokens resident: the table upload and
the launches), cells and cells per second (m x n per pair), call_ms (the Python entry point end to end: pooling, upload, kernel,
copy back, EditCounts), ref (a numpy anti-diagonal implementation on the host, on the first --ref-pairs pairs; its results must
equal the kernel's), and the share the metric adds to transcribing the same number of utterances: transcribe_ms is one
Wav2Vec2ForCTC.transcribe call on tools/packed_bench.py's 64 seeded utterances (base model, seeded weights, fp32; beam 16 and
nbest 1 for wer, beam 64 and nbest 64 for mbr), scaled by utterances / 64.

    python tools/edit_bench.py [--steps 20] [--warmup 3] [--ref-pairs 300] [--no-transcribe] [--out profiles/edit_distance.md]
"""
import argparse
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))

SR = 16000


def source_hash():
    """sha256 over csrc/*.hip + *.h, as tools/prof_summary.py's provenance line"""
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "gsoc-wav2vec2_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "gsoc-wav2vec2_amd", "csrc", "*.h")))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16], len(files)


def mutate(rng, seq, rate, alphabet):
    out = []
    for x in seq:
        u = rng.random()
        if u < rate / 3:
            continue                                     # deleted
        if u < 2 * rate / 3:
            out.append(int(rng.integers(0, alphabet)))   # substituted
            continue
        out.append(int(x))
        if u > 1 - rate / 3:
            out.append(int(rng.integers(0, alphabet)))   # inserted behind it
    return np.asarray(out, np.int32)


def wer_case(rng):
    lens = np.clip(np.round(rng.gamma(2.2, 9.0, 2939)), 3, 80).astype(int)
    refs = [rng.integers(0, 8000, n).astype(np.int32) for n in lens]
    hyps = [mutate(rng, r, 0.08, 8000) for r in refs]
    pool = hyps + refs
    return pool, [(k, len(hyps) + k) for k in range(len(hyps))]


def mbr_case(rng):
    pool, pairs = [], []
    for _ in range(64):
        text = rng.integers(0, 28, int(rng.integers(240, 361)))
        base = len(pool)
        pool.extend(mutate(rng, text, 0.03, 28) for _ in range(64))
        pairs.extend((base + k, base + j) for k in range(64) for j in range(k + 1, 64))
    return pool, pairs


def numpy_antidiagonal(a, b):
    """(distance, substitutions, deletions, insertions): the DP over (errors, substitutions) as errors * K + substitutions,
    one anti-diagonal per numpy step"""
    m, n = len(a), len(b)
    K = np.int64(1 << 20)
    if m == 0 or n == 0:
        C, S = m + n, 0
    else:
        a, br = np.asarray(a, np.int64), np.asarray(b, np.int64)[::-1]
        BIG = np.int64(1) << 60
        p2 = np.full(m + 1, BIG)                         # diagonal d - 2, indexed by the row
        p1 = np.full(m + 1, BIG)
        p2[0] = 0
        p1[0] = K
        p1[1] = K
        for d in range(2, m + n + 1):
            lo, hi = max(0, d - n), min(m, d)            # rows of the diagonal; column d - row
            new = np.full(m + 1, BIG)
            i0, i1 = max(lo, 1), min(hi, d - 1)          # interior cells
            if i0 <= i1:
                # a[i - 1] against b[d - i - 1] = br[n - d + i]
                ne = a[i0 - 1:i1] != br[n - d + i0:n - d + i1 + 1]
                new[i0:i1 + 1] = np.minimum(p2[i0 - 1:i1] + ne * (K + 1), np.minimum(p1[i0 - 1:i1], p1[i0:i1 + 1]) + K)
            if lo == 0:
                new[0] = d * K
            if hi == d:
                new[d] = d * K
            p2, p1 = p1, new
        C, S = divmod(int(p1[m]), int(K))
    D = (C - S - (m - n)) // 2
    return C, S, D, D + m - n


def run_case(name, pool, pairs, args, torch, N, transcribe_ms, utterances):
    from wav2vec2.metrics import edit_distance_pairs
    lib = N.load()
    lens = np.asarray([s.size for s in pool], np.int64)
    start = np.concatenate(([0], np.cumsum(lens)[:-1]))
    flat = np.concatenate(pool + [np.zeros(1, np.int32)])
    pairs = np.asarray(pairs, np.int64)
    hi, ri = pairs[:, 0], pairs[:, 1]
    hyp0, ref0 = np.ascontiguousarray(start[hi], np.int64), np.ascontiguousarray(start[ri], np.int64)
    hyp_len, ref_len = np.ascontiguousarray(lens[hi], np.int32), np.ascontiguousarray(lens[ri], np.int32)
    tokens = torch.from_numpy(flat).cuda()
    out = torch.empty((len(pairs), 4), dtype=torch.int32, device="cuda")

    def kernel():
        N.check(lib.w2v2_edit_distance(N.ptr(tokens), int(flat.size - 1), len(pairs), N.ptr(hyp0), N.ptr(hyp_len), N.ptr(ref0),
                                       N.ptr(ref_len), N.ptr(out), N.current_stream()))

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
    got = out.cpu().numpy()
    ct = []
    for _ in range(3):
        t0 = time.perf_counter()
        counts = edit_distance_pairs(pool, pairs)
        ct.append(time.perf_counter() - t0)
    call_ms = float(np.median(ct)) * 1e3
    assert [c.distance for c in counts] == got[:, 0].tolist()
    cells = int((hyp_len.astype(np.int64) * ref_len).sum())
    res = {"case": name, "pairs": len(pairs), "pool": len(pool), "tokens": int(flat.size - 1), "mean_hyp_len": round(float(hyp_len.mean()), 1),
           "mean_ref_len": round(float(ref_len.mean()), 1), "cells": cells, "kernel_ms": round(kernel_ms, 3), "kernel_ms_min": round(kt[0], 3),
           "gcells_per_s": round(cells / kernel_ms / 1e6, 2), "call_ms": round(call_ms, 2), "errors": int(got[:, 0].sum())}
    nref = min(args.ref_pairs, len(pairs))
    if nref:
        t0 = time.perf_counter()
        ref = [numpy_antidiagonal(pool[h], pool[r]) for h, r in pairs[:nref].tolist()]
        ref_s = time.perf_counter() - t0
        rc = int((hyp_len[:nref].astype(np.int64) * ref_len[:nref]).sum())
        res.update(ref_pairs=nref, ref_ms=round(ref_s * 1e3, 1), ref_mcells_per_s=round(rc / ref_s / 1e6, 2),
                   ref_ms_whole_case_extrapolated=round(ref_s * 1e3 * cells / max(rc, 1), 0),
                   equal_reference=bool(np.array_equal(got[:nref], np.asarray(ref, np.int32).reshape(nref, 4))))
    if transcribe_ms is not None:
        scaled = transcribe_ms * utterances / 64.0
        res.update(transcribe_ms_64=round(transcribe_ms, 1), utterances=utterances,
                   kernel_share_of_transcribe=round(kernel_ms / scaled, 6), call_share_of_transcribe=round(call_ms / scaled, 6))
    return res


def transcribe_times(torch):
    import wav2vec2
    from wav2vec2 import variables as V
    from wav2vec2.processor import Wav2Vec2Processor
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(ROOT, "tests", "golden", "vocab.json"))
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    rng = np.random.default_rng(0)                       # the packed_bench set
    lens = rng.integers(int(1.5 * SR), int(35.0 * SR) + 1, size=64)
    waves = [torch.randn(int(n), device="cuda") for n in lens]
    out = {}
    for key, kw in (("wer", dict(beam_width=16, nbest=1)), ("mbr", dict(beam_width=64, nbest=64))):
        m.transcribe(waves, tok, **kw)
        torch.cuda.synchronize()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            m.transcribe(waves, tok, **kw)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        out[key] = float(np.median(t)) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-pairs", type=int, default=300, help="pairs per case the numpy reference runs on (0: skip)")
    ap.add_argument("--no-transcribe", action="store_true")
    ap.add_argument("--out", default=None, help="write the markdown report here (profiles/edit_distance.md)")
    args = ap.parse_args()

    import torch
    from wav2vec2 import _native as N
    torch.cuda.set_device(0)
    tt = {"wer": None, "mbr": None} if args.no_transcribe else transcribe_times(torch)
    rng = np.random.default_rng(args.seed)
    results = [run_case("wer", *wer_case(rng), args, torch, N, tt["wer"], 2939),
               run_case("mbr", *mbr_case(rng), args, torch, N, tt["mbr"], 64)]
    for r in results:
        print(json.dumps(r))
    if args.out:
        sha, nfiles = source_hash()
        lines = ["# Edit distance (`edit.hip`, `w2v2_edit_distance`): measured", "",
                 f"`python tools/edit_bench.py` (seed {args.seed}, {args.steps} timed calls after {args.warmup}), one MI355X; sha256 over "
                 f"csrc/*.hip + *.h ({nfiles} files) {sha}.  The cases and the columns are described in the tool's header.", ""]
        for r in results:
            lines += ["```json", json.dumps(r), "```", ""]
        lines += ["| case | pairs | cells (sum of m x n) | kernel ms (min) | 10^9 cells / s | Python call ms | numpy anti-diagonal, whole case (extrapolated) | "
                  "kernel share of transcribe | call share of transcribe |", "|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            share = (f"{100 * r['kernel_share_of_transcribe']:.4f} % | {100 * r['call_share_of_transcribe']:.4f} %"
                     if "kernel_share_of_transcribe" in r else "n/a | n/a")
            ref = f"{r['ref_ms_whole_case_extrapolated'] / 1e3:.1f} s, equal: {r['equal_reference']}" if "ref_ms" in r else "n/a"
            lines.append(f"| {r['case']} | {r['pairs']} | {r['cells']:.3e} | {r['kernel_ms']} ({r['kernel_ms_min']}) | {r['gcells_per_s']} | "
                         f"{r['call_ms']} | {ref} | {share} |")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
