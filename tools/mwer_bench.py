#!/usr/bin/env python
"""Cost of MWER training (w2v2_ctc_score_grad, wav2vec2.losses.MWERLoss), all numbers from one run:

  (1) on the 1024 (utterance, hypothesis) pairs of tools/score_bench.py (the packed_bench set through the base model, width 16 /
      nbest 16): one w2v2_ctc_score_grad call next to one w2v2_ctc_score call (HIP events; median, min, max), the bytes of a
      one-pass workspace, and the call again with a cap that takes it in one pass where the default of 8 GiB splits it into groups;
  (2) on wav2vec2-base bf16, 32 x 246000 (bench.py's training leg): an MWER step (width 8, nbest 4, the reference added) next to
      the CTC step, split into forward, search, edit distance, score, score_grad and backward (wall clock around a device
      synchronisation per part; the whole steps are timed without the inner synchronisations).

Prints one JSON line; --write PATH also writes the markdown of profiles/mwer.md.

    python tools/mwer_bench.py [--steps 5] [--warmup 1] [--skip-step] [--write profiles/mwer.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SR = 16000


def wall(torch, fn, steps, warmup):
    """median wall-clock ms of fn() with the device drained before and after"""
    t = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), out


def pairs_part(args, torch):
    import wav2vec2
    from score_bench import timed
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import beam_search
    cfg = wav2vec2.Wav2Vec2Config()
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
    m.set_weights(V.seeded_weights(cfg, seed=1))
    rng = np.random.default_rng(0)                               # the packed_bench set
    lens = rng.integers(int(1.5 * SR), int(35.0 * SR) + 1, size=64)
    logits = m.predict_packed([torch.randn(int(n), device="cuda") for n in lens])
    vs, blank = cfg.vocab_size, cfg.pad_id
    base, row0, fl = _logits_base(logits, None)
    n = len(fl)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    hyps = beam_search(logits, beam_width=16, nbest=16, blank=blank)
    pairs = [(i, h) for i, hs in enumerate(hyps) for h in hs]
    utt = np.asarray([i for i, _ in pairs], np.int32)
    nlab = np.asarray([len(h.ids) for _, h in pairs], np.int32)
    label0 = np.concatenate(([0], np.cumsum(nlab[:-1], dtype=np.int64))).astype(np.int64)
    lab_dev = torch.from_numpy(np.concatenate([np.asarray(h.ids, np.int32) for _, h in pairs] + [np.zeros(1, np.int32)])).cuda()
    mp = len(pairs)
    logp = torch.empty(mp, dtype=torch.float64, device="cuda")
    logp_g = torch.empty(mp, dtype=torch.float64, device="cuda")
    coef = torch.from_numpy(np.random.default_rng(1).standard_normal(mp)).cuda()
    grad = torch.zeros_like(base)
    lib = N.load()

    def scorer():
        N.check(lib.w2v2_ctc_score(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), mp, N.ptr(utt), N.ptr(lab_dev), N.ptr(label0),
                                   N.ptr(nlab), blank, N.ptr(logp), N.current_stream()))

    def grader(cap):
        N.check(lib.w2v2_ctc_score_grad(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), mp, N.ptr(utt), N.ptr(lab_dev), N.ptr(label0),
                                        N.ptr(nlab), blank, N.ptr(coef), N.ptr(logp_g), N.ptr(grad), cap, N.current_stream()))

    need = int(lib.w2v2_ctc_score_grad_workspace(n, N.ptr(frames_h), mp, N.ptr(utt), N.ptr(nlab), vs))
    score_ms, score_min, score_max = timed(torch, scorer, args.steps, args.warmup)
    grad_ms, grad_min, grad_max = timed(torch, lambda: grader(0), args.steps, args.warmup)
    res = {"pairs": mp, "utterances": n, "frames": int(sum(fl)), "labels_mean": round(float(nlab.mean()), 1), "labels_max": int(nlab.max()),
           "score_ms": round(score_ms, 3), "score_ms_min": round(score_min, 3), "score_ms_max": round(score_max, 3),
           "score_grad_ms": round(grad_ms, 3), "score_grad_ms_min": round(grad_min, 3), "score_grad_ms_max": round(grad_max, 3),
           "ratio": round(grad_ms / score_ms, 3), "workspace_one_pass_bytes": need, "default_cap_bytes": 8 << 30,
           "same_logp_bits": bool(torch.equal(logp.view(torch.int64), logp_g.view(torch.int64)))}
    if need > (8 << 30) and need <= (96 << 30):
        one_ms, one_min, one_max = timed(torch, lambda: grader(need), args.steps, args.warmup)
        res.update(one_pass_ms=round(one_ms, 3), one_pass_ms_min=round(one_min, 3), one_pass_ms_max=round(one_max, 3),
                   one_pass_ratio=round(one_ms / score_ms, 3))
    # where the time goes: the launches' time by the library's own counters is per family only, so time the sweeps' share by
    # running the call on one utterance's longest pair alone next to the scorer on the same pair
    j = int(np.argmax(nlab.astype(np.int64) * frames_h[utt]))
    one = (utt[j:j + 1].copy(), label0[j:j + 1].copy(), nlab[j:j + 1].copy())
    lp1 = torch.empty(1, dtype=torch.float64, device="cuda")

    def scorer1():
        N.check(lib.w2v2_ctc_score(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), 1, N.ptr(one[0]), N.ptr(lab_dev), N.ptr(one[1]),
                                   N.ptr(one[2]), blank, N.ptr(lp1), N.current_stream()))

    def grader1():
        N.check(lib.w2v2_ctc_score_grad(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), 1, N.ptr(one[0]), N.ptr(lab_dev), N.ptr(one[1]),
                                        N.ptr(one[2]), blank, N.ptr(coef), N.ptr(lp1), N.ptr(grad), 0, N.current_stream()))

    s1, _, _ = timed(torch, scorer1, args.steps, args.warmup)
    g1, _, _ = timed(torch, grader1, args.steps, args.warmup)
    res["longest_pair"] = {"frames": int(frames_h[utt[j]]), "labels": int(nlab[j]), "score_ms": round(s1, 3), "score_grad_ms": round(g1, 3),
                           "ratio": round(g1 / s1, 3)}
    del m
    return res


def step_part(args, torch):
    import wav2vec2 as W
    from wav2vec2 import decoding as D
    from wav2vec2 import losses as LS
    from wav2vec2 import metrics as M
    B, L, delim = 32, 246000, 4
    cfg = W.Wav2Vec2Config()
    model = W.Wav2Vec2ForCTC(cfg, input_shape=(B, L))
    model.set_precision("bf16")
    model.freeze_feature_extractor()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    x = torch.randn((B, L), generator=gen, device="cuda", dtype=torch.float32)
    rs = np.random.RandomState(77)                              # bench.py's label shape: 24..200 labels in [1, 31] per row
    labels = np.zeros((B, 256), np.int32)
    for b in range(B):
        k = rs.randint(24, 201)
        labels[b, :k] = rs.randint(1, 32, size=k)
    ctc = W.CTCLoss(cfg, (B, L), division_factor=B)
    mwer = W.MWERLoss(cfg, (B, L), division_factor=B, beam_width=8, nbest=4, delimiter_id=delim)
    tr = W.Trainer(model, ctc, learning_rate=1e-4, seed=0)
    labels_dev = torch.from_numpy(labels).cuda()
    T = int(ctc._get_logit_length(L))
    refs = [tuple(int(v) for v in row if v != cfg.pad_id) for row in labels]
    st, wu = args.steps, args.warmup

    ctc_step_ms, _ = wall(torch, lambda: tr.step(x, labels_dev), st, wu)
    tr.loss = mwer
    mwer_step_ms, _ = wall(torch, lambda: tr.step(x, labels), st, wu)
    parts = {}
    parts["forward"], logits = wall(torch, lambda: tr.forward(x), st, wu)
    parts["ctc_loss"], (_, g_ctc) = wall(torch, lambda: ctc.per_sample(labels_dev, logits, with_grad=True), st, wu)
    parts["search"], hyps = wall(torch, lambda: D.beam_search(logits, beam_width=8, nbest=4, blank=cfg.pad_id, frame_lengths=[T] * B), st, wu)
    lists, priors = LS.build_lists(hyps, refs, True)

    def edit():
        pool, pairs = LS.token_pool(lists, refs, "word", delim)
        return M.edit_distance_pairs(pool, pairs)

    parts["edit_distance"], counts = wall(torch, edit, st, wu)
    flat = [list(h) for hs in lists for h in hs]
    utt = [i for i, hs in enumerate(lists) for _ in hs]
    parts["score"], logp = wall(torch, lambda: D.ctc_score(logits, flat, blank=cfg.pad_id, frame_lengths=[T] * B, utterance=utt), st, wu)
    coef = np.random.default_rng(2).standard_normal(len(flat) + B)
    parts["score_grad"], (_, g) = wall(torch, lambda: D.ctc_score_grad(logits, flat + [list(r) for r in refs], coef, blank=cfg.pad_id,
                                                                      frame_lengths=[T] * B, utterance=utt + list(range(B))), st, wu)
    parts["mwer_loss"], _ = wall(torch, lambda: mwer.per_sample(labels, logits, with_grad=True, with_total=True), st, wu)

    def backward():
        tr.backward(g_ctc)
        tr.apply_gradients()

    tr.forward(x)
    parts["backward_and_update"], _ = wall(torch, backward, 1, 0)           # (one backward per forward: a single measurement)
    nl = np.asarray([len(h) for h in flat])
    return {"batch": B, "samples": L, "frames": T, "precision": "bf16", "beam_width": 8, "nbest": 4, "pairs": len(flat) + B,
            "hyp_labels_mean": round(float(nl.mean()), 1), "hyp_labels_max": int(nl.max()), "ref_labels_mean": round(float(np.mean([len(r) for r in refs])), 1),
            "ctc_step_ms": round(ctc_step_ms, 2), "mwer_step_ms": round(mwer_step_ms, 2), "step_ratio": round(mwer_step_ms / ctc_step_ms, 3),
            "parts_ms": {k: round(v, 3) for k, v in parts.items()}}


def markdown(res):
    p = res["pairs_1024"]
    out = ["# MWER training: the cost of w2v2_ctc_score_grad and of an MWER step", "",
           "Written by `tools/mwer_bench.py`; every number from one run on one MI355X.", "",
           "## (1) The 1024 pairs of tools/score_bench.py", "",
           f"{p['pairs']} pairs over {p['utterances']} utterances, {p['frames']} frames, labels per pair {p['labels_mean']} on average and "
           f"{p['labels_max']} at most.", "",
           "| call | median ms | min | max |", "|---|---|---|---|",
           f"| `w2v2_ctc_score` | {p['score_ms']} | {p['score_ms_min']} | {p['score_ms_max']} |",
           f"| `w2v2_ctc_score_grad`, default cap of 8 GiB | {p['score_grad_ms']} | {p['score_grad_ms_min']} | {p['score_grad_ms_max']} |"]
    if "one_pass_ms" in p:
        out.append(f"| `w2v2_ctc_score_grad`, one pass | {p['one_pass_ms']} | {p['one_pass_ms_min']} | {p['one_pass_ms_max']} |")
    out += ["", f"Ratio gradient / scorer: {p['ratio']}" + (f" (one pass: {p['one_pass_ratio']})" if "one_pass_ratio" in p else "") + ".  "
            f"A one-pass workspace is {p['workspace_one_pass_bytes']} bytes ({p['workspace_one_pass_bytes'] / 2 ** 30:.2f} GiB).  "
            f"`logp` carries the scorer's bits: {p['same_logp_bits']}.", "",
            f"The longest pair alone ({p['longest_pair']['frames']} frames, {p['longest_pair']['labels']} labels): scorer "
            f"{p['longest_pair']['score_ms']} ms, gradient {p['longest_pair']['score_grad_ms']} ms, ratio {p['longest_pair']['ratio']}."]
    if "step" in res:
        s = res["step"]
        out += ["", "## (2) An MWER step next to the CTC step", "",
                f"wav2vec2-base, {s['precision']}, {s['batch']} x {s['samples']} ({s['frames']} frames per row), seeded weights, feature extractor "
                f"frozen; width {s['beam_width']}, nbest {s['nbest']}, the reference added: {s['pairs']} pairs, hypotheses of {s['hyp_labels_mean']} "
                f"labels on average ({s['hyp_labels_max']} at most), references of {s['ref_labels_mean']}.", "",
                f"CTC step {s['ctc_step_ms']} ms; MWER step {s['mwer_step_ms']} ms; ratio {s['step_ratio']}.", "",
                "| part | ms |", "|---|---|"]
        out += [f"| {k} | {v} |" for k, v in s["parts_ms"].items()]
        out += ["", "`mwer_loss` is one `MWERLoss.per_sample` call (search, lists, edit distance, score, score_grad, and the host work between "
                "them); `ctc_loss` one `CTCLoss.per_sample` call.  The parts are wall clock around a drained device, so they add up to more than "
                "the step."]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-step", action="store_true", help="part (1) only")
    ap.add_argument("--write", default=None, help="also write the markdown of profiles/mwer.md to this path")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {"pairs_1024": pairs_part(args, torch)}
    from wav2vec2 import _native as N
    N.load().w2v2_release_scratch()
    torch.cuda.empty_cache()
    if not args.skip_step:
        res["step"] = step_part(args, torch)
    if args.write:
        with open(args.write, "w") as f:
            f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
