#!/usr/bin/env python
"""Time of the CTC prefix beam search with a word n-gram language model and a lexicon (w2v2_ctc_beam_search_words) on
tools/packed_bench.py's utterance set: 64 seeded lengths of 1.5-35 s through the base Wav2Vec2ForCTC (seeded weights, fp32) as one
predict_packed call.  The model: a lexicon of about 20 000 pseudo-words (seeded letter strings) and a 3-gram counted by
WordNgramLM.from_text on seeded sentences over them (Zipf-distributed words).  Decoded at widths 16 and 64, open (unk_penalty -4)
and constrained, and IN THE SAME RUN without a language model and with the character 3-gram of tools/beam_bench.py, beside the
packed forward.  One JSON line:

  packed_ms     the packed fp32 forward of the set (median of 5)
  lm            words, n-grams, states, arcs, lexicon nodes, MiB of the dense child table and of everything on the device
  configs[]     kind (none / char3 / word_open / word_constrained), beam_width, kernel_ms (HIP events around the C call; median,
                min, max of --steps), us_per_step (kernel_ms over the frame count of the longest utterance), over_packed, and for
                the word model over_char3 (against the character 3-gram at the same width), mean_len (labels of the best
                hypothesis), no_hypothesis (utterances without one), ref_equal on the first --ref-n utterances at width 16
                (tests/wordlm_reference.py; fragile ones left out, as tools/beam_bench.py does)

    python tools/wordlm_bench.py [--n 64] [--steps 10] [--warmup 2] [--words 20000] [--sentences 40000] [--ref-n 1]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000


def pseudo_text(rng, n_words, n_sentences):
    """seeded pseudo-words (2-9 letters, distinct) and sentences of 4-14 words drawn with Zipf weights"""
    words = set()
    while len(words) < n_words:
        for k in rng.integers(2, 10, size=n_words):
            words.add("".join(chr(65 + int(c)) for c in rng.integers(0, 26, size=int(k))))
            if len(words) == n_words:
                break
    words = sorted(words)
    rng.shuffle(words)
    p = 1.0 / np.arange(1, n_words + 1)
    p /= p.sum()
    lens = rng.integers(4, 15, size=n_sentences)
    draw = rng.choice(n_words, size=int(lens.sum()), p=p)
    draw[:n_words] = np.arange(n_words)                          # every word occurs
    out, at = [], 0
    for k in lens:
        out.append(" ".join(words[int(i)] for i in draw[at:at + int(k)]))
        at += int(k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nbest", type=int, default=1)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--sentences", type=int, default=40000)
    ap.add_argument("--ref-n", type=int, default=1, help="utterances the host reference is run on at width 16 (0: skip)")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import CharNgramLM, WordNgramLM, beam_search
    from wav2vec2.processor import Wav2Vec2Processor
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
    tok = Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(ROOT, "tests", "golden", "vocab.json"))
    assert max(tok.get_vocab().values()) + 1 == vs
    lrng = np.random.default_rng(args.seed + 2)
    letters = [v for v in range(vs) if v != blank]
    lm3 = CharNgramLM.from_ids([lrng.choice(letters, size=200).tolist() for _ in range(50)], vs, blank, order=3, add_k=0.5,
                               alpha=0.5, beta=0.1)
    t0 = time.perf_counter()
    text = pseudo_text(np.random.default_rng(args.seed + 3), args.words, args.sentences)
    word_open = WordNgramLM.from_text(text, tok, 3, alpha=0.5, beta=0.1, unk_penalty=-4.0)
    word_con = WordNgramLM(word_open.ngrams, word_open.backoffs, word_open.lexicon, vs, word_open.delimiter, alpha=0.5, beta=0.1,
                           unk_penalty=-float("inf"))
    build_s = time.perf_counter() - t0
    w = word_open
    dev_bytes = sum(getattr(w, k).nbytes for k in ("child", "word_at", "arc0", "arc_word", "arc_logp", "arc_next", "bo", "bstate"))

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
           "packed_ms": round(packed_ms, 2), "packed_ms_spread": [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)],
           "lm": {"words": len(w.words), "lexicon": len(w.lexicon), "ngrams": len(w.ngrams), "order": w.order, "states": len(w.bo),
                  "arcs": len(w.arc_word), "nodes": len(w.word_at), "child_mib": round(w.child.nbytes / 2 ** 20, 2),
                  "device_mib": round(dev_bytes / 2 ** 20, 2), "host_build_s": round(build_s, 1)},
           "configs": []}

    char_ms = {}
    for W in (16, 64):
        for kind, lm in (("none", None), ("char3", lm3), ("word_open", word_open), ("word_constrained", word_con)):
            if nbest > W:
                continue
            if kind.startswith("word"):
                st, _keep = lm.device_arrays(base.device)

                def kernel():
                    N.check(lib.w2v2_ctc_beam_search_words(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, nbest,
                                                           ctypes.byref(st), lm.delimiter, lm.alpha, lm.beta, lm.unk_penalty, 1, max_len,
                                                           N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))
            else:
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
            hyps = beam_search(logits, beam_width=W, nbest=nbest, blank=blank, lm=lm)
            c = {"kind": kind, "beam_width": W, "kernel_ms": round(kernel_ms, 3), "kernel_ms_min": round(kt[0], 3),
                 "kernel_ms_max": round(kt[-1], 3), "us_per_step": round(kernel_ms * 1e3 / max_len, 3),
                 "over_packed": round(kernel_ms / packed_ms, 4),
                 "mean_len": round(float(np.mean([len(h[0].ids) for h in hyps if h] or [0])), 1),
                 "no_hypothesis": sum(1 for h in hyps if not h)}
            if kind == "char3":
                char_ms[W] = kernel_ms
            if kind.startswith("word"):
                c["over_char3"] = round(kernel_ms / char_ms[W], 4)
                c["mean_words"] = round(float(np.mean([len([x for x in h[0].text(tok).split(" ") if x]) for h in hyps if h] or [0])), 1)
                if args.ref_n and W == 16:
                    import beam_reference as BR
                    import wordlm_reference as WR
                    hosts = [l.cpu().numpy() for l in logits[:args.ref_n]]
                    sc = WR.Scorer(lm)
                    t0 = time.perf_counter()
                    refs = [WR.search(h, W, nbest, blank, lm, sc) for h in hosts]
                    c["ref_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    firm = [i for i, (r, h) in enumerate(zip(refs, hosts)) if r.margin >= BR.tau(h.shape[0], r.kmax)]
                    c["ref_n"], c["ref_fragile"] = len(hosts), len(hosts) - len(firm)
                    c["ref_equal"] = all([x.ids for x in hyps[i]] == [k for k, _, _ in refs[i].hyps] for i in firm)
            res["configs"].append(c)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
