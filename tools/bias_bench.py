#!/usr/bin/env python
"""Time of the CTC prefix beam search with a phrase bias (w2v2_ctc_beam_search_biased, wav2vec2.decoding.ContextBias) on
tools/beam_bench.py's utterance set: 64 seeded lengths of 1.5-35 s through the base Wav2Vec2ForCTC (seeded weights, fp32) as one
predict_packed call, decoded at width 16 without a language model and with the word model of tools/wordlm_bench.py (open and
constrained), each with 0 phrases (the existing entry: the unbiased kernel), 100 phrases and 10 000 phrases.  The phrases are one
or two pseudo-words of the word model's lexicon, whole words, boost 2.0.  One JSON line:

  packed_ms     the packed fp32 forward of the set (median of 5)
  biases[]      phrases, states, MiB of the three tables, seconds of the host compile
  configs[]     kind (none / word_open / word_constrained), phrases, kernel_ms (HIP events around the C call; median, min, max of
                --steps), us_per_step (kernel_ms over the frame count of the longest utterance), over_unbiased (against 0 phrases of
                the same kind), with_bonus (utterances whose best hypothesis holds a phrase), changed (utterances whose best
                hypothesis differs from the unbiased one)

    python tools/bias_bench.py [--n 64] [--steps 10] [--warmup 2] [--words 20000] [--sentences 40000] [--width 16]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.5)
    ap.add_argument("--max-s", type=float, default=35.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nbest", type=int, default=1)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--sentences", type=int, default=40000)
    ap.add_argument("--phrases", type=int, nargs="*", default=[100, 10000])
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2 import variables as V
    from wav2vec2.alignment import _logits_base
    from wav2vec2.decoding import ContextBias, WordNgramLM, beam_search
    from wav2vec2.processor import Wav2Vec2Processor
    from wordlm_bench import pseudo_text
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
    text = pseudo_text(np.random.default_rng(args.seed + 3), args.words, args.sentences)       # the wordlm_bench model
    word_open = WordNgramLM.from_text(text, tok, 3, alpha=0.5, beta=0.1, unk_penalty=-4.0)
    word_con = WordNgramLM(word_open.ngrams, word_open.backoffs, word_open.lexicon, vs, word_open.delimiter, alpha=0.5, beta=0.1,
                           unk_penalty=-float("inf"))
    words = sorted(word_open.lexicon)
    prng = np.random.default_rng(args.seed + 4)
    biases, info = {}, []
    for k in args.phrases:
        picks = set()
        while len(picks) < k:
            nw = int(prng.integers(1, 3))
            picks.add(" ".join(words[int(i)] for i in prng.integers(len(words), size=nw)))
        t0 = time.perf_counter()
        biases[k] = ContextBias.from_phrases(sorted(picks), tok, boost=2.0)
        b = biases[k]
        info.append({"phrases": k, "states": b.n_states, "tables_mib": round((b.next.nbytes + b.delta.nbytes + b.final.nbytes) / 2 ** 20, 2),
                     "host_compile_s": round(time.perf_counter() - t0, 2)})

    base, row0, fl = _logits_base(logits, None)
    n, max_len, tot = len(fl), max(fl), sum(fl)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(fl, np.int32)
    nbest, W = args.nbest, args.width
    labels = torch.empty((n, nbest, max_len), dtype=torch.int32, device="cuda")
    length = torch.empty((n, nbest), dtype=torch.int32, device="cuda")
    score = torch.empty((n, nbest), dtype=torch.float64, device="cuda")
    total = torch.empty((n, nbest), dtype=torch.float64, device="cuda")
    lib = N.load()
    res = {"n": n, "audio_s": round(float(lens.sum()) / SR, 2), "frames": tot, "max_frames": max_len, "vocab": vs, "nbest": nbest,
           "beam_width": W, "packed_ms": round(packed_ms, 2), "biases": info, "configs": []}

    for kind, lm in (("none", None), ("word_open", word_open), ("word_constrained", word_con)):
        st = lm.device_arrays(base.device)[0] if lm is not None else None
        wp = ctypes.byref(st) if lm is not None else None
        delim, alpha, beta = (lm.delimiter, lm.alpha, lm.beta) if lm is not None else (0, 0.0, 0.0)
        pen = lm.unk_penalty if lm is not None else 0.0
        plain, unbiased_ms = None, None
        for k in [0] + list(args.phrases):
            bias = biases.get(k)
            if bias is None and lm is None:
                def kernel():
                    N.check(lib.w2v2_ctc_beam_search(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, nbest, None, 1, 0.0, 0.0,
                                                     max_len, N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))
            elif bias is None:
                def kernel():
                    N.check(lib.w2v2_ctc_beam_search_words(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, nbest, wp, delim,
                                                           alpha, beta, pen, 1, max_len, N.ptr(labels), N.ptr(length), N.ptr(score),
                                                           N.ptr(total), N.current_stream()))
            else:
                bst = bias.device_arrays(base.device)[0]

                def kernel():
                    N.check(lib.w2v2_ctc_beam_search_biased(N.ptr(base), vs, n, N.ptr(row0_h), N.ptr(frames_h), blank, W, nbest, None, 1, wp,
                                                            delim, alpha, beta, pen, 1, ctypes.byref(bst), max_len, N.ptr(labels),
                                                            N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()))

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
            hyps = beam_search(logits, beam_width=W, nbest=nbest, blank=blank, lm=lm, bias=bias)
            best = [h[0].ids if h else None for h in hyps]
            c = {"kind": kind, "phrases": k, "kernel_ms": round(kernel_ms, 3), "kernel_ms_min": round(kt[0], 3),
                 "kernel_ms_max": round(kt[-1], 3), "us_per_step": round(kernel_ms * 1e3 / max_len, 3),
                 "no_hypothesis": sum(1 for h in hyps if not h)}
            if bias is None:
                plain, unbiased_ms = best, kernel_ms
            else:
                c["over_unbiased"] = round(kernel_ms / unbiased_ms, 4)
                c["with_bonus"] = sum(1 for ids in best if ids is not None and bias.score(ids)[1])
                c["changed"] = sum(1 for x, y in zip(best, plain) if x != y)
            res["configs"].append(c)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
