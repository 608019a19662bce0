#!/usr/bin/env python
"""Time of the resampler on seeded noise.  Reports one JSON line.

Cases, all to 16 kHz at the default filter: one recording of --seconds (default 3600 s) at 48 kHz, the same at 44.1 kHz, and the
packed_bench.py set (64 utterances of 1.5-35 s) at 8 kHz.  Per case:
  kernel        one w2v2_resample call on buffers allocated before (HIP events; median, min and max of --steps)
  gbps          bytes of input read plus output written, once each, over the median; `of_copy` is its share of the 6.29 TB/s that
                a copy kernel writes on this GPU (tools/write_bw.hip)
  gfma_per_s    taps over the median
  call          wav2vec2.audio.resample() from Python, everything included (the concatenation, the output buffer, the views)
  cpu           the same job on the host, on the first --cpu-seconds of the case and scaled to its length: the same filter through
                scipy.signal.resample_poly (one thread), or, where scipy does not import, as torch.conv1d over the phases at 16
                threads; `max_diff` is the largest difference from the kernel's output on that stretch
With --model (default on) the base Wav2Vec2ForCTC with seeded weights, fp32, on the 48 kHz recording:
  predict_long / transcribe_long (greedy path) given the 48 kHz audio with sampling_rate=48000, against the same calls given the
  audio already at 16 kHz.

    python tools/resample_bench.py [--seconds 3600] [--steps 10] [--warmup 2] [--cpu-seconds 60] [--no-model]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))

COPY_GBPS = 6290.0      # tools/write_bw.hip on this GPU


def stats(t, digits=3):
    t = sorted(t)
    return {"ms": round(float(np.median(t)), digits), "min": round(t[0], digits), "max": round(t[-1], digits)}


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
    return stats(t, 2)


def cpu_form(x, r, threads=16):
    """(seconds, output) of the filter of Resampler `r` on the host array `x`."""
    L, M, K, lead = r.L, r.M, r.taps, r.lead
    try:
        from scipy import signal
    except ImportError:
        signal = None
    if signal is not None:
        c = max(lead * L + L - 1, (K - 1 - lead) * L)
        p = np.zeros(2 * c + 1, np.float64)
        t, ph = np.meshgrid(np.arange(K), np.arange(L))
        p[c + (t - lead) * L - ph] = r.table[ph, t]
        t0 = time.perf_counter()
        y = signal.resample_poly(x, L, M, window=p) / L
        return time.perf_counter() - t0, y, "scipy.signal.resample_poly, 1 thread"
    import torch
    torch.set_num_threads(threads)
    n_out = -(-len(x) * L // M)
    xt = torch.from_numpy(np.concatenate([np.zeros(lead, np.float32), x, np.zeros(K + M, np.float32)]))[None, None]
    w = torch.from_numpy(r.table)[:, None, :]
    t0 = time.perf_counter()
    y = np.zeros(n_out, np.float32)
    for ph in range(L):                      # outputs n with n M % L == ph: n = n_ph + j L, their windows M apart
        ns = [n for n in range(L) if n * M % L == ph]
        n_ph = ns[0]
        q0 = n_ph * M // L
        got = torch.nn.functional.conv1d(xt[:, :, q0:], w[ph:ph + 1], stride=M)[0, 0].numpy()
        cnt = len(range(n_ph, n_out, L))
        y[n_ph::L] = got[:cnt]
    return time.perf_counter() - t0, y, f"torch.conv1d, {threads} threads"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()

    import torch
    import wav2vec2
    from wav2vec2 import _native as N
    from wav2vec2.audio import Resampler, resample
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    lib = N.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    rng = np.random.default_rng(args.seed)
    utt_s = rng.integers(int(1.5 * 16000), int(35.0 * 16000) + 1, size=64) / 16000.0
    cases = [("hour_48k", 48000, [args.seconds]), ("hour_44k1", 44100, [args.seconds]), ("packed_set_8k", 8000, list(utt_s))]
    res = {"seconds": args.seconds, "steps": args.steps, "copy_gbps": COPY_GBPS}
    for name, rate, seconds in cases:
        r = Resampler(rate)
        lens = np.asarray([int(s * rate) for s in seconds], np.int64)
        out_len = np.asarray([-(-int(n) * r.L // r.M) for n in lens], np.int64)
        x = torch.randn(int(lens.sum()), device="cuda", generator=gen)
        y = torch.empty(int(out_len.sum()), device="cuda")
        in0 = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        out0 = np.concatenate(([0], np.cumsum(out_len)[:-1])).astype(np.int64)
        table = r._table(x.device)
        fs = (N.W2V2ResampleFilter * 1)()
        fs[0].table, fs[0].L, fs[0].M, fs[0].K, fs[0].lead = table.data_ptr(), r.L, r.M, r.taps, r.lead

        def kernel():
            N.check(lib.w2v2_resample(N.ptr(x), len(lens), N.ptr(in0), N.ptr(lens), None, fs, 1, N.ptr(y), N.ptr(out0),
                                      N.current_stream()), "w2v2_resample")

        for _ in range(args.warmup):
            kernel()
        sync()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            kernel()
            b.record()
        sync()
        k = stats([a.elapsed_time(b) for a, b in ev])
        nbytes = 4.0 * (float(lens.sum()) + float(out_len.sum()))
        one = {"rate": rate, "segments": len(lens), "audio_s": round(float(sum(seconds)), 1), "L": r.L, "M": r.M, "taps": r.taps,
               "in_MB": round(4e-6 * float(lens.sum()), 1), "out_MB": round(4e-6 * float(out_len.sum()), 1), "kernel": k,
               "gbps": round(nbytes / k["ms"] * 1e-6, 1), "gfma_per_s": round(float(out_len.sum()) * r.taps / k["ms"] * 1e-6, 1)}
        one["of_copy"] = round(one["gbps"] / COPY_GBPS, 4)
        waves = list(torch.split(x, lens.tolist()))
        one["call"] = wall(lambda: resample(waves if len(waves) > 1 else waves[0], rate), max(3, args.steps // 2), 1, sync)
        n_cpu = int(min(args.cpu_seconds, seconds[0]) * rate)
        host = x[:n_cpu].cpu().numpy()
        t_cpu, y_cpu, how = cpu_form(host, r)
        got = resample(host, rate).cpu().numpy()
        one["cpu"] = {"how": how, "audio_s": round(n_cpu / rate, 1), "s": round(t_cpu, 3),
                      "s_scaled_to_case": round(t_cpu * float(sum(seconds)) * rate / n_cpu, 2),
                      "max_diff": float(np.abs(got - y_cpu).max())}
        res[name] = one
        if name != "hour_48k" or args.no_model:
            del x, y, waves
            continue
        # ---- the model on the 48 kHz recording, and on the same audio already at 16 kHz ----
        from wav2vec2 import variables as V
        cfg = wav2vec2.Wav2Vec2Config()
        m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=(1, 2048))
        m.set_weights(V.seeded_weights(cfg, seed=1))
        tok = wav2vec2.Wav2Vec2Processor(is_tokenizer=True, vocab_path=os.path.join(ROOT, "tests", "golden", "vocab.json"))
        at16 = y.clone()
        steps = max(2, min(3, args.steps))
        res["model"] = {
            "predict_long_16k": wall(lambda: m.predict_long(at16), steps, 1, sync),
            "predict_long_48k": wall(lambda: m.predict_long(x, sampling_rate=48000), steps, 1, sync),
            "transcribe_long_16k": wall(lambda: m.transcribe_long(at16, tok, beam_width=None), steps, 1, sync),
            "transcribe_long_48k": wall(lambda: m.transcribe_long(x, tok, beam_width=None, sampling_rate=48000), steps, 1, sync),
        }
        del m, at16, x, y, waves
    print(json.dumps(res))


if __name__ == "__main__":
    main()
