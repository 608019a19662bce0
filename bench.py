#!/usr/bin/env python
"""Headline benchmark: audio-seconds/s of the Wav2Vec2ForCTC forward (BASELINE.json).

Workload (configs[1]): wav2vec2-base, fp32, forward only, batch 32 x 246000 samples of
synthetic 16 kHz audio per GPU, random-init (seeded) weights.  A "step" is one forward of
that batch with the input already resident in HBM.  Multi-GPU is pure data parallel: every
rank runs its own 32-row shard, no collective on the data path (forward needs none); timing
is bracketed by barrier + synchronize and the MAX over ranks is reported ("weak" scaling).

    python bench.py --gpus 1 --steps 10 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR     # + DIR/logits.npy of the last timed step
    python bench.py --gpus 1 --steps K --warmup W --full                 # + everything measured beside the headline

A plain run sets up, runs --warmup untimed and --steps timed steps, writes the --dump-outputs files and prints the line;
`ms_per_step` is one timed step.  Rank 0 prints ONE JSON line.  Its `roofline` object costs no run of its own:
  roofline     -- the dominant kernel family (fp32 MFMA GEMM / implicit-GEMM conv): algorithmic
                  FLOPs / HIP-event time of its launches inside the timed region, against the
                  157.3 TFLOP/s fp32 matrix peak of gfx950.
--full adds what takes runs of its own or checks the result (--steps timed steps after --warmup untimed ones per leg):
  families, clock -- per-family breakdown from two extra instrumented steps; the shader clock under load.
  bf16x3, f16x2 -- the same forward in the two fp32-grade split modes (N=1 only).
  configs2_train_bf16, configs3_large_fwd_f32, configs4_large_train_bf16 -- the other BASELINE configurations.
  cpu_baseline -- the CPU oracle (numpy restatement of the reference path; TensorFlow cannot be
                  run here) timed on this box's host cores per BASELINE.md section 3 (B=1 and B=8, best /
                  median of 5, plus an aggregate of concurrent workers), rank 0, N=1 only.
  max_abs_logit_err -- rows 0-1 of the timed batch are the committed HF fixture's waveforms (in every run: the
                  inputs do not depend on --full); the logits of the timed forward are compared with HF-PyTorch fp64 (bar 1e-3).
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "gsoc-wav2vec2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SAMPLE_RATE = 16000
EVENT_STRIDE = 5          # of the dominant family's launches, every 5th is bracketed by HIP events inside the timed region
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense (no sparsity)
PEAK_HBM_GBS = 8000.0


_CPU_WORKER = r"""
import os, sys, time
pin = {pin!r}
if pin:
    os.sched_setaffinity(0, pin)                   # one disjoint set of physical cores (one NUMA node) per worker -- BEFORE numpy is
for v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):      # imported: the BLAS creates its worker threads at load
    os.environ[v] = str({nt})                      # time, and only threads created after the call inherit the affinity
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "gsoc-wav2vec2_amd"))
import numpy as np
from threadpoolctl import threadpool_limits
from oracle import w2v2_oracle as O
from wav2vec2 import variables as V
from wav2vec2.config import Wav2Vec2Config
cfg = Wav2Vec2Config(); w = dict(np.load({weights!r}))
x = V.hash_normal("bench/cpu", {L}, {seed}).reshape(1, {L})
with threadpool_limits(limits={nt}):
    O.ctc_forward(cfg, w, x)                       # warm-up
    print("CPU_WORKER_READY", flush=True)
    sys.stdin.readline()                           # all workers start their timed forwards together
    t0 = time.time()
    for _ in range({reps}):
        O.ctc_forward(cfg, w, x)
    print("CPU_WORKER_SPAN", t0, time.time(), len(os.sched_getaffinity(0)), flush=True)
"""


def _core_sets(workers, width):
    """`workers` disjoint lists of logical CPUs covering `width` PHYSICAL cores each -- every allowed hardware thread of those
    cores, so a worker's BLAS threads and its element-wise pool threads (oracle: one pool thread per usable CPU) each find a
    hardware thread; pinned to one thread per core the two pools fought over 16 CPUs and the leg ran 4x slower than unpinned --
    each list inside one NUMA node (nodes filled round-robin so the workers spread over all memory channels), drawn from this
    process's allowed CPUs.  Returns fewer lists than asked when the host has fewer whole sets; [] when the topology cannot be read."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        return []

    def read(path):
        try:
            with open(path) as f:
                return f.read().strip()
        except OSError:
            return None

    by_node, threads = {}, {}
    for cpu in allowed:
        base = f"/sys/devices/system/cpu/cpu{cpu}"
        core, pkg = read(f"{base}/topology/core_id"), read(f"{base}/topology/physical_package_id")
        if core is None:
            return []
        if (pkg, core) in threads:                     # an SMT sibling of a core already listed: it travels with that core
            threads[(pkg, core)].append(cpu)
            continue
        threads[(pkg, core)] = [cpu]
        node = next((d[4:] for d in (os.listdir(base) if os.path.isdir(base) else []) if d.startswith("node") and d[4:].isdigit()), pkg)
        by_node.setdefault(node, []).append((pkg, core))
    pools = [by_node[k] for k in sorted(by_node, key=str)]
    sets, progressed = [], True
    while len(sets) < workers and progressed:
        progressed = False
        for pool in pools:
            if len(sets) < workers and len(pool) >= width:
                sets.append(sorted(c for _ in range(width) for c in threads[pool.pop(0)]))
                progressed = True
    return sets


def _ranges(cpus):
    """[0, 1, 2, 128, 129, 130] -> '0-2,128-130'"""
    out, cpus = [], sorted(cpus)
    i = 0
    while i < len(cpus):
        j = i
        while j + 1 < len(cpus) and cpus[j + 1] == cpus[j] + 1:
            j += 1
        out.append(str(cpus[i]) if i == j else f"{cpus[i]}-{cpus[j]}")
        i = j + 1
    return ",".join(out)


def _cpu_quota():
    """CPUs' worth of time this container may use (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited.  The MI355X boxes
    expose 256 logical CPUs but run the job under a 16-CPU quota: more runnable threads than that are throttled, which is why
    OpenBLAS "gets slower" past 16 threads there and why concurrent workers do not add throughput."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = float(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = float(f.read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def _cpu_model():
    model, phys = "unknown CPU", set()
    try:
        pid = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name") and model == "unknown CPU":
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    pid = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    phys.add((pid, line.split(":", 1)[1].strip()))
    except OSError:
        pass
    return model, len(phys)


def _timed_runs(fn, runs):
    import statistics
    fn()                                                   # 1 warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts), ts


def cpu_baseline(cfg, weights, L, wave_row0=None):
    """the CPU restatement of the reference path (oracle/: numpy + OpenBLAS + threaded ufuncs;
    TensorFlow cannot be run) on this box's host cores -- base, fp32, L = 246000, B = 1 and B = 8 (row 0 = sample.wav
    normalised then zero-padded, other rows seeded noise), 1 warm-up, best and median of 5, CPU model and core counts
    printed.  OpenBLAS gets SLOWER beyond 8-32 threads on these shapes, so the BLAS width is probed first, and a third
    leg fills the host with several such workers, one utterance each (utterances are independent), as fresh
    subprocesses started together -- never a fork of this GPU process.  `value` is the best figure of the three legs
    (the aggregate when it ran); a leg that fails says why in `legs`."""
    import subprocess
    import tempfile
    import numpy as np
    from threadpoolctl import threadpool_limits
    from oracle import w2v2_oracle as O
    from wav2vec2 import variables as V
    ncpu = os.cpu_count() or 1
    model, phys = _cpu_model()
    phys = phys or max(1, ncpu // 2)
    quota = _cpu_quota()
    usable = phys if quota is None else max(1, min(phys, int(quota)))      # cores' worth of CPU time this job can actually burn
    rows = [V.hash_normal("bench/cpu", L, i) for i in range(8)]
    if wave_row0 is not None:
        rows[0] = np.asarray(wave_row0, np.float32)
    x8 = np.stack(rows)
    x1 = x8[:1]
    # -- BLAS width probe (B = 1, one timed forward per width after a warm-up)
    probe = {}
    for nt in (8, 16, 32, 64):
        if nt > ncpu:
            continue
        with threadpool_limits(limits=nt):
            O.ctc_forward(cfg, weights, x1)
            t0 = time.perf_counter()
            O.ctc_forward(cfg, weights, x1)
            probe[nt] = time.perf_counter() - t0
    if not probe:
        probe[ncpu] = float("inf")
    best_nt = min(probe, key=probe.get)
    legs = {}
    # -- leg 1: B = 1, best / median of 5
    with threadpool_limits(limits=best_nt):
        b1, m1, _ = _timed_runs(lambda: O.ctc_forward(cfg, weights, x1), 5)
    legs["B=1"] = {"best_s": round(b1, 4), "median_s": round(m1, 4), "runs": 5, "threads": best_nt,
                   "audio_s_per_s_best": round(L / SAMPLE_RATE / b1, 2), "audio_s_per_s_median": round(L / SAMPLE_RATE / m1, 2)}
    # -- leg 2: B = 8 in one process (5 timed runs unless one forward takes > 6 s, then 3 -- the bench must stay bounded)
    nt8 = min(ncpu, max(best_nt, 32)) if probe.get(32, float("inf")) < 1.5 * probe[best_nt] else best_nt
    with threadpool_limits(limits=nt8):
        t0 = time.perf_counter()
        O.ctc_forward(cfg, weights, x8)
        first = time.perf_counter() - t0
        runs8 = 5 if first < 6.0 else 3
        b8, m8, _ = _timed_runs(lambda: O.ctc_forward(cfg, weights, x8), runs8)
    legs["B=8"] = {"best_s": round(b8, 4), "median_s": round(m8, 4), "runs": runs8, "threads": nt8,
                   "audio_s_per_s_best": round(8 * L / SAMPLE_RATE / b8, 2), "audio_s_per_s_median": round(8 * L / SAMPLE_RATE / m8, 2)}
    # -- leg 3: fill the host: W concurrent single-utterance workers of the probed width, timed forwards started together
    procs = int(os.environ.get("W2V2_CPU_WORKERS", 0)) or max(1, min(16, usable // best_nt))
    pins = _core_sets(procs, best_nt)                 # pinned: unpinned workers migrate and share memory channels
    if pins:
        procs = len(pins)
    reps = 3
    if procs > 1:
        children, tmp = [], None
        try:
            tmp = tempfile.NamedTemporaryFile(suffix=".npz", delete=False)
            tmp.close()
            np.savez(tmp.name, **weights)
            for i in range(procs):
                code = _CPU_WORKER.format(root=ROOT, L=L, seed=i, nt=best_nt, reps=reps, weights=tmp.name,
                                          pin=pins[i] if pins else None)
                children.append(subprocess.Popen([sys.executable, "-c", code], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                                 stderr=subprocess.PIPE, text=True))
            deadline = time.perf_counter() + 150.0
            for ch in children:                                        # wait until every worker is warmed up
                line = ""
                while "CPU_WORKER_READY" not in line:
                    if time.perf_counter() > deadline:
                        raise TimeoutError("workers not ready within 150 s")
                    line = ch.stdout.readline()
                    if line == "":
                        raise RuntimeError(f"worker exited early: {ch.stderr.read()[-400:]}")
            for ch in children:
                ch.stdin.write("go\n")
                ch.stdin.flush()
            spans = []
            for ch in children:
                out, err = ch.communicate(timeout=max(1.0, deadline - time.perf_counter()))
                hit = [ln for ln in out.splitlines() if ln.startswith("CPU_WORKER_SPAN")]
                if not hit:
                    raise RuntimeError(f"worker gave no timing: {err[-400:]}")
                spans.append(tuple(float(v) for v in hit[0].split()[1:4]))
            wall = max(s[1] for s in spans) - min(s[0] for s in spans)
            legs["aggregate"] = {"workers": procs, "threads_each": best_nt, "forwards_each": reps, "wall_s": round(wall, 3),
                                 "audio_s_per_s": round(procs * reps * L / SAMPLE_RATE / wall, 2),
                                 "pinned": bool(pins), "cpus_per_worker_seen": sorted({int(s[2]) for s in spans}),
                                 "pin_sets": [_ranges(p) for p in pins] if pins else None}
        except Exception as exc:                                       # noqa: BLE001 -- reported, not hidden
            legs["aggregate"] = {"workers": procs, "threads_each": best_nt, "error": repr(exc)[:300]}
        finally:
            for ch in children:
                if ch.poll() is None:
                    ch.kill()
            if tmp is not None:
                try:
                    os.unlink(tmp.name)
                except OSError:
                    pass
    else:
        legs["aggregate"] = {"workers": 1, "note": f"{usable} usable cores ({phys} physical, cgroup quota {quota}) / {best_nt} BLAS threads leaves room for one "
                                                   "worker only: concurrent workers would share the same quota (measured on this pool: 8 pinned workers x 16 "
                                                   "threads = 21.4 audio-s/s against 21.4 for one)"}
    cands = [(legs["B=1"]["audio_s_per_s_best"], best_nt, "B=1"), (legs["B=8"]["audio_s_per_s_best"], nt8, "B=8")]
    if "audio_s_per_s" in legs["aggregate"]:
        cands.append((legs["aggregate"]["audio_s_per_s"], procs * best_nt, "aggregate"))
    value, cores, which = max(cands)
    return {
        "value": round(value, 3),
        "unit": "audio-seconds/s",
        "cores": cores,
        "kind": "port",
        "sample": f"CPU restatement of the reference path (numpy oracle; TensorFlow not run), wav2vec2-base fp32, L = {L}: "
                  f"value = best leg ({which}); legs: B=1 and B=8 best / median of 5 after 1 warm-up, plus an aggregate of "
                  f"concurrent single-utterance workers; BLAS width probed {sorted(probe)} -> {best_nt}",
        "cpu_model": model, "host_cpus": ncpu, "physical_cores": phys, "cgroup_cpu_quota": quota,
        "blas_probe_s": {str(k): round(v, 4) for k, v in probe.items()},
        "legs": legs,
        "reference_published": "1.10 (TF jit) / 2.58 (TF eager) / 3.71 (ONNX) audio-s/s at L = 50000, B = 1, Colab CPU (BASELINE.md section 1)",
    }


def golden_rows(L):
    """The two committed waveforms of tests/golden/base_sample_padded.npz (row 0 = data/sample.wav normalised then
    right-padded with zeros to 246000, row 1 = seeded noise) and their HF-PyTorch fp64 logits."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "base_sample_padded.npz")
    with np.load(path) as z:
        wave, logits = z["wave"], z["logits_f64"]
    if wave.shape[1] != L:
        return None, None
    return wave, logits


def _sha16(path):
    import hashlib
    try:
        with open(path, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return None


KERNEL_SOURCES = {"fp32": ("gemm_f32.hip", "gemm_epilogue.h"), "bf16": ("gemm_bf16.hip", "gemm_bf16_sw.hip", "gemm_sw_common.h", "gemm_epilogue.h"),
                  "bf16x3": ("gemm_split_sw.hip", "gemm_sw_common.h", "gemm_epilogue.h"), "f16x2": ("gemm_split_sw.hip", "gemm_sw_common.h", "gemm_epilogue.h")}
FAMILY_KERNEL_TAG = {"fp32": "gemm_f32", "bf16": "gemm_bf16", "bf16x3": "gemm_split", "f16x2": "gemm_split"}     # substring of the family's kernel names


def kernel_source_hash(precision):
    """sha256 (first 16 hex digits) over the kernel sources of the dominant GEMM family: the key a committed PMC figure is valid for."""
    import hashlib
    h = hashlib.sha256()
    for fn in KERNEL_SOURCES.get(precision, ()):
        try:
            with open(os.path.join(ROOT, "gsoc-wav2vec2_amd", "csrc", fn), "rb") as f:
                h.update(f.read())
        except OSError:
            return None
    return h.hexdigest()[:16]


def traffic_key(model, precision, mode, L):
    return f"{model}/{precision}/{mode}/{L}"


def measured_traffic(model, precision, mode, L):
    """HBM bytes PER STEP of the dominant GEMM family from the committed rocprofv3 --pmc summaries of this same command (separate
    FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 fetch correction; tools/pmc_traffic.sh writes profiles/hbm_traffic_configs.json with,
    per configuration, the family's kernel launches per step, bytes per launch and the hash of the kernel sources they were measured
    on).  PMC counters cannot be collected from inside the run, so this is a STORED figure: returned with its provenance, and refused
    (None, with the reason) when the kernel sources have changed since it was measured -- a stale number is never printed as current."""
    out = {"bytes_per_step": None, "bytes_per_launch": None, "kernel_launches_per_step": None, "source": None}
    fn = "hbm_traffic_configs.json"
    try:
        with open(os.path.join(ROOT, "profiles", fn)) as f:
            js = json.load(f)
        e = js[traffic_key(model, precision, mode, L)]
        want = kernel_source_hash(precision)
        if e.get("kernel_source_sha16") != want:
            out["source"] = (f"profiles/{fn} [{traffic_key(model, precision, mode, L)}] was measured on kernel sources {e.get('kernel_source_sha16')} "
                             f"(round {e.get('round')}); the sources are now {want}: stale, not printed -- rerun tools/pmc_traffic.sh")
            return out
        n = e["kernel_launches_per_step"]
        if not n:
            raise ValueError("no launches of the family in the profile")
        out["bytes_per_launch"] = round(e["fetch_corrected_bytes_per_launch"] + e["write_bytes_per_launch"])
        out["kernel_launches_per_step"] = n
        out["bytes_per_step"] = round(n * (e["fetch_corrected_bytes_per_launch"] + e["write_bytes_per_launch"]))
        out["source"] = f"committed PMC profile profiles/{fn} (round {e.get('round')}, kernel sources {want}); not measured in this run"
    except (OSError, ValueError, KeyError, ZeroDivisionError, TypeError) as exc:
        out["source"] = f"no usable PMC profile: {exc!r}"
    return out


def add_traffic(roof, model, precision, mode, L):
    """roofline.traffic* on ONE denominator: HBM bytes per step of the family (PMC, stored) beside the compulsory bytes per step (A + B + C
    of every op-level call once), and their ratio."""
    if roof is None:
        return
    tr = measured_traffic(model, precision, mode, L)
    alg = roof.get("traffic_algorithmic_per_step")
    roof["traffic"] = tr["bytes_per_launch"]
    roof["traffic_unit"] = "HBM bytes per kernel launch of the family (rocprofv3 PMC FETCH_SIZE x 2 + WRITE_SIZE, separate passes)"
    roof["traffic_per_step"] = tr["bytes_per_step"]
    roof["traffic_over_algorithmic"] = round(tr["bytes_per_step"] / alg, 3) if tr["bytes_per_step"] and alg else None
    roof["traffic_source"] = tr["source"]


def self_launch(n):
    """Re-run this command line under `python -m torch.distributed.run --nnodes=1 --nproc-per-node n` (the form the
    driver itself uses for N > 1); returns the launcher's exit code.  Ranks inherit stdout, so rank 0's JSON line is this
    process's output."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


PEAK_CLOCK_MHZ = 2400.0           # MI355X_MICROARCH.md: the clock the peak figures are quoted at


def clock_under_load(ctx, run_step, window_us):
    """Shader clock while a workload runs, measured live: a one-wave probe kernel (w2v2_clock_probe, csrc/clock_probe.hip) on a side
    stream samples the shader-cycle counter (s_memtime: one tick per shader cycle) and the constant-rate wall clock over a window
    inside one untimed step of the workload on the main stream.  MI355X clocks to its power budget, so the 2.4 GHz behind the nominal
    peak need not be what a kernel mix runs at; `frac_clock_adjusted` = achieved / (peak x measured clock / 2400).  The idle figure
    (probe alone) is printed beside it."""
    import ctypes as C
    torch = ctx["torch"]
    from wav2vec2 import _native as N
    lib = N.load()
    side = torch.cuda.Stream()
    buf = torch.zeros(8, dtype=torch.int64, device=ctx["dev"])
    khz = C.c_int32()

    def mhz(t):
        v = t.cpu().tolist()
        dc, dw = v[2] - v[0], v[3] - v[1]
        return (dc / dw * khz.value / 1000.0, dw * 1e3 / khz.value) if dw > 0 else (None, 0.0)

    try:
        torch.cuda.synchronize()
        time.sleep(0.05)
        N.check(lib.w2v2_clock_probe(C.c_void_p(side.cuda_stream), 5000, C.c_void_p(buf[:4].data_ptr()), C.byref(khz)), "w2v2_clock_probe")
        torch.cuda.synchronize()
        idle, _ = mhz(buf[:4])
        run_step()                                              # re-warm, then the probed step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_step()                                              # enqueue only (asynchronous)
        t_enq = time.perf_counter() - t0
        N.check(lib.w2v2_clock_probe(C.c_void_p(side.cuda_stream), int(window_us), C.c_void_p(buf[4:].data_ptr()), C.byref(khz)), "w2v2_clock_probe")
        torch.cuda.synchronize()
        busy, got_us = mhz(buf[4:])
        return {"clock_mhz_under_load": round(busy, 1) if busy else None, "clock_mhz_idle": round(idle, 1) if idle else None,
                "clock_method": f"live: one-wave probe kernel on a side stream, d(s_memtime) / d(s_memrealtime) over a {got_us / 1e3:.1f} ms window "
                                f"inside one untimed step of this workload (its enqueue took {1e3 * t_enq:.1f} ms); cross-check by PMC "
                                "(GRBM_GUI_ACTIVE / 8 XCDs / kernel duration) in profiles/"}
    except Exception as exc:                                    # noqa: BLE001 -- a side measurement never costs the line
        return {"clock_mhz_under_load": None, "clock_error": repr(exc)[:200]}


def add_clock(roof, clk):
    if roof is None or not clk:
        return
    roof.update(clk)
    if clk.get("clock_mhz_under_load"):
        adj = roof["peak"] * clk["clock_mhz_under_load"] / PEAK_CLOCK_MHZ
        roof["peak_at_measured_clock"] = round(adj, 1)
        roof["frac_clock_adjusted"] = round(roof["achieved"] / adj, 4)


DEFAULT_BATCH = {"base": 32, "large-robust": 16}      # per-GPU batch of the BASELINE configurations (the PMC profiles are kept for these)
FAMILY_OF = {"fp32": "gemm_f32", "bf16": "gemm_bf16", "bf16x3": "gemm_split", "f16x2": "gemm_split"}
PEAK_OF = {"fp32": PEAK_F32_MFMA_TFLOPS, "bf16": PEAK_BF16_MFMA_TFLOPS, "bf16x3": round(PEAK_BF16_MFMA_TFLOPS / 6, 1),
           "f16x2": round(PEAK_BF16_MFMA_TFLOPS / 3, 1)}
KERNEL_OF = {
    "fp32": "gemm_f32_dma_kernel (fp32 MFMA 32x32x2, LDS-DMA staged, 256x128x16 tiles for the well-filled shapes, 128x128x32 for the rest, 64x64 "
            "for underfilled last rounds: conv1-6 implicit GEMM + all Dense layers)",
    "bf16": "gemm_bf16 family (bf16 MFMA 32x32x16, operands from bf16 shadows by LDS-DMA: gemm_bf16_sw_kernel 128x256 software-pipelined "
            "for the large shapes, gemm_bf16_kernel 128x128 for the rest, gemm_bf16_tr_kernel for weight gradients: conv1-6 + all Dense)",
    "bf16x3": "gemm_split_sw_kernel<.., bf16x3> (fp32 GEMM as 6 bf16 MFMA 32x32x16 products of exact 3-term operand splits, both operands streamed as "
              "planes written by their producers; peak = bf16 dense peak / 6)",
    "f16x2": "gemm_split_sw_kernel<.., f16x2> (fp32-grade GEMM as 3 fp16 MFMA 32x32x16 products of 2-term operand splits; peak = fp16 dense peak / 3)",
}
DTYPE_OF = {"fp32": "f32", "bf16": "bf16 operands, f32 accumulate (Dense / Conv1D); f32 elsewhere",
            "bf16x3": "f32 operands as exact 3 x bf16 sums, 6 bf16 MFMA products per f32 product, f32 accumulate (Dense / Conv1D); f32 elsewhere",
            "f16x2": "f32 operands as 2 x fp16 sums (22 bits), 3 fp16 MFMA products per f32 product, f32 accumulate (Dense / Conv1D); f32 elsewhere"}
ALT_NOTE = {"bf16x3": "bf16x3 (fp32 operands as exact 3 x bf16 sums, 6 bf16 MFMA products per fp32 product, fp32 accumulate)",
            "f16x2": "f16x2 (fp32 operands as 2 x fp16 sums of x 2^e, 3 fp16 MFMA products per fp32 product, fp32 accumulate; |activation| < 4094)"}
MATRIX_FAMILIES = ("gemm_f32", "gemm_bf16", "gemm_split", "pos_conv", "attention", "conv0_apply")


def make_labels(B, rank):
    """labels (B, 256) int32, first 24..200 entries uniform in [1, 31], rest 0."""
    import numpy as np
    rs = np.random.RandomState(7 + rank)
    labels = np.zeros((B, 256), np.int32)
    for b in range(B):
        n = rs.randint(24, 201)
        labels[b, :n] = rs.randint(1, 32, size=n)
    return labels


def run_leg(ctx, spec, model=None):
    """Time one workload: `warmup` untimed steps, then exactly `steps` steps between barrier + synchronize on both sides, MAX over
    ranks.  spec: model ("base" | "large-robust"), precision, mode ("forward" | "train"), B (rows per GPU), L, steps, warmup, profile,
    extras.  Returns (numbers, model, last output).  A training leg on more than one rank runs the bucketed RCCL gradient all-reduce
    inside every timed step (Trainer.step).  With extras (the default; a plain run's headline leg has it off) the leg also measures
    what takes steps of its own after the timed ones -- a training leg on more than one rank is timed again WITHOUT the collective to
    report the exposed communication time; the per-family breakdown; the clock -- and checks the golden rows against HF fp64."""
    torch, D, W, dev, world, rank = ctx["torch"], ctx["D"], ctx["W"], ctx["dev"], ctx["world"], ctx["rank"]
    cfg = W.Wav2Vec2Config() if spec["model"] == "base" else W.RobustWav2Vec2Config()
    B, L, mode, precision = spec["B"], spec["L"], spec["mode"], spec["precision"]
    steps, warmup, do_prof = spec["steps"], spec["warmup"], spec.get("profile", True)
    extras = spec.get("extras", True)
    T = cfg.num_frames(L)
    if model is None:
        model = W.Wav2Vec2ForCTC(cfg, input_shape=(B, L))       # random-init weights from the seeded generator (seed 0)
    model.set_precision(precision)
    family = FAMILY_OF[precision]

    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    x = torch.randn((B, L), generator=gen, device=dev, dtype=torch.float32)   # resident in HBM
    # Parity inside the timed workload: rows 0-1 of every rank's batch are the two waveforms of the committed
    # HF fixture, so the logits the timed forward produces for them are checked against HF-PyTorch fp64.
    gold_wave, gold_logits = (None, None)
    if spec["model"] == "base" and mode == "forward" and B >= 2:
        gold_wave, gold_logits = golden_rows(L)
        if gold_wave is not None:
            x[:2] = torch.from_numpy(gold_wave).to(dev)
    amask = torch.ones((B, L), device=dev, dtype=torch.int32) if cfg.is_robust else None   # robust models take a mask

    def barrier():
        D.barrier(sync_device=torch.cuda.synchronize)

    trainer = None
    if mode == "train":
        labels_dev = torch.from_numpy(make_labels(B, rank)).to(dev)
        model.freeze_feature_extractor()                      # stage 2 of the reference (main.py:234-237)
        trainer = W.Trainer(model, W.CTCLoss(cfg, (B, L), division_factor=world * B), learning_rate=1e-4, seed=rank,
                            collective=ctx.get("collective", "torch"))

        def step(all_reduce=True):
            return trainer.step(x, labels_dev, attention_mask=amask, all_reduce=all_reduce)
    else:
        def step(all_reduce=True):
            return model(x, attention_mask=amask)

    out = None
    for _ in range(warmup):
        out = step()
    barrier()
    # Timed region: HIP events bracket ONLY the dominant kernel family (the roofline object), and of that family every
    # EVENT_STRIDE-th launch: an event pair costs ~7 us of stream time (all ~150 GEMM launches of a bf16 fine-tune step:
    # +0.9 ms = 2.3 % on `value`, measured).  The stride is coprime to the launches per step of every configuration, so over the
    # timed steps the samples rotate through all shapes equally and the flop-weighted average is the family's.
    if do_prof:
        model.profile(True, families=[family], stride=EVENT_STRIDE)
    model.profile_reset()                                      # (also clears the kernel-launch counters)
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    prof = model.profile_read()
    model.profile(False)
    elapsed = D.max_over_ranks(elapsed, device=dev)            # the slowest rank defines the step
    timed_out = out                                            # (a training leg's loss is reported from the last TIMED step: the steps further
                                                               #  down that skip the collective let the replicas' weights diverge)
    res = {"elapsed": elapsed, "ms_per_step": 1e3 * elapsed / steps, "B": B, "L": L, "T": T, "cfg": cfg, "x": x, "amask": amask,
           "timed_out": timed_out, "family": family, "prof": prof if do_prof else {}, "gold_wave": gold_wave, "gold_logits": gold_logits,
           "kernel_launches_per_step": {k: v["kernels"] // steps for k, v in prof.items() if v["kernels"]},
           "op_calls_per_step": {k: v["issued"] // steps for k, v in prof.items() if v["issued"]}}

    # -- the gradient collective, measured (N > 1 training legs): the same steps without it, and the collective alone
    if trainer is not None:
        payload, buckets, colls = trainer.all_reduce_payload()
        ar = {"payload_bytes": payload, "buckets": buckets, "collectives_per_step": colls, "payload_dtype": trainer.allreduce_dtype,
              "op": "SUM all-reduce of the trainable slots of the flat gradient buffer, one per bucket (lm_head, encoder layers N-1 .. 0, front) "
                    "on a communication stream behind that bucket's completion event, under the rest of the backward (Trainer.all_reduce_gradients)",
              "backend": ctx["comm"]["backend"], "world_size": world,
              "engine": {"torch": "torch.distributed all_reduce per run (RCCL)", "native": "library: ncclAllReduce per bucket on its own stream (csrc/comm.hip)",
                         "native-rs": "library: ncclReduceScatter + ncclAllGather per bucket on its own stream (csrc/comm.hip)"}[trainer.collective]}
        if world > 1 and extras:
            for _ in range(1):
                step(all_reduce=False)
            barrier()
            t1 = time.perf_counter()
            for _ in range(steps):
                step(all_reduce=False)
            barrier()
            e_no = D.max_over_ranks(time.perf_counter() - t1, device=dev)
            overlap_was = trainer.overlap_all_reduce
            trainer.overlap_all_reduce = False                 # the collective alone: all buckets back to back on the calling stream
            trainer.all_reduce_gradients()
            barrier()
            reps = 3
            t2 = time.perf_counter()
            for _ in range(reps):
                trainer.all_reduce_gradients()
            barrier()
            e_ar = D.max_over_ranks(time.perf_counter() - t2, device=dev) / reps
            trainer.overlap_all_reduce = overlap_was
            ar.update({"ms_per_step_without_collective": round(1e3 * e_no / steps, 3),
                       "exposed_ms": round(1e3 * (elapsed - e_no) / steps, 3),
                       "standalone_ms": round(1e3 * e_ar, 3),
                       "busbw_GBps": round(payload * 2 * (world - 1) / world / e_ar / 1e9, 3),
                       "algbw_GBps": round(payload / e_ar / 1e9, 3),
                       "busbw_note": "payload x 2 (N - 1) / N / standalone time (ring all-reduce convention); xGMI: 7 links x ~153 GB/s per GPU"})
        elif world == 1:
            ar["note"] = "one rank: no collective is issued (SUM over one replica is the identity); the N > 1 lines carry exposed_ms / busbw"
        res["allreduce"] = ar

    # -- per-family breakdown: two extra, untimed steps with every family instrumented
    if do_prof and extras:
        model.profile(True)
        model.profile_reset()
        for _ in range(2):
            out = step()
        barrier()
        res["prof_all"] = model.profile_read()
        model.profile(False)
    if do_prof and extras and rank == 0:
        # the probed window: 40 % of a step, started right after the step's enqueue (long enough to average over many kernels)
        res["clock"] = clock_under_load(ctx, lambda: step(all_reduce=False), max(2000, min(60000, int(400 * res["ms_per_step"]))))
    if mode == "train":
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(timed_out).all()), "training loss is not finite"
        res["final_loss"] = round(float(timed_out), 4)
    else:
        assert tuple(out.shape) == (B, T, cfg.vocab_size) and bool(torch.isfinite(out).all())
    if gold_logits is not None and extras:
        # `out` is the output of the last TIMED-configuration forward (per-family instrumentation does not change results)
        err = float((out[:2].double().cpu() - torch.from_numpy(gold_logits).double()).abs().max())
        bar = 1e-3 if precision in ("fp32", "bf16x3", "f16x2") else 0.15
        assert err < bar, f"rank {rank}: max |logits - HF fp64| = {err:.3e} exceeds {bar}"
        res["logit_err"] = D.max_over_ranks(err, device=dev)
    return res, model, out


def roofline_of(res, spec, steps):
    """The `roofline` object of a leg: algorithmic FLOPs of the event-bracketed launches of the dominant GEMM family / their HIP-event time."""
    gm = res["prof"].get(res["family"])
    if not gm or gm["ms"] <= 0:
        return None
    precision = spec["precision"]
    ach, peak = gm["flops"] / (gm["ms"] * 1e-3) / 1e12, PEAK_OF[precision]
    return {"kernel": KERNEL_OF[precision], "bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "launches_per_step": gm["issued"] // max(1, steps),
            "kernel_launches_per_step": gm["kernels"] // max(1, steps),
            "launches_note": "launches_per_step = op-level GEMM calls; kernel_launches_per_step = kernels enqueued for them (a call whose last "
                             "round of tiles is underfilled runs a main + a tail-tile kernel): the count a rocprofv3 kernel trace shows",
            "avg_launch_ms": round(gm["ms"] / max(1, gm["launches"]), 4),
            "traffic_algorithmic_per_step": round(gm["bytes"] / max(1, gm["launches"]) * (gm["issued"] // max(1, steps))),
            "traffic_algorithmic_note": "compulsory HBM bytes per step of the family (A + B + C of every op-level call once; mean over the bracketed "
                                        "launches x calls per step) -- the same denominator as traffic_per_step",
            "event_sampling": f"every {EVENT_STRIDE}th launch of the family bracketed ({gm['launches']} of {gm['issued']})"}


def families_of(res, world, steps):
    """Per-family ms / step from the two instrumented steps, with `share` of the TIMED step (so the shares plus `unattributed`
    add to 1: launch gaps, host time and anything un-instrumented show up instead of being normalised away)."""
    pa = res.get("prof_all") or {}
    step_ms = res["ms_per_step"]
    fam = {k: {"ms_per_step": round(v["ms"] / 2, 3), "share": round(v["ms"] / 2 / step_ms, 4),
               "kernel_launches_per_step": v["kernels"] // 2,
               "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 else 0.0,
               "gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["ms"] > 0 else 0.0}
           for k, v in pa.items() if v["launches"] > 0}
    attributed = sum(v["ms"] for v in pa.values()) / 2
    flops_step = sum(v["flops"] for k, v in pa.items() if k in MATRIX_FAMILIES) / 2
    return fam, round(step_ms - attributed, 3), sum(v["kernels"] for v in pa.values()) // 2, flops_step


def side_object(ctx, spec, res, label):
    """One BASELINE configuration measured beside the headline, as a self-contained object of the JSON line."""
    world = ctx["world"]
    B, L, steps = res["B"], res["L"], spec["steps"]
    fam, unattr, kernels, flops_step = families_of(res, world, steps)
    obj = {"workload": label, "n_gpus": world, "global_batch": world * B, "samples": L, "frames": res["T"], "steps": steps, "warmup": spec["warmup"],
           "ms_per_step": round(res["ms_per_step"], 3), "value": round(world * B * L / SAMPLE_RATE * steps / res["elapsed"], 2),
           "unit": "audio-seconds/s", "dtype": DTYPE_OF[spec["precision"]], "roofline": roofline_of(res, spec, steps),
           "families": fam, "unattributed_ms": unattr, "kernel_launches_per_step": kernels,
           "matrix_tflops": round(flops_step * world / (res["ms_per_step"] * 1e-3) / 1e12, 2)}
    if B == DEFAULT_BATCH.get(spec["model"]):
        add_traffic(obj["roofline"], spec["model"], spec["precision"], spec["mode"], L)
    add_clock(obj["roofline"], res.get("clock"))
    if "final_loss" in res:
        obj["final_loss"] = res["final_loss"]
    if "allreduce" in res:
        obj["allreduce"] = res["allreduce"]
    return obj


def measure_alt(ctx, model, x, amask, model_name, B, L, steps, warmup, prec, ref_logits, gold_logits, profile):
    """Beside a fp32 forward leg (never as it): the same workload on the same model in an fp32-grade split mode -- "bf16x3" (six bf16 MFMA
    products of exact three-term operand splits) or "f16x2" (three fp16 products of two-term splits), DESIGN.md section 5 (history: profiles/history.md 7.2, 7.3).  Single-process,
    timed after the leg; its own roofline (GEMM family, events on every launch of two extra untimed steps), families, clock, traffic."""
    torch = ctx["torch"]
    model.set_precision(prec)
    try:
        for _ in range(warmup):
            out3 = model(x, attention_mask=amask)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            out3 = model(x, attention_mask=amask)
        torch.cuda.synchronize()
        e3 = time.perf_counter() - t1
        ms_step = 1e3 * e3 / steps
        roof, fam, unattr = None, None, None
        if profile:
            model.profile(True)
            model.profile_reset()
            for _ in range(2):
                out3 = model(x, attention_mask=amask)
            torch.cuda.synchronize()
            pa = model.profile_read()
            model.profile(False)
            gs = pa.get("gemm_split")
            fam = {k: {"ms_per_step": round(v["ms"] / 2, 3), "share": round(v["ms"] / 2 / ms_step, 4), "kernel_launches_per_step": v["kernels"] // 2,
                       "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 else 0.0,
                       "gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["ms"] > 0 else 0.0} for k, v in pa.items() if v["launches"] > 0}
            unattr = round(ms_step - sum(v["ms"] for v in pa.values()) / 2, 3)
            if gs and gs["ms"] > 0:
                ach, pk = gs["flops"] / (gs["ms"] * 1e-3) / 1e12, PEAK_OF[prec]
                roof = {"kernel": KERNEL_OF[prec], "bound": "mfma", "achieved": round(ach, 2), "peak": pk, "unit": "TFLOP/s (fp32-equivalent)",
                        "frac": round(ach / pk, 4), "launches_per_step": gs["issued"] // 2, "kernel_launches_per_step": gs["kernels"] // 2,
                        "ms_per_step": round(gs["ms"] / 2, 3),
                        "traffic_algorithmic_per_step": round(gs["bytes"] / 2),
                        "peak_note": "peak = nominal dense bf16 / fp16 MFMA peak / products per fp32 product.  On real operands the matrix pipe itself "
                                     "sustains 0.68-0.76 of the nominal figure at 1.67-1.85 GHz (power-limited: a register-only MFMA loop, "
                                     "profiles/r05_mfma_power_probe.txt), which bounds frac for any kernel"}
                if B == DEFAULT_BATCH.get(model_name):
                    add_traffic(roof, model_name, prec, "forward", L)
                # the clock this mode runs at (the bf16 / fp16 matrix pipe draws more power than the fp32 one: the chip throttles)
                add_clock(roof, clock_under_load(ctx, lambda: model(x, attention_mask=amask), max(2000, int(400 * ms_step))))
    finally:
        model.set_precision("fp32")
    o = {"precision": ALT_NOTE[prec], "value": round(B * L / SAMPLE_RATE * steps / e3, 2), "unit": "audio-seconds/s", "steps": steps,
         "ms_per_step": round(ms_step, 3), "roofline": roof, "families": fam, "unattributed_ms": unattr,
         "max_abs_logit_diff_vs_fp32_path": float((out3 - ref_logits).abs().max()),
         "note": "opt-in mode, not the headline; logit error vs the fp64 reference at the fp32 path's level (tests/test_model_gpu.py)"}
    if gold_logits is not None:
        o["max_abs_logit_err"] = float((out3[:2].double().cpu() - torch.from_numpy(gold_logits).double()).abs().max())
    if prec == "f16x2":
        o["range_overflow"] = bool(model.range_overflow())
    return o


DUMP_MAX_ELEMS = 8 << 20          # --dump-outputs: at most 32 MiB of float32 per array


def dump_outputs(out_dir, mode, timed_out):
    """--dump-outputs DIR: what a caller of the timed path received from its last timed step, as float32 .npy files in DIR -- the
    logits (B, T, vocab) of a forward leg, the loss of a training step.  The inputs are seeded, so two builds run with the same
    arguments can be compared file for file.  An array above DUMP_MAX_ELEMS is replaced by a fixed, seeded sample of its elements
    (flat; the same positions on every run with the same shape)."""
    import numpy as np
    name = "logits" if mode == "forward" else "loss"
    a = np.asarray(timed_out.detach().float().cpu().numpy(), np.float32)
    if a.size > DUMP_MAX_ELEMS:
        idx = np.sort(np.random.default_rng(0).integers(0, a.size, DUMP_MAX_ELEMS))
        a = a.reshape(-1)[idx]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + ".npy")
    np.save(path, a)
    return path


COMPACT_LIMIT = 4096              # the driver keeps 8 KB of stdout; the line it parses must stay far below that
ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic", "clock_mhz_under_load",
             "frac_clock_adjusted")


def _compact_roofline(roof, full=True):
    """The roofline object without prose: numbers + a short kernel name."""
    if not roof:
        return None
    out = {k: roof[k] for k in ROOF_KEYS if k in roof}
    if "kernel" in out:
        out["kernel"] = out["kernel"].split(" (")[0][:48]
    if not full:
        out = {k: out[k] for k in ("achieved", "frac", "traffic_over_algorithmic") if k in out}
    return out


def _compact_side(obj):
    """A side configuration on the stdout line: one flat object {ms_per_step, value, frac, ...}."""
    if not isinstance(obj, dict):
        return None
    if "error" in obj:
        return {"error": str(obj["error"])[:120]}
    out = {"ms_per_step": obj.get("ms_per_step"), "value": obj.get("value")}
    roof = obj.get("roofline") or {}
    for k_out, k_in in (("frac", "frac"), ("achieved", "achieved"), ("traffic_over_algorithmic", "traffic_over_algorithmic")):
        if roof.get(k_in) is not None:
            out[k_out] = roof[k_in]
    ar = obj.get("allreduce") or {}
    for k in ("exposed_ms", "standalone_ms", "busbw_GBps", "payload_bytes", "collectives_per_step"):
        if ar.get(k) is not None:
            out.setdefault("allreduce", {})[k] = ar[k]
    for prec in ("bf16x3", "f16x2"):
        alt = obj.get(prec)
        if isinstance(alt, dict) and "ms_per_step" in alt:
            out[prec] = {"ms_per_step": alt["ms_per_step"], "value": alt["value"], "frac": (alt.get("roofline") or {}).get("frac")}
    return out


def compact_line(full):
    """The ONE stdout line the driver parses: the contract keys, the roofline and cpu_baseline objects as
    numbers only and one flat triple per side configuration -- no prose.  The complete object (notes, per-family tables, provenance of
    every figure) goes to gpurun_out/bench_full.json and to stderr.  Always < COMPACT_LIMIT bytes: optional keys are dropped, in a fixed
    order, until it is (tests/test_host_cpu.py pins that on the stored round-5 object)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "data",
            "max_abs_logit_err", "gpu_over_cpu", "forward_tflops", "final_loss", "bench_wall_s")
    line = {k: full[k] for k in keep if k in full}
    line["dtype"] = str(full.get("dtype", "")).split(" ")[0].rstrip(",") or None
    comm = full.get("comm") or {}
    line["comm"] = {k: comm[k] for k in ("backend", "world_size", "rccl_version", "launcher") if k in comm}
    cfgo = dict(full.get("config") or {})
    if "workload" in cfgo:
        cfgo["workload"] = str(cfgo["workload"])[:120]
    line["config"] = cfgo
    if "roofline" in full:
        line["roofline"] = _compact_roofline(full["roofline"])
    cb = full.get("cpu_baseline")
    if cb:
        c = {k: cb[k] for k in ("value", "unit", "cores", "kind", "cpu_model") if k in cb}
        legs = {}
        for name, leg in (cb.get("legs") or {}).items():
            if "audio_s_per_s_best" in leg:
                legs[name] = {"best": leg["audio_s_per_s_best"], "median": leg["audio_s_per_s_median"]}
            elif "audio_s_per_s" in leg:
                legs[name] = {"best": leg["audio_s_per_s"], "workers": leg.get("workers")}
        if legs:
            c["legs"] = legs
            meds = [v["median"] for v in legs.values() if "median" in v]
            if meds:
                c["value_median"] = max(meds)
        c["sample"] = str(cb.get("sample", ""))[:160]
        line["cpu_baseline"] = c
    if "allreduce" in full:
        line["allreduce"] = {k: full["allreduce"][k] for k in ("payload_bytes", "buckets", "collectives_per_step", "payload_dtype", "backend",
                                                                 "world_size", "exposed_ms", "standalone_ms", "busbw_GBps", "engine")
                             if k in full["allreduce"]}
    for prec in ("bf16x3", "f16x2"):
        alt = full.get(prec)
        if isinstance(alt, dict) and "ms_per_step" in alt:
            line[prec] = {"ms_per_step": alt["ms_per_step"], "value": alt["value"], "frac": (alt.get("roofline") or {}).get("frac"),
                          "max_abs_logit_err": alt.get("max_abs_logit_err")}
    for name in ("configs2_train_bf16", "configs3_large_fwd_f32", "configs4_large_train_bf16"):
        if name in full:
            line[name] = _compact_side(full[name])
    if "full_object" in full:
        line["full_object"] = full["full_object"]
    # a hard guarantee, not a hope: shed optional keys until the line fits
    for victim in ("f16x2", "bf16x3", "forward_tflops", "comm", "configs3_large_fwd_f32", "configs4_large_train_bf16", "configs2_train_bf16",
                   "allreduce", "full_object"):
        if len(json.dumps(line)) < COMPACT_LIMIT:
            break
        line.pop(victim, None)
    return line


def emit(full):
    """Full object -> gpurun_out/bench_full.json + stderr; compact line -> stdout (the last line, the only one on stdout)."""
    path = os.path.join(ROOT, "gpurun_out", "bench_full.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f)
        full["full_object"] = "gpurun_out/bench_full.json (also on stderr)"
    except OSError:
        full["full_object"] = "stderr"
    print("BENCH_FULL " + json.dumps(full), file=sys.stderr, flush=True)
    out = json.dumps(compact_line(full))
    assert len(out) < COMPACT_LIMIT, len(out)
    print(out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="rows per GPU")
    ap.add_argument("--samples", type=int, default=246000)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: the per-family breakdown and the clock (extra untimed "
                         "steps), the split modes, the other BASELINE configurations, the CPU baseline, the logits against HF fp64, "
                         "the exposed collective of a multi-rank training leg.  Off: a plain run times the headline only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--cpu-baseline-only", action="store_true", help="run only the CPU leg (no GPU needed) and print its object")
    ap.add_argument("--no-alt", action="store_true", help="(--full) skip the bf16x3 / f16x2 measurements beside the fp32 forwards")
    ap.add_argument("--no-side", action="store_true",
                    help="(--full) skip the other BASELINE configurations measured beside the headline (configs[2] bf16 fine-tune step, "
                         "configs[3] large-robust fp32 forward, configs[4] large bf16 fine-tune step at 480000 samples)")
    ap.add_argument("--side-shrink", type=int, default=1, help="(--full, tests) divide the side legs' per-GPU batch by this factor")
    ap.add_argument("--side-legs", default="configs2_train_bf16,configs3_large_fwd_f32,configs4_large_train_bf16",
                    help="(--full, tests) comma-separated subset of the side legs to run")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket kernels with HIP events")
    ap.add_argument("--model", choices=["base", "large-robust"], default="base",
                    help="base = wav2vec2-base (the headline); large-robust = 24L/1024d prenorm, LayerNorm convs, conv bias, "
                         "attention mask (BASELINE configs[3] / [4] shapes, e.g. --batch 16 --samples 480000)")
    ap.add_argument("--precision", choices=["fp32", "bf16", "bf16x3", "f16x2"], default="fp32",
                    help="fp32 = the reference's arithmetic and the headline metric; bf16 = Dense / Conv1D operands rounded "
                         "to bf16 with fp32 accumulation (BASELINE configs[2]/[4] 'bf16 CTC fine-tune'), reported separately")
    ap.add_argument("--mode", choices=["forward", "train"], default="forward",
                    help="forward = BASELINE configs[1] (the headline metric); train = one CTC fine-tune step "
                         "(BASELINE configs[2] shape, fp32: forward + CTC + backward + gradient all-reduce + Adam)")
    ap.add_argument("--collective", choices=["torch", "native", "native-rs"], default=os.environ.get("W2V2_BENCH_COLLECTIVE", "torch"),
                    help="engine of the gradient SUM in the training legs: torch.distributed (default), or the library's own RCCL communicator "
                         "(include/w2v2.h w2v2_allreduce_bucket): native = ncclAllReduce, native-rs = ncclReduceScatter + ncclAllGather; needs --backend nccl")
    ap.add_argument("--backend", default=os.environ.get("W2V2_BENCH_BACKEND", "nccl"),
                    help="process-group backend: nccl (= RCCL, the default and the only one a result may be quoted on); gloo exists so the "
                         "N > 1 code path can be exercised by two processes on ONE GPU, which RCCL refuses (tests/test_dist_gpu.py)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0: logits of a forward, loss of a training "
                         "step) as DIR/<name>.npy in float32, for comparing two builds output for output")
    args = ap.parse_args()

    if args.cpu_baseline_only:
        # the cpu_baseline object alone (host cores only; the same call the N = 1 fp32 forward line makes after its timed region)
        sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))
        import wav2vec2
        from wav2vec2 import variables as V
        cfg = wav2vec2.Wav2Vec2Config()
        gold_wave, _ = golden_rows(args.samples)
        print(json.dumps({"cpu_baseline": cpu_baseline(cfg, V.seeded_weights(cfg, seed=0), args.samples, None if gold_wave is None else gold_wave[0])}))
        return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU under
        # torch.distributed.run, rendezvous on 127.0.0.1 at a free port) and pass rank 0's JSON line through.
        raise SystemExit(self_launch(args.gpus))

    t_start = time.perf_counter()
    import gc

    import torch
    import torch.distributed as dist

    import wav2vec2
    from wav2vec2 import dist as D
    from wav2vec2 import variables as V

    world, rank, local_rank = D.env_world()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size and --gpus must agree")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    local_dev = local_rank % torch.cuda.device_count() if args.backend != "nccl" else local_rank     # (gloo test: ranks may share a GPU)
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    # RCCL prints a version banner ("RCCL version : ...", five lines) on the process's stdout when its communicator is created: keep
    # stdout for the ONE JSON line -- file descriptor 1 points at stderr while the group comes up (init is eager with device_id) and
    # through a first barrier
    sys.stdout.flush()
    saved_fd = os.dup(1)
    os.dup2(2, 1)
    try:
        D.init(backend=args.backend, device=dev)      # nccl = RCCL; no-op for a single un-launched process
        D.barrier(sync_device=torch.cuda.synchronize)
    finally:
        sys.stdout.flush()
        os.dup2(saved_fd, 1)
        os.close(saved_fd)
    comm = D.describe()                           # what the process group itself reports (echoed in the JSON line)
    if args.collective != "torch" and world > 1 and args.backend != "nccl":
        raise SystemExit("--collective native needs one GPU per rank (RCCL): use it with --backend nccl")
    ctx = {"torch": torch, "D": D, "W": wav2vec2, "dev": dev, "world": world, "rank": rank, "comm": comm, "collective": args.collective}

    spec = {"model": args.model, "precision": args.precision, "mode": args.mode, "B": args.batch, "L": args.samples,
            "steps": args.steps, "warmup": args.warmup, "profile": not args.no_profile, "extras": args.full}
    res, model, out = run_leg(ctx, spec)
    if args.dump_outputs and rank == 0:
        print(f"bench: outputs of the last timed step -> {dump_outputs(args.dump_outputs, args.mode, res['timed_out'])}", file=sys.stderr)
    cfg, B, L, T, x, amask = res["cfg"], res["B"], res["L"], res["T"], res["x"], res["amask"]
    elapsed, prof, logit_err, gold_wave = res["elapsed"], res["prof"], res.get("logit_err"), res["gold_wave"]
    gemm_family = res["family"]

    alts = {}
    if args.full and world == 1 and args.mode == "forward" and args.precision == "fp32" and not args.no_alt:
        for prec in ("bf16x3", "f16x2"):
            try:                                               # never let the side measurement cost the headline line
                alts[prec] = measure_alt(ctx, model, x, amask, args.model, B, L, args.steps, max(1, args.warmup), prec, out, res.get("gold_logits"),
                                         not args.no_profile)
            except Exception as exc:                           # noqa: BLE001
                alts[prec] = {"precision": prec, "error": repr(exc)}

    line = None
    if rank == 0:
        audio_s = world * B * L / SAMPLE_RATE * args.steps
        line = {
            "metric": f"audio-seconds/s (wav2vec2-{args.model} forward, {L}-sample pad)" if args.mode == "forward"
                      else f"audio-seconds/s (wav2vec2-{args.model} CTC fine-tune step, {L}-sample pad)",
            "value": round(audio_s / elapsed, 2),
            "unit": "audio-seconds/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": DTYPE_OF[args.precision],
            "data": "synthetic",
            "comm": comm,
            "config": {"workload": (f"wav2vec2-{args.model} {args.precision} forward-only, batch={B}x{L} samples per GPU"
                                    + (" (BASELINE configs[1])" if (args.model, B, L, args.precision) == ("base", 32, 246000, "fp32") else "")
                                    if args.mode == "forward" else
                                    f"wav2vec2-{args.model} CTC fine-tune step, {args.precision} contractions (conv stack frozen, "
                                    f"dropout 0.1, spec-augment, Adam, fp32 variables / optimizer state), batch={B}x{L} per GPU"
                                    + (" (BASELINE configs[2]/[4] name bf16: see --precision bf16)" if args.precision == "fp32" else
                                       " (BASELINE configs[2]/[4] arithmetic)")),
                       "global_batch": world * B, "samples": L, "frames": T, "parallelism": f"dp{world}"},
        }
        if prof:
            roof = roofline_of(res, spec, args.steps)
            if B == DEFAULT_BATCH.get(args.model):
                add_traffic(roof, args.model, args.precision, args.mode, L)
            elif roof is not None:
                roof["traffic"], roof["traffic_source"] = None, "PMC profiles are kept for the BASELINE batch sizes only"
            add_clock(roof, res.get("clock"))
            line["roofline"] = roof
        if "prof_all" in res:
            fam, unattr, kernels, flops_step = families_of(res, world, args.steps)
            line["families"] = fam
            line["unattributed_ms"] = unattr
            line["kernel_launches_per_step"] = kernels
            line["families_note"] = ("per-family breakdown from 2 extra untimed steps with every family instrumented; share = family ms / the TIMED "
                                     "ms_per_step, unattributed_ms = the rest (launch gaps, host time, un-instrumented work)")
            # whole-forward algorithmic rate: 235.56 GFLOP per 246000-sample utterance scales with T
            line["forward_tflops"] = round(flops_step * world / (elapsed / args.steps) / 1e12, 2)
        if logit_err is not None:
            line["max_abs_logit_err"] = logit_err
            line["logit_err_note"] = ("rows 0-1 of the timed batch = tests/golden/base_sample_padded.npz (sample.wav normalised + zero-padded to "
                                      f"{L}, and a noise row); max |logits - HF-PyTorch fp64 logits| over both rows, max over ranks; bar "
                                      + ("1e-3 (BASELINE.json; the reference's TF-vs-HF bar)" if args.precision != "bf16" else "0.15 (bf16 mode, self-declared)"))
        for prec, alt in alts.items():
            line[prec] = alt
        if "final_loss" in res:
            line["final_loss"] = res["final_loss"]
        if "allreduce" in res:
            line["allreduce"] = res["allreduce"]

    # ---- with --full, the other BASELINE configurations, measured by this same command beside the headline (every rank takes part:
    # the two training legs run the bucketed RCCL gradient all-reduce when N > 1).  Each leg is guarded: a failure is reported in its
    # object and never costs the headline line.
    side_legs = (args.full and not args.no_side
                 and (args.model, args.precision, args.mode, args.batch, args.samples) == ("base", "fp32", "forward", 32, 246000))
    if side_legs and rank == 0:
        try:                                                   # insurance: the headline as measured, on disk before anything else runs
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "bench_headline.json"), "w") as f:
                json.dump(line, f)
        except OSError:
            pass
    if side_legs:
        del model, out, x, amask, res
        gc.collect()
        k = max(1, args.side_shrink)
        # the side legs time --steps steps after --warmup ones, like the headline (the shrunken legs exist for the multi-process tests:
        # at most 3 + 1 there, to keep them short)
        side_steps, side_warm = (args.steps, args.warmup) if k == 1 else (min(3, args.steps), min(1, args.warmup))
        legs = [("configs2_train_bf16", {"model": "base", "precision": "bf16", "mode": "train", "B": 32 // k, "L": 246000, "steps": side_steps, "warmup": side_warm},
                 "BASELINE configs[2] per-GPU shard: wav2vec2-base CTC fine-tune step, bf16 contractions (conv stack frozen, dropout 0.1, "
                 "spec-augment, Adam, fp32 variables / optimizer state), 32 x 246000 per GPU (global batch 256 at 8 GPUs)"),
                ("configs3_large_fwd_f32", {"model": "large-robust", "precision": "fp32", "mode": "forward", "B": 16 // k, "L": 246000, "steps": side_steps, "warmup": side_warm},
                 "BASELINE configs[3]: wav2vec2-large-robust (24L / 1024d, prenorm, LayerNorm convs, attention mask) fp32 forward, 16 x 246000 on 1 GPU"),
                ("configs4_large_train_bf16", {"model": "large-robust", "precision": "bf16", "mode": "train", "B": 16 // k, "L": 480000, "steps": side_steps, "warmup": side_warm},
                 "BASELINE configs[4] per-GPU shard: large (24L / 1024d; xlsr-53 is run as the robust architecture, SURVEY 8d) bf16 CTC fine-tune "
                 "step, 16 x 480000 per GPU (global batch 128 at 8 GPUs)")]
        keep = None                                            # the large model is built once and serves configs[3] and [4]
        wanted = {n.strip() for n in args.side_legs.split(",") if n.strip()}
        unknown = wanted - {n for n, _, _ in legs}
        if unknown:
            raise SystemExit(f"--side-legs: unknown leg(s) {sorted(unknown)}")
        legs = [leg for leg in legs if leg[0] in wanted]
        for name, sp, label in legs:
            sp["profile"] = not args.no_profile
            t_leg = time.perf_counter()
            try:
                reuse = keep if sp["model"] == "large-robust" else None
                r, m2, o2 = run_leg(ctx, sp, model=reuse)
                obj = side_object(ctx, sp, r, label) if rank == 0 else None
                if name == "configs3_large_fwd_f32" and world == 1 and not args.no_alt:
                    # the same forward in the two fp32-grade split modes (single process; each guarded like the leg itself)
                    for prec in ("bf16x3", "f16x2"):
                        try:
                            obj[prec] = measure_alt(ctx, m2, r["x"], r["amask"], sp["model"], r["B"], r["L"], sp["steps"], sp["warmup"], prec, o2, None,
                                                    sp["profile"])
                        except Exception as exc:               # noqa: BLE001
                            obj[prec] = {"precision": prec, "error": repr(exc)[:400]}
                keep = m2 if sp["model"] == "large-robust" else None
                del r, o2, m2
            except Exception as exc:                           # noqa: BLE001 -- reported, the headline still prints
                obj = {"workload": label, "error": repr(exc)[:400]}
                keep = None
                failed = 1
            else:
                failed = 0
            if world > 1:
                # every rank learns whether ANY rank failed this leg (a failure all ranks share -- out of memory, an unsupported shape --
                # reaches this point on all of them; one that hits a single rank inside a collective cannot be recovered from without
                # aborting the group, which is why the headline line is also kept in gpurun_out/bench_headline.json before the legs)
                if D.max_over_ranks(float(failed), device=dev) > 0 and not failed:
                    obj = {"workload": label, "error": "another rank failed this leg"} if rank == 0 else None
                    keep = None
            gc.collect()
            if rank == 0:
                obj["leg_wall_s"] = round(time.perf_counter() - t_leg, 1)
                line[name] = obj
        del keep
        gc.collect()

    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline and args.mode == "forward" and args.model == "base" and args.precision == "fp32":
            try:
                line["cpu_baseline"] = cpu_baseline(cfg, V.seeded_weights(cfg, seed=0), L, None if gold_wave is None else gold_wave[0])
                if line["cpu_baseline"]["value"]:
                    line["gpu_over_cpu"] = round(line["value"] / line["cpu_baseline"]["value"], 1)
            except Exception as exc:                           # noqa: BLE001 -- the GPU line must still be printed
                line["cpu_baseline"] = {"value": None, "unit": "audio-seconds/s", "cores": 0, "kind": "port",
                                        "sample": f"CPU baseline failed: {exc!r}"}
        line["bench_wall_s"] = round(time.perf_counter() - t_start, 1)
        emit(line)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
