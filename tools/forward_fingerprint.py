#!/usr/bin/env python
"""Fingerprint of what the forwards compute, launch and leave readable, for comparing two builds of the library bit for bit (a
host-side restructuring of the forward must change none of it).

Runs a fixed matrix and prints one JSON object per entry:

  fixtures    tiny_base, tiny_robust, base_sample_padded x 8 copies, robust_full_246000 x 4 copies with its mask (the last two are
              the shapes at which every GEMM call site goes plane-fed)
  dense       precision fp32 / bf16 / bf16x3 / f16x2 x keep_activations off / on x bf16_shadows off / on (bf16) x split_planes
              off / on (bf16x3, f16x2)
  packed      predict_packed of three utterances of unequal length (cuts of the fixture's first row) in fp32 / bf16x3 / f16x2,
              same options
  train       one training forward + backward in fp32 / bf16 / bf16x3 with dropout 0 and 0.1, fixed seed, spec-augment off
  train_plan  tiny_base, tiny_robust and base dims at 3 x 24080 and 9 x 24080 samples (B T = 225: one weight-gradient slab; 675:
              three uneven slabs; both ragged): spec-augment on, a dropped layer,
              bf16_shadows off, defer_folds off / on, wgrad_stream on, only lm_head / only layer 0 trainable; each entry also holds
              Trainer.activation_storage() (`storage`, `storage_bytes`)

Each object holds the sha256 of the output bytes (`out`; train entries: the logits, and `grads` = the flat gradient buffer), the
per-family kernel-launch counts (`kernels`, profile_read() after a profile_reset()) and the sorted taps for which activation()
raises (`untappable`).  Select the library with W2V2_NATIVE_LIB and diff the two outputs:

    python tools/forward_fingerprint.py [--fixtures tiny_base,tiny_robust] [--skip-train] > fingerprint.json

The hashes belong to one compiler and one commit: no test depends on them.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsoc-wav2vec2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURES = ["tiny_base", "tiny_robust", "base_sample_padded", "robust_full_246000"]
COPIES = {"base_sample_padded": 8, "robust_full_246000": 4}


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def option_sets(precision):
    for keep in (False, True):
        if precision == "bf16":
            for shadows in (False, True):
                yield dict(keep_activations=keep, bf16_shadows=shadows)
        elif precision in ("bf16x3", "f16x2"):
            for planes in (False, True):
                yield dict(keep_activations=keep, split_planes=planes)
        else:
            yield dict(keep_activations=keep)


def build(name):
    import helpers as H
    import wav2vec2
    from wav2vec2 import variables as V
    g = H.golden(name)
    copies = COPIES.get(name, 1)
    wave = np.concatenate([g["wave"]] * copies, 0)
    mask = g.get("attention_mask")
    mask = None if mask is None else np.concatenate([mask.astype(np.int32)] * copies, 0)
    if name == "robust_full_246000":
        from wav2vec2.config import RobustWav2Vec2Config
        cfg = RobustWav2Vec2Config()
        weights = V.seeded_weights(cfg, seed=5)
    else:
        cfg = H.case_config(name)
        weights = H.case_weights(name)
    m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=wave.shape)
    m.set_weights(weights)
    return m, cfg, wave, mask


def train_plan_cases(cfg):
    """(precisions, options, keyword) of the training-step matrix: every switch the backward's decisions depend on."""
    n = cfg.num_layers
    drop = np.ones(n, dtype=np.float32)
    drop[max(0, n - 2)] = 0.0                                   # one dropped layer that is not the last
    all3, two = ("fp32", "bf16", "bf16x3"), ("fp32", "bf16")
    return [(all3, {}, dict(spec=True)),
            (all3, {}, dict(sd_keep=drop)),
            (("bf16",), dict(bf16_shadows=False), {}),
            (two, dict(defer_folds=False), {}),
            (two, dict(defer_folds=True), {}),
            (("bf16",), dict(wgrad_stream=True), {}),
            (two, {}, dict(trainable="lm_head/")),              # stage 1
            (two, {}, dict(trainable="encoder/layers/0/"))]


def train_plan(emit):
    """Training forward + backward of tiny_base, tiny_robust (postnorm + group norm, prenorm + layer norm + mask) and base dims at a
    ragged row count (3 and 9 x 24080 samples: B T = 225 and 675, H % 128 == 0) over train_plan_cases; each entry also records
    activation_storage()."""
    import helpers as H
    import torch
    import wav2vec2
    from wav2vec2 import variables as V
    from wav2vec2.spec_augment import compute_mask_indices
    from wav2vec2.training import Trainer
    for name, batch in (("tiny_base", 0), ("tiny_robust", 0), ("base_sample_padded", 3), ("base_sample_padded", 9)):
        if batch:
            cfg, mask = H.case_config(name), None
            wave = V.hash_normal("fingerprint/train_plan", batch * 24080, 8).reshape(batch, 24080)
            m = wav2vec2.Wav2Vec2ForCTC(cfg, input_shape=wave.shape)
            m.set_weights(H.case_weights(name))
        else:
            m, cfg, wave, mask = build(name)
        defaults = {k: m.get_option(k) for k in ("bf16_shadows", "defer_folds", "wgrad_stream")}
        T = cfg.num_frames(wave.shape[1])
        spec = compute_mask_indices((wave.shape[0], T), 0.05, 10, rng=np.random.RandomState(4))
        for precisions, opts, kw in train_plan_cases(cfg):
            for precision in precisions:
                m.set_precision(precision)
                for k, v in opts.items():
                    m.set_option(k, v)
                if "trainable" in kw:
                    m.set_trainable("", False)
                    m.set_trainable(kw["trainable"], True)
                else:
                    m.set_trainable("", True)
                    m.freeze_feature_extractor()
                tr = Trainer(m, None, seed=0, dropout=0.1, apply_spec_augment=False)
                m.profile_reset()
                sd_keep = kw.get("sd_keep", np.ones(cfg.num_layers, dtype=np.float32))
                logits = tr.forward(wave, attention_mask=mask, spec_mask=spec if kw.get("spec") else None, sd_keep=sd_keep, step_seed=1234)
                tr.backward(torch.sin(logits))
                names, nbytes = tr.activation_storage()
                tag = dict(opts, **{k: (v if isinstance(v, (str, bool)) else [float(x) for x in v]) for k, v in kw.items()})
                emit(dict(fixture=name, form="train_plan", precision=precision, batch=wave.shape[0], **tag), m, [], out=sha(logits), grads=sha(tr.grad_buffer()),
                     storage=sorted(names), storage_bytes=nbytes)
                for k, v in defaults.items():
                    m.set_option(k, v)
        del m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixtures", default=",".join(FIXTURES))
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-forward", action="store_true", help="only the train entries of --fixtures (and the train_plan matrix)")
    ap.add_argument("--skip-train-plan", action="store_true")
    args = ap.parse_args()

    import torch
    from wav2vec2.training import Trainer
    torch.cuda.set_device(0)

    def emit(entry, m, taps, **hashes):
        torch.cuda.synchronize()
        entry["kernels"] = {k: v["kernels"] for k, v in sorted(m.profile_read().items()) if v["kernels"]}
        untappable = []
        for tap in taps:
            try:
                m.activation(tap)
            except RuntimeError:
                untappable.append(tap)
        entry["untappable"] = sorted(untappable)
        entry.update(hashes)
        print(json.dumps(entry, sort_keys=True), flush=True)

    for name in args.fixtures.split(","):
        m, cfg, wave, mask = build(name)
        taps = [f"conv{i}" for i in range(len(cfg.kernal_sizes))] + ["projection", "encoder_in"] + \
               [f"layer{i}" for i in range(cfg.num_layers)] + ["encoder_out"]
        L = wave.shape[1]
        utterances = [wave[0, :L], wave[0, :(2 * L) // 3], wave[0, :L // 2 + 37]]
        for precision in () if args.skip_forward else ("fp32", "bf16", "bf16x3", "f16x2"):
            m.set_precision(precision)
            for opts in option_sets(precision):
                for k, v in opts.items():
                    m.set_option(k, v)
                m.profile_reset()
                out = m(wave, attention_mask=mask)
                emit(dict(fixture=name, form="dense", precision=precision, **opts), m, taps, out=sha(out))
                if precision != "bf16":
                    m.profile_reset()
                    outs = m.predict_packed(utterances)
                    emit(dict(fixture=name, form="packed", precision=precision, **opts), m, taps, out=sha(torch.cat(outs)))
            for k in ("keep_activations", "bf16_shadows", "split_planes"):
                m.set_option(k, k != "keep_activations")       # back to the defaults
        if args.skip_train:
            continue
        m.freeze_feature_extractor()                            # (it has no backward: the reference freezes it too)
        for precision in ("fp32", "bf16", "bf16x3"):
            m.set_precision(precision)
            for dropout in (0.0, 0.1):
                tr = Trainer(m, None, seed=0, dropout=dropout, apply_spec_augment=False)
                m.profile_reset()
                logits = tr.forward(wave, attention_mask=mask, sd_keep=np.ones(cfg.num_layers, dtype=np.float32), step_seed=1234)
                tr.backward(torch.sin(logits))                  # any fixed function of the logits
                emit(dict(fixture=name, form="train", precision=precision, dropout=dropout), m, taps, out=sha(logits),
                     grads=sha(tr.grad_buffer()))
        del m
        torch.cuda.empty_cache()
    if not (args.skip_train or args.skip_train_plan):
        train_plan(emit)


if __name__ == "__main__":
    main()
