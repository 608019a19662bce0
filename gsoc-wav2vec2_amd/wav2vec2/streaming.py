"""Streaming transcription: audio that arrives while it is spoken, transcribed as it arrives.

``stream_plan``       which windows of ``wav2vec2.longform.window_plan`` can be computed from the samples received so far;
``StreamingSession``  per stream a device buffer of the samples not yet consumed; every ``feed`` runs the windows that are ready,
                      of all streams, in ONE ``w2v2_forward_windows`` call and ONE ``wav2vec2.decoding.BeamStream.advance``;
                      ``finish`` runs what is left and returns the transcripts.

The plan is host code over a few integers; everything that touches samples, frames or logits is a HIP kernel.  The windows lie
on ``window_plan``'s fixed grid and each is computed as if alone, so the logits a session produces are, bit for bit, the rows
``predict_long`` returns for the finished recording, and the beam is resumed with the bits of one search over all of them: the
transcript of ``finish`` is the transcript of ``beam_search`` on ``predict_long``'s logits, however the audio was cut into chunks.
"""

from typing import NamedTuple

import numpy as np

from . import _native as N
from .longform import seconds_to_samples, total_stride, window_plan


def stream_plan(received, done_windows, window, margin, config, final=False):
    """The windows of a recording that can be computed now: ``received`` samples are in, the first ``done_windows`` windows of the
    plan were returned by earlier calls.  Growing recording: ``window_plan(received, ...)[done_windows:]`` without its last entry;
    ``final=True`` (no more samples will come): all of ``window_plan(received, ...)[done_windows:]``.

    Why the last entry is held back: for every R <= N, ``window_plan(R)[:-1]`` is a prefix of ``window_plan(N)``, but the last
    window of ``window_plan(R)`` keeps its rows to the end of the R samples and may be cut short, which a longer recording would
    not do.  In particular a recording that ends exactly at k H + window makes window k its last; only when one more sample has
    arrived is it known to be an inner window.  Too few samples for one frame give no window (``final`` or not)."""
    received, done_windows = int(received), int(done_windows)
    if done_windows < 0:
        raise ValueError(f"done_windows {done_windows} is negative")
    if config.num_frames(received) < 1:
        window_plan(max(received, 0) + window, window, margin, config)       # (the checks of window and margin)
        return []
    plan = window_plan(received, window, margin, config)
    return plan[done_windows:] if final else plan[done_windows:-1]


class Partial(NamedTuple):
    text: str           # the best hypothesis of everything decoded so far
    stable_text: str    # the part of it that can no longer change; it only ever grows
    ids: tuple          # the best hypothesis' label ids
    stable_len: int     # leading ids shared by every entry of the beam
    frames: int         # frames decoded so far
    seconds: float      # the audio they cover


class StreamingSession:
    """See ``Wav2Vec2ForCTC.stream``."""

    def __init__(self, model, tokenizer, n_streams=1, window_s=8.0, margin_s=2.0, beam_width=16, nbest=1, lm=None, bias=None,
                 normalize=True, keep_logits=False, sampling_rate=16000, window=None, margin=None):
        import torch
        from .decoding import BeamStream
        from .modeling import _require_gpu
        _require_gpu()
        if sampling_rate is not None and int(sampling_rate) != 16000:
            raise ValueError(f"a streaming session takes 16 kHz audio, not {sampling_rate} Hz: resample the chunks with a filter "
                             "that carries its state across them first")
        if not model._with_lm_head:
            raise ValueError("a streaming session needs a model with the CTC head")
        if model.precision == "bf16" and not model.get_option("bf16_packed"):
            raise RuntimeError('a streaming session runs the windowed forward, which takes the precision modes "fp32", "bf16x3" and '
                               '"f16x2"; the model is in "bf16" (set_option("bf16_packed", True) lets it through)')
        cfg = model.config
        w_s, m_s = seconds_to_samples(window_s, margin_s, cfg)
        self.window = w_s if window is None else int(window)
        self.margin = m_s if margin is None else int(margin)
        window_plan(self.window, self.window, self.margin, cfg)               # (the checks of window and margin)
        self.model, self.tokenizer, self.n = model, tokenizer, int(n_streams)
        self.normalize, self.keep_logits = bool(normalize), bool(keep_logits)
        self.hop = self.window - 2 * self.margin
        self.seconds_per_frame = float(total_stride(cfg)) / 16000.0
        self.beams = BeamStream(self.n, cfg.vocab_size, beam_width=beam_width, nbest=nbest, blank=cfg.pad_id, lm=lm, bias=bias)
        self.device = self.beams.device
        self._buf = [torch.empty(0, dtype=torch.float32, device=self.device) for _ in range(self.n)]
        self._buf0 = [0] * self.n               # the recording's sample at _buf[i][0]: the next unfinished window's start
        self.received = [0] * self.n
        self.done_windows = [0] * self.n
        self._kept = [[] for _ in range(self.n)]
        self._partial = [Partial("", "", (), 0, 0, 0.0) for _ in range(self.n)]
        self._finished = False

    # ---- the two halves ------------------------------------------------------------------------------------------------------------
    def _forward(self, plans):
        """the windows ``plans[i]`` of every stream in one w2v2_forward_windows call: per stream its new logits rows (a view of the
        call's output) or None"""
        import torch
        model, cfg = self.model, self.model.config
        streams = [i for i, p in enumerate(plans) if p]
        if not streams:
            return [None] * self.n
        parts, sample0, samples, keep0, keepn, base = [], [], [], [], [], 0
        for i in streams:
            for w in plans[i]:
                sample0.append(w.sample0 - self._buf0[i] + base)
                samples.append(w.samples)
                keep0.append(w.keep0)
                keepn.append(w.keepn)
            parts.append(self._buf[i])
            base += int(self._buf[i].shape[0])
        wave = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
        rows = [sum(w.keepn for w in plans[i]) for i in streams]
        out = torch.empty((sum(rows), cfg.vocab_size), device=self.device, dtype=torch.float32)
        model._finalize()
        sample0, samples = np.asarray(sample0, np.int64), np.asarray(samples, np.int64)
        keep0, keepn = np.asarray(keep0, np.int32), np.asarray(keepn, np.int32)
        N.check(model._lib.w2v2_forward_windows(model._handle, N.ptr(wave), base, len(sample0), N.ptr(sample0), N.ptr(samples),
                                                N.ptr(keep0), N.ptr(keepn), int(self.normalize), N.ptr(out), N.current_stream()),
                "w2v2_forward_windows")
        new = [None] * self.n
        for i, piece in zip(streams, torch.split(out, rows, dim=0)):
            new[i] = piece
            self.done_windows[i] += len(plans[i])
            start = self.done_windows[i] * self.hop                 # (only a recording's last window can be missing from its plan)
            drop = min(start - self._buf0[i], int(self._buf[i].shape[0]))
            self._buf[i] = self._buf[i][drop:]
            self._buf0[i] += drop
            if self.keep_logits:
                self._kept[i].append(piece)
        return new

    def _decode(self, new):
        steps = self.beams.advance(new)
        for i, st in enumerate(steps):
            if new[i] is None and self._partial[i].frames == st.frames_done:
                continue
            old = self._partial[i]
            if st.hypotheses:
                ids = st.hypotheses[0].ids
                text = self.tokenizer.decode(ids, skip_special_tokens=True, group_tokens=False)
                stable = self.tokenizer.decode(ids[:st.stable_len], skip_special_tokens=True, group_tokens=False)
                self._partial[i] = Partial(text, stable, ids, st.stable_len, st.frames_done, st.frames_done * self.seconds_per_frame)
            else:                                                   # no hypothesis (a dead stream, or a lexicon left): nothing new is promised
                self._partial[i] = Partial("", old.stable_text, (), old.stable_len, st.frames_done,
                                           st.frames_done * self.seconds_per_frame)
        return steps

    # ---- the interface -------------------------------------------------------------------------------------------------------------
    def feed(self, chunks, sampling_rate=None):
        """Append one chunk per stream (a 1-D array or tensor of 16 kHz samples, or None) and decode every window that became
        ready.  Returns one ``Partial(text, stable_text, ids, stable_len, frames, seconds)`` per stream.  ``sampling_rate``: None
        or 16000; any other rate is a ValueError."""
        import torch
        if self._finished:
            raise RuntimeError("the session is finished")
        if sampling_rate is not None and int(sampling_rate) != 16000:
            raise ValueError(f"a streaming session takes 16 kHz audio, not {sampling_rate} Hz")
        if self.n == 1 and (chunks is None or getattr(chunks, "ndim", 0) == 1):
            chunks = [chunks]
        chunks = list(chunks)
        if len(chunks) != self.n:
            raise ValueError(f"{len(chunks)} chunks for {self.n} streams")
        for i, c in enumerate(chunks):
            if c is None:
                continue
            if not isinstance(c, torch.Tensor):
                c = torch.as_tensor(np.asarray(c, dtype=np.float32))
            if c.dim() != 1:
                raise ValueError(f"stream {i}: a chunk must be 1-D, got shape {tuple(c.shape)}")
            if c.shape[0]:
                self._buf[i] = torch.cat([self._buf[i], c.to(device=self.device, dtype=torch.float32)])
                self.received[i] += int(c.shape[0])
        plans = [stream_plan(self.received[i], self.done_windows[i], self.window, self.margin, self.model.config)
                 for i in range(self.n)]
        if any(plans):
            self._decode(self._forward(plans))
        return list(self._partial)

    def logits(self, i=0):
        """the logits of stream ``i`` decoded so far (``keep_logits=True``): ``predict_long``'s rows of the recording"""
        import torch
        if not self.keep_logits:
            raise ValueError("the session was opened without keep_logits=True")
        kept = self._kept[i]
        if not kept:
            return torch.empty((0, self.model.config.vocab_size), dtype=torch.float32, device=self.device)
        return kept[0] if len(kept) == 1 else torch.cat(kept)

    def finish(self, timestamps=False):
        """No more audio: run the windows that were held back (``stream_plan`` with ``final=True``), advance the beams a last time
        and return one ``wav2vec2.decoding.Transcript(text, hypotheses, texts, words)`` per stream.  ``timestamps=True`` needs
        ``keep_logits=True`` (else ValueError): the best hypothesis is aligned to the kept logits with ``forced_align`` (or
        ``forced_align_long`` beyond its label limit).  A stream that received less than one frame of audio, or died on a NaN,
        has an empty transcript."""
        from .alignment import forced_align, forced_align_long, token_spans, word_spans
        from .decoding import Transcript
        from .processor import WORD_DELIMITER
        if self._finished:
            raise RuntimeError("the session is finished")
        if timestamps and not self.keep_logits:
            raise ValueError("timestamps=True needs the logits: open the session with keep_logits=True")
        plans = [stream_plan(self.received[i], self.done_windows[i], self.window, self.margin, self.model.config, final=True)
                 for i in range(self.n)]
        steps = self._decode(self._forward(plans))
        self._finished = True
        self._buf = [b[:0] for b in self._buf]
        out = []
        for i, st in enumerate(steps):
            hyps = st.hypotheses or []
            texts = [h.text(self.tokenizer) for h in hyps]
            words = None
            if timestamps:
                words = []
                if hyps and hyps[0].ids:
                    tokens = self.tokenizer.get_vocab()
                    vocab = {k: (" " if t == WORD_DELIMITER else t) for t, k in tokens.items()}
                    align = forced_align_long if len(hyps[0].ids) > N.ALIGN_MAX_LABELS else forced_align
                    a = align([self.logits(i)], [list(hyps[0].ids)], blank=self.model.config.pad_id)[0]
                    words = word_spans(token_spans(a), tokens[WORD_DELIMITER], self.seconds_per_frame, vocab)
            out.append(Transcript(texts[0] if texts else "", hyps, texts, words))
        return out
