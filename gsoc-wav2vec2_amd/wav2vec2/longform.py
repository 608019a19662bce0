"""Long recordings: the windowed forward and pause-segmented decoding.

A recording of minutes or hours is no utterance: the checkpoints were trained on at most 35 s, self-attention is quadratic in
the frames and the beam search is one serial sweep per utterance.  This module cuts a recording up and puts it back together:

``window_plan``   overlapping windows of the waveform, each frame of the recording taken from the window that holds the most
                  context around it;
``predict_long``  the windows of all recordings through ``w2v2_forward_windows`` (gathered on the device straight from the
                  recording, normalised per window there), stitched into one logits matrix per recording;
``pause_cuts``    where those logits pause (``w2v2_ctc_pause_cuts``, csrc/segment.hip);
``choose_cuts``   which of the pauses become segment boundaries;
``decode_long``   ONE ``beam_search`` call over the segments of all recordings, optionally ONE ``forced_align`` call, and the
                  pieces concatenated.

The plan and the choice of cuts are host code over a few numbers per window; everything that touches samples, frames or
logits is a HIP kernel.
"""

import bisect
from typing import NamedTuple

import numpy as np

from . import _native as N


class Window(NamedTuple):
    sample0: int    # first sample of the window in the recording
    samples: int    # its length
    keep0: int      # first of the window's own frame rows that is kept
    keepn: int      # rows kept
    out0: int       # global frame of the first kept row


def total_stride(config):
    """A: samples per frame, the product of the conv strides."""
    a = 1
    for s in config.strides:
        a *= int(s)
    return a


def window_plan(num_samples, window, margin, config):
    """The windows of one recording of ``num_samples`` samples: a list of ``Window(sample0, samples, keep0, keepn, out0)``.

    ``window`` and ``margin`` are in samples, multiples of A = ``total_stride(config)``, with ``margin >= A`` and
    ``window >= 2 * margin + A`` (else ValueError).  With H = window - 2 * margin and m = margin / A, window k covers samples
    [k H, min(k H + window, num_samples)); its local frame j is the recording's frame k H / A + j (both see samples
    [A g, A g + R)).  Frame g of the recording is taken from window clamp(floor((g - m) / (H / A)), 0, K - 1), K the number
    of windows that cover the recording: every kept frame's hop [A j, A j + A) has at least ``margin`` samples of its window
    on each side (m whole frames before it, m - 1 behind it: the window's last hop is short of a receptive field), except
    at the true start and end of the recording.  A window that owns no frame (this can happen to the last) is dropped;
    a recording no longer than ``window`` gives one window that keeps everything."""
    num_samples, window, margin = int(num_samples), int(window), int(margin)
    A = total_stride(config)
    if window % A or margin % A:
        raise ValueError(f"window {window} and margin {margin} must be multiples of the total stride {A}")
    if margin < A:
        raise ValueError(f"margin {margin} below one frame ({A} samples)")
    if window < 2 * margin + A:
        raise ValueError(f"window {window} below 2 * margin + {A} = {2 * margin + A}: no frame would be kept")
    F = config.num_frames(num_samples)
    if F < 1:
        raise ValueError(f"a recording of {num_samples} samples is shorter than the feature extractor's receptive field")
    H = window - 2 * margin
    h, m = H // A, margin // A
    K = max(1, -(-(num_samples - window) // H) + 1)
    plan = []
    for k in range(K):
        lo = 0 if k == 0 else k * h + m
        hi = F if k == K - 1 else min(F, (k + 1) * h + m)
        if hi <= lo:
            continue
        samples = min(window, num_samples - k * H)
        if lo - k * h + (hi - lo) > config.num_frames(samples):
            raise AssertionError("window_plan: a kept frame lies outside its window")
        plan.append(Window(k * H, samples, lo - k * h, hi - lo, lo))
    return plan


def seconds_to_samples(window_s, margin_s, config, rate=16000):
    """(window, margin) in samples: the seconds rounded to multiples of the total stride with ``round``."""
    A = total_stride(config)
    return int(round(window_s * rate / A)) * A, int(round(margin_s * rate / A)) * A


def group_windows(windows, max_stream_samples, config):
    """Consecutive windows grouped, in order, into packed calls: a list of (first, one past the last) index pairs.  A call's
    stream holds every window rounded up to whole frames; a group is closed when the next window would take the stream past
    ``max_stream_samples`` (a single window longer than that is a call of its own)."""
    A = total_stride(config)
    groups, first, used = [], 0, 0
    for i, w in enumerate(windows):
        need = -(-int(w.samples) // A) * A
        if i > first and used + need > max_stream_samples:
            groups.append((first, i))
            first, used = i, 0
        used += need
    if len(windows) > first:
        groups.append((first, len(windows)))
    return groups


def predict_long(model, waveform, window_s=20.0, margin_s=2.0, normalize=True, max_stream_s=1200.0, window=None, margin=None,
                 sampling_rate=None):
    """See ``TFKerasModel.predict_long``.  ``window`` / ``margin`` (samples of the 16 kHz audio) override the seconds."""
    import torch
    from .modeling import DeviceTensor, _require_gpu
    _require_gpu()
    single = isinstance(waveform, (np.ndarray, torch.Tensor)) and getattr(waveform, "ndim", 0) == 1
    recordings = [waveform] if single else list(waveform)
    if not recordings:
        raise ValueError("`waveform` must be a 1-D waveform or a non-empty list of them")
    if sampling_rate is not None and sampling_rate != 16000:
        from .audio import resample
        recordings = resample(recordings, sampling_rate)
    cfg = model.config
    w_s, m_s = seconds_to_samples(window_s, margin_s, cfg)
    window = w_s if window is None else int(window)
    margin = m_s if margin is None else int(margin)
    dev = torch.device("cuda", torch.cuda.current_device())
    parts, windows, frames, base = [], [], [], 0
    for i, w in enumerate(recordings):
        if not isinstance(w, torch.Tensor):
            w = torch.as_tensor(np.asarray(w, dtype=np.float32))
        if w.dim() != 1:
            raise ValueError(f"recording {i} must be 1-D, got shape {tuple(w.shape)}")
        n = int(w.shape[0])
        if cfg.num_frames(n) < 1:
            raise ValueError(f"recording {i} has {n} samples, shorter than the feature extractor's receptive field")
        for p in window_plan(n, window, margin, cfg):
            windows.append(p._replace(sample0=p.sample0 + base))
        parts.append(w.to(device=dev, dtype=torch.float32))
        frames.append(cfg.num_frames(n))
        base += n
    model._finalize()
    wave = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
    width = cfg.vocab_size if model._with_lm_head else cfg.hidden_size
    out = torch.empty((sum(frames), width), device=dev, dtype=torch.float32)
    sample0 = np.asarray([p.sample0 for p in windows], np.int64)
    samples = np.asarray([p.samples for p in windows], np.int64)
    keep0 = np.asarray([p.keep0 for p in windows], np.int32)
    keepn = np.asarray([p.keepn for p in windows], np.int32)
    row0 = np.concatenate(([0], np.cumsum(keepn, dtype=np.int64)))
    assert row0[-1] == out.shape[0]
    for a, b in group_windows(windows, int(max_stream_s * 16000), cfg):
        N.check(model._lib.w2v2_forward_windows(model._handle, N.ptr(wave), base, b - a, N.ptr(sample0[a:b]), N.ptr(samples[a:b]),
                                                N.ptr(keep0[a:b]), N.ptr(keepn[a:b]), int(bool(normalize)),
                                                N.ptr(out[int(row0[a]):]), N.current_stream()), "w2v2_forward_windows")
    out = DeviceTensor.wrap(out)
    return out if single else list(torch.split(out, frames, dim=0))


def normalize_windows(wave, sample0, samples):
    """``w2v2_op_normalize_windows``: the windows ``wave[sample0_i : sample0_i + samples_i]`` of a 1-D device tensor, each
    normalised over its own samples as ``Wav2Vec2Processor._normalize`` does it, back to back in one new tensor."""
    import torch
    sample0 = np.ascontiguousarray(sample0, np.int64)
    samples = np.ascontiguousarray(samples, np.int64)
    if sample0.shape != samples.shape or sample0.ndim != 1 or not sample0.size:
        raise ValueError("`sample0` and `samples`: one entry per window, at least one window")
    if (sample0 < 0).any() or (samples < 1).any() or (sample0 + samples > wave.shape[0]).any():
        raise ValueError("a window lies outside the waveform or is empty")
    wave = wave.to(device="cuda", dtype=torch.float32).contiguous()
    out = torch.empty(int(samples.sum()), dtype=torch.float32, device=wave.device)
    N.check(N.load().w2v2_op_normalize_windows(N.ptr(wave), int(sample0.size), N.ptr(sample0), N.ptr(samples), N.ptr(out),
                                               N.current_stream()), "w2v2_op_normalize_windows")
    return out


class PauseCuts(NamedTuple):
    cuts: np.ndarray      # the stored cuts (frames), ascending
    pauses: np.ndarray    # the length of each cut's pause (frames)
    count: int            # the true number of pauses; len(cuts) = min(count, max_cuts)


def pause_cuts(logits, blank=0, delimiter_id=None, margin=2.0, min_pause=10, max_cuts=None, frame_lengths=None):
    """The pauses of each utterance's logits (``w2v2_ctc_pause_cuts``; exact definition in include/w2v2.h): one
    ``PauseCuts(cuts, pauses, count)`` per utterance.  ``logits``: what ``beam_search`` accepts, read in place.  A frame is
    quiet when its argmax is the blank and the blank's logit leads every other by at least ``margin``; a pause is a maximal run
    of at least ``min_pause`` quiet frames strictly inside the utterance; with ``delimiter_id`` it counts only where the last
    label of the greedy path before it is the word delimiter.  ``max_cuts`` defaults to what an utterance can hold."""
    import torch
    from .alignment import _logits_base
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    blank, min_pause = int(blank), int(min_pause)
    delim = -1 if delimiter_id is None else int(delimiter_id)
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    if delim != -1 and (not 0 <= delim < V or delim == blank):
        raise ValueError(f"delimiter {delim} must be a label of the vocabulary [0, {V}) other than the blank {blank}")
    if min_pause < 1:
        raise ValueError(f"min_pause {min_pause}: at least one frame")
    if max(lens) > N.CUTS_MAX_FRAMES:
        raise ValueError(f"an utterance of {max(lens)} frames; at most {N.CUTS_MAX_FRAMES}")
    if max_cuts is None:
        max_cuts = max(lens) // (min_pause + 1) + 1       # (a pause needs min_pause quiet frames and one that ends it)
    max_cuts = int(max_cuts)
    if max_cuts < 1:
        raise ValueError(f"max_cuts {max_cuts}: at least one")
    dev = base.device
    cut = torch.empty((n, max_cuts), dtype=torch.int32, device=dev)
    pause = torch.empty((n, max_cuts), dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    row0_h = np.asarray(row0, np.int64)
    frames_h = np.asarray(lens, np.int32)
    N.check(N.load().w2v2_ctc_pause_cuts(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), blank, delim, float(margin), min_pause,
                                         max_cuts, N.ptr(cut), N.ptr(pause), N.ptr(count), N.current_stream()), "w2v2_ctc_pause_cuts")
    count_h, cut_h, pause_h = count.cpu().numpy(), cut.cpu().numpy(), pause.cpu().numpy()
    return [PauseCuts(cut_h[i, :min(int(c), max_cuts)].copy(), pause_h[i, :min(int(c), max_cuts)].copy(), int(c))
            for i, c in enumerate(count_h)]


def choose_cuts(cuts, pauses, T, min_frames=250, max_frames=1500):
    """Segment boundaries among the candidate ``cuts`` (ascending frames in (0, T), ``pauses`` their pauses' lengths).
    Walking from ``last = 0``: the LAST candidate in (last + min_frames, last + max_frames]; if there is none, the FIRST
    candidate beyond last + max_frames.  ``max_frames`` is therefore a target and not a bound: a stretch without a pause
    stays one long segment.  Returns the chosen cuts, ascending."""
    cuts = [int(c) for c in cuts]
    if len(pauses) != len(cuts):
        raise ValueError(f"{len(cuts)} cuts with {len(pauses)} pause lengths")
    if min_frames < 0 or max_frames <= min_frames:
        raise ValueError(f"need 0 <= min_frames < max_frames, got {min_frames} and {max_frames}")
    if any(b <= a for a, b in zip(cuts, cuts[1:])) or (cuts and not (0 < cuts[0] and cuts[-1] < T)):
        raise ValueError(f"cuts must ascend strictly inside (0, {T})")
    chosen, last = [], 0
    while True:
        lo = bisect.bisect_right(cuts, last + min_frames)       # first candidate > last + min_frames
        hi = bisect.bisect_right(cuts, last + max_frames)       # first candidate > last + max_frames
        if hi > lo:
            last = cuts[hi - 1]
        elif hi < len(cuts):
            last = cuts[hi]
        else:
            return chosen
        chosen.append(last)


class Segment(NamedTuple):
    start_s: float
    end_s: float
    transcript: object    # the segment's own wav2vec2.decoding.Transcript (its n-best; word times relative to the segment)


class LongTranscript(NamedTuple):
    text: object          # the ids as text (None without a tokenizer)
    ids: tuple            # the segments' best hypotheses, concatenated
    score: float          # sum of the best hypotheses' scores (NaN on the greedy path)
    total: float          # sum of their totals
    words: object         # WordSpans in the recording's time (timestamps=True), else None
    segments: list        # Segment(start_s, end_s, transcript)


class ScoredLongTranscript(NamedTuple):
    text: object          # as LongTranscript
    ids: tuple
    score: float          # sum of the best hypotheses' exact scores
    total: float
    words: list           # WordSpans in the recording's time
    segments: list        # Segment(start_s, end_s, transcript), the transcript a wav2vec2.decoding.ScoredTranscript
    confidence: float     # geometric mean of the segments' confidences, weighted by their word counts (NaN without a word)
    word_confidence: list # parallel to ``words``: each word's confidence within its segment


def _collapse(path, blank):
    keep = np.flatnonzero((path != blank) & (np.concatenate(([True], path[1:] != path[:-1]))))
    return tuple(int(v) for v in path[keep])


def decode_long(logits, tokenizer=None, beam_width=16, nbest=1, lm=None, blank=0, delimiter_id=None, timestamps=False,
                pause_margin=2.0, min_pause=10, min_frames=250, max_frames=1500, seconds_per_frame=0.02, rescore=False,
                confidence=False, posterior_scale=1.0, bias=None):
    """Transcripts of long recordings from their logits: one ``LongTranscript`` per recording (a single (T, V) tensor gives one
    result, a list gives a list).  Model-free, like ``beam_search``.

    The logits are cut at pauses (``pause_cuts`` with ``pause_margin`` / ``min_pause``, then ``choose_cuts`` with
    ``min_frames`` / ``max_frames``) into views; ALL segments of ALL recordings go through ONE ``beam_search`` call
    (``beam_width=None``: the argmax of every frame instead) and, with ``timestamps=True``, the best hypothesis of every
    non-empty segment through ONE ``forced_align`` call.  ``delimiter_id`` (default: the tokenizer's ``|``) makes a pause count
    only between words of the greedy path, so that a constrained word LM never sees half a word at a segment's end.

    A cut lies inside a run of frames whose argmax is the blank, so no repeated label can merge across it: for the greedy
    decode the collapse of the whole equals the concatenation of the collapses of the pieces, and ``ids`` is the
    concatenation of the segments' best hypotheses; ``text`` decodes ``ids`` without grouping.  A language model sees every
    segment as an utterance: a ``WordNgramLM`` restarts from its start state at each segment and scores ``</s>`` at each
    segment's end when its ``score_eos`` is set; no LM state or beam entry is carried across a cut.  ``bias`` (a ``ContextBias``)
    likewise restarts at its start state in every segment and settles its end-of-utterance term at every segment's end.

    ``rescore=True``: the segments' n-best lists go through ONE ``wav2vec2.decoding.rescore`` call (exact scores, lists ordered
    by the exact totals) before anything is made of them.  ``confidence=True`` (implies ``rescore``; needs a beam with
    ``nbest >= 2``, else ValueError) aligns ALL hypotheses of all segments in one ``forced_align`` call and returns
    ``ScoredLongTranscript``: posteriors are per segment (each ``Segment.transcript`` a ``ScoredTranscript``), a word's confidence
    comes from its segment, and the recording's ``confidence`` is the geometric mean of its segments' confidences weighted by
    their word counts."""
    import math
    import torch
    from .alignment import forced_align, token_spans, word_spans
    from .decoding import Hypothesis, Transcript, beam_search
    from .decoding import rescore as rescore_lists, score_transcripts
    from .processor import WORD_DELIMITER
    single = isinstance(logits, torch.Tensor)
    recs = [logits] if single else list(logits)
    if not recs or any(not isinstance(l, torch.Tensor) or l.dim() != 2 or l.shape[0] < 1 for l in recs):
        raise ValueError("`logits` must be a (T, V) tensor or a non-empty list of them")
    vocab = None
    if tokenizer is not None:
        tokens = tokenizer.get_vocab()
        vocab = {i: (" " if t == WORD_DELIMITER else t) for t, i in tokens.items()}
        if delimiter_id is None:
            delimiter_id = tokens[WORD_DELIMITER]
    if timestamps and delimiter_id is None:
        raise ValueError("timestamps without a tokenizer: pass delimiter_id")
    if beam_width is None and lm is not None:
        raise ValueError("the greedy path takes no language model")
    if beam_width is None and bias is not None:
        raise ValueError("the greedy path takes no phrase bias")
    if confidence and (beam_width is None or nbest < 2):
        raise ValueError("confidence=True needs a beam search with nbest >= 2: a posterior is taken over a list")
    if confidence and delimiter_id is None:
        raise ValueError("confidence without a tokenizer: pass delimiter_id")
    found = pause_cuts(recs, blank=blank, delimiter_id=delimiter_id, margin=pause_margin, min_pause=min_pause)
    bounds, pieces = [], []
    for l, f in zip(recs, found):
        T = int(l.shape[0])
        b = [0] + choose_cuts(f.cuts, f.pauses, T, min_frames, max_frames) + [T]
        bounds.append(b)
        pieces.extend(torch.split(l, [y - x for x, y in zip(b, b[1:])], dim=0))
    if beam_width is None:
        hyps = [[Hypothesis(_collapse(p.argmax(dim=1).cpu().numpy(), blank), float("nan"), float("nan"))] for p in pieces]
    else:
        hyps = beam_search(pieces, beam_width=beam_width, nbest=nbest, blank=blank, lm=lm, bias=bias)
    if rescore or confidence:
        hyps = rescore_lists(pieces, hyps, blank=blank)
    if confidence:
        scored = score_transcripts(pieces, hyps, tokenizer, blank, delimiter_id, seconds_per_frame, posterior_scale, vocab)
        out, k = [], 0
        for b in bounds:
            segments, ids, all_words, all_conf, score, total, logc, nw = [], [], [], [], 0.0, 0.0, 0.0, 0
            for x, y in zip(b, b[1:]):
                st = scored[k]
                k += 1
                start = x * seconds_per_frame
                segments.append(Segment(start, y * seconds_per_frame, st))
                if st.hypotheses:
                    ids.extend(st.hypotheses[0].ids)
                    score += st.hypotheses[0].score
                    total += st.hypotheses[0].total
                all_words.extend(s._replace(start_s=s.start_s + start, end_s=s.end_s + start) for s in st.words)
                all_conf.extend(st.word_confidence)
                if st.words:
                    logc += len(st.words) * math.log(st.confidence)
                    nw += len(st.words)
            text = tokenizer.decode(ids, skip_special_tokens=True, group_tokens=False) if tokenizer is not None else None
            out.append(ScoredLongTranscript(text, tuple(ids), score, total, all_words, segments,
                                            math.exp(logc / nw) if nw else float("nan"), all_conf))
        return out[0] if single else out
    words = [None] * len(pieces)
    if timestamps:
        words = [[] for _ in pieces]
        have = [i for i, h in enumerate(hyps) if h and h[0].ids]
        if have:
            alignments = forced_align([pieces[i] for i in have], [list(hyps[i][0].ids) for i in have], blank=blank)
            for i, a in zip(have, alignments):
                words[i] = word_spans(token_spans(a), delimiter_id, seconds_per_frame, vocab)
    out, k = [], 0
    for b in bounds:
        segments, ids, all_words, score, total = [], [], [] if timestamps else None, 0.0, 0.0
        for x, y in zip(b, b[1:]):
            h, w = hyps[k], words[k]
            k += 1
            texts = [e.text(tokenizer) for e in h] if tokenizer is not None else [None] * len(h)
            start = x * seconds_per_frame
            segments.append(Segment(start, y * seconds_per_frame, Transcript(texts[0] if texts else "", h, texts, w)))
            if h:
                ids.extend(h[0].ids)
                score += h[0].score
                total += h[0].total
            if timestamps:
                all_words.extend(s._replace(start_s=s.start_s + start, end_s=s.end_s + start) for s in w)
        text = tokenizer.decode(ids, skip_special_tokens=True, group_tokens=False) if tokenizer is not None else None
        out.append(LongTranscript(text, tuple(ids), score, total, all_words, segments))
    return out[0] if single else out
