"""CTC phrase search on the GPU (w2v2_ctc_spot, csrc/spot.hip): where in recordings phrases are spoken.

``find_phrases`` searches logits for label sequences: a Viterbi recursion with a free begin and a free end whose score is the
log-ratio of the phrase's best path to the frame-wise best path over the same frames (0 where the phrase IS the greedy path,
more negative the less it fits).  It finds occurrences the 1-best transcript spells slightly wrong, and unlike a forced
alignment it does not make the phrase cover the recording.  ``phrase_labels`` encodes a phrase; the model's ``search`` /
``search_long`` run it over ``predict_packed`` / ``predict_long`` and report seconds.  The recursion and the hit pass are a HIP
kernel (exact definition in include/w2v2.h); this module is pairing, thresholds, the optional chunk plan and the conversion of the
kernel's arrays.
"""

from typing import NamedTuple

import numpy as np

from . import _native as N
from .alignment import _host, _logits_base


class PhraseHit(NamedTuple):
    phrase: int     # index of the phrase in `phrases`
    begin: int      # first frame (a frame of the phrase's first label)
    end: int        # last frame, inclusive (a frame of its last label)
    score: float    # ln P(best path of the phrase over [begin, end]) - ln P(greedy path over them): <= 0
    logp: object    # exact=True: the phrase's exact CTC log-probability over [begin, end] per frame; else None


class PhraseSpan(NamedTuple):
    text: object    # the phrase as it was given (text, or the tuple of its ids)
    start_s: float  # begin * seconds_per_frame
    end_s: float    # (end + 1) * seconds_per_frame
    score: float
    logp: object


def phrase_labels(text, tokenizer, whole_words=True):
    """The label ids of a phrase: ``tokenizer(text)`` (a Wav2Vec2Processor(is_tokenizer=True)) with the ends stripped of word
    delimiters; ``whole_words=True`` then puts ONE word delimiter on both ends, so that "CAT" does not match inside
    "CATALOGUE" (pass ``delimiter_id`` to ``find_phrases`` so that a word at a recording's edge still matches)."""
    from .processor import WORD_DELIMITER
    delim = tokenizer.get_vocab()[WORD_DELIMITER]
    ids = [int(i) for i in tokenizer(text)]
    while ids and ids[0] == delim:
        ids.pop(0)
    while ids and ids[-1] == delim:
        ids.pop()
    if whole_words and ids:
        ids = [delim] + ids + [delim]
    return ids


def chunk_plan(T, chunk_frames, overlap_frames):
    """[(start, frames)] of the overlapping pieces of a recording of T frames: piece k starts at k (chunk - overlap); the last
    piece is the first that reaches the recording's end."""
    out, start = [], 0
    while True:
        out.append((start, min(chunk_frames, T - start)))
        if start + chunk_frames >= T:
            return out
        start += chunk_frames - overlap_frames


def _overlap_pass(cands):
    """the kernel's hit rule over (score, begin, end) candidates in their order"""
    out, cur = [], None
    for h in cands:
        if cur is not None and h[1] <= cur[2]:
            if h[0] > cur[0]:
                cur = h
        else:
            if cur is not None:
                out.append(cur)
            cur = h
    if cur is not None:
        out.append(cur)
    return out


def _check_phrases(phrases, V, blank):
    labs = []
    for j, lab in enumerate(phrases):
        a = np.asarray(_host(lab) if hasattr(lab, "cpu") else list(lab), dtype=np.int64).reshape(-1)
        if not a.size:
            raise ValueError(f"phrase {j} is empty")
        if a.min() < 0 or a.max() >= V:
            raise ValueError(f"phrase {j}: labels must lie in [0, {V}), got [{a.min()}, {a.max()}]")
        if (a == blank).any():
            raise ValueError(f"phrase {j}: label {blank} is the blank")
        if a.size > N.SPOT_MAX_LABELS:
            raise ValueError(f"phrase {j}: {a.size} labels; at most {N.SPOT_MAX_LABELS} per phrase")
        labs.append(a.astype(np.int32))
    return labs


def _spot(base, row0, frames, utt, labs, blank, delim, thr, max_hits, trace):
    """ONE w2v2_ctc_spot call: pair j = rows [row0[utt[j]], + frames[utt[j]]) of `base` against labs[j].  Returns host arrays
    (score (m, max_hits) f64, begin, end (m, max_hits) i32, count (m) i32, traces: per pair (z, c) or None)."""
    import torch
    dev = base.device
    V, n, m = int(base.shape[1]), len(frames), len(labs)
    flat = np.concatenate(labs + [np.zeros(1, np.int32)])
    label0 = np.cumsum([0] + [a.size for a in labs[:-1]]).astype(np.int64)
    nlab = np.asarray([a.size for a in labs], np.int32)
    labels_dev = torch.from_numpy(flat).to(dev)
    score = torch.empty((m, max_hits), dtype=torch.float64, device=dev)
    begin = torch.empty((m, max_hits), dtype=torch.int32, device=dev)
    end = torch.empty((m, max_hits), dtype=torch.int32, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    row0_h, frames_h = np.asarray(row0, np.int64), np.asarray(frames, np.int32)
    utt_h, thr_h = np.asarray(utt, np.int32), np.asarray(thr, np.float64)
    tz = tc = trace0 = None
    if trace:
        lens = frames_h[utt_h].astype(np.int64)
        trace0 = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        tz = torch.empty(int(lens.sum()), dtype=torch.float64, device=dev)
        tc = torch.empty(int(lens.sum()), dtype=torch.int32, device=dev)
    N.check(N.load().w2v2_ctc_spot(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), m, N.ptr(utt_h), N.ptr(labels_dev), N.ptr(label0),
                                   N.ptr(nlab), blank, delim, N.ptr(thr_h), max_hits, N.ptr(score), N.ptr(begin), N.ptr(end),
                                   N.ptr(count), N.ptr(tz), N.ptr(tc), N.ptr(trace0), N.current_stream()), "w2v2_ctc_spot")
    traces = [None] * m
    if trace:
        tz_h, tc_h = tz.cpu().numpy(), tc.cpu().numpy()
        traces = [(tz_h[o:o + l], tc_h[o:o + l]) for o, l in zip(trace0, lens)]
    return score.cpu().numpy(), begin.cpu().numpy(), end.cpu().numpy(), count.cpu().numpy(), traces


def find_phrases(logits, phrases, blank=0, delimiter_id=None, margin_per_label=1.0, min_score=None, max_hits=64, utterance=None,
                 frame_lengths=None, trace=False, exact=False, chunk_frames=None, overlap_frames=None):
    """Where each phrase is spoken in each recording: one list of ``PhraseHit(phrase, begin, end, score, logp)`` per pair, the
    hits in time order and pairwise non-overlapping.

    ``logits``: what ``forced_align`` accepts, read in place.  ``phrases``: one id sequence per phrase (1 to 256 ids, none the
    blank; see ``phrase_labels``).  By default every phrase is searched in every recording and pair ``i * len(phrases) + p`` is
    (recording i, phrase p); ``utterance=`` gives explicit pairs instead, as in ``ctc_score``: pair j is (recording utterance[j],
    phrase j).  A hit's ``score`` is the log-ratio of the phrase's best path over ``[begin, end]`` to the greedy path over the same
    frames; a frame ends a candidate hit when its score reaches the threshold, and of overlapping candidates the best is kept.
    The threshold is ``min_score`` (one number, or one per phrase) or, by default, ``-margin_per_label`` times the phrase's label
    count -- a convention, not a tuned value: raise it for fewer false alarms.  ``delimiter_id``: the word delimiter's id; a
    phrase that begins (ends) with it then also matches where the recording begins (ends) with the word itself, without the
    delimiter.  At most ``max_hits`` hits are kept per pair (and per piece), the earliest.  A recording with a NaN or +inf logit
    (or a frame of -inf only) gives ``None`` in the place of its pairs' lists.

    ``trace=True`` returns ``(hits, traces)``, ``traces[j] = (z, c)``: the phrase's end score and begin at every frame (float64,
    int32 numpy).  ``exact=True`` fills ``logp`` with the exact CTC log-probability per frame of the phrase over ``[begin, end]``:
    ONE ``ctc_score`` call on views of the logits for all hits.

    ``chunk_frames=C, overlap_frames=O`` (0 < O < C) searches a recording as overlapping views -- piece k starts at k (C - O),
    nothing is copied -- so that ONE long recording is spread over many waves.  A piece behind the first keeps the hits whose
    local end is >= O; all kept hits of a pair are sorted by (end, begin) and passed once more through the overlap rule.  This is
    approximate only for hits longer than O frames and for hits that compete with a path begun before their piece; the edge rule
    of ``delimiter_id`` is off (a piece's edges are not the recording's), and ``trace`` is not available.

    Raises ValueError, naming the phrase, for an empty phrase, a label outside the vocabulary, a blank label or more than 256
    labels, before anything is launched."""
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    blank, max_hits = int(blank), int(max_hits)
    if V < 2:
        raise ValueError(f"vocabulary {V}; the blank and at least one label")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    delim = -1 if delimiter_id is None else int(delimiter_id)
    if delim != -1 and (not 0 <= delim < V or delim == blank):
        raise ValueError(f"delimiter_id {delim} must be a label of [0, {V}) other than the blank")
    if max_hits < 1:
        raise ValueError(f"max_hits {max_hits}; at least one")
    labs = _check_phrases(list(phrases), V, blank)
    if not labs:
        raise ValueError("no phrase to search for")
    # thresholds per phrase
    if min_score is None:
        thr_p = np.asarray([-float(margin_per_label) * a.size for a in labs], np.float64)
    else:
        thr_p = np.asarray(min_score, np.float64)
        thr_p = np.full(len(labs), float(thr_p)) if thr_p.ndim == 0 else thr_p.reshape(-1)
        if thr_p.size != len(labs):
            raise ValueError(f"{thr_p.size} entries of `min_score` for {len(labs)} phrases")
    if np.isnan(thr_p).any():
        raise ValueError("`min_score` / `margin_per_label` gives a NaN threshold")
    # pairs (recording, phrase)
    if utterance is None:
        pair_utt = [i for i in range(n) for _ in labs]
        pair_phrase = [p for _ in range(n) for p in range(len(labs))]
    else:
        u = np.asarray(list(utterance), dtype=np.int64).reshape(-1)
        if u.size != len(labs):
            raise ValueError(f"{len(labs)} phrases with {u.size} entries of `utterance`")
        if u.min() < 0 or u.max() >= n:
            raise ValueError(f"`utterance` must lie in [0, {n}), got [{u.min()}, {u.max()}]")
        pair_utt, pair_phrase = [int(x) for x in u], list(range(len(labs)))
    m = len(pair_utt)
    chunked = chunk_frames is not None or overlap_frames is not None
    if chunked:
        if chunk_frames is None or overlap_frames is None:
            raise ValueError("chunk_frames and overlap_frames go together")
        C, O = int(chunk_frames), int(overlap_frames)
        if not 0 < O < C:
            raise ValueError(f"need 0 < overlap_frames < chunk_frames, got {O}, {C}")
        if trace:
            raise ValueError("trace=True is not available with chunk_frames: a piece's trace is not the recording's")
        # every piece of every recording is a recording of the call; a pair becomes one pair per piece of its recording
        piece_row0, piece_len, pieces_of = [], [], []
        for i in range(n):
            plan = chunk_plan(lens[i], C, O)
            pieces_of.append((len(piece_row0), plan))
            piece_row0 += [row0[i] + s for s, _ in plan]
            piece_len += [f for _, f in plan]
        k_utt, k_lab, k_thr, owner = [], [], [], []
        for j in range(m):
            first, plan = pieces_of[pair_utt[j]]
            for k in range(len(plan)):
                k_utt.append(first + k)
                k_lab.append(labs[pair_phrase[j]])
                k_thr.append(thr_p[pair_phrase[j]])
                owner.append((j, k, plan[k][0]))
        score, begin, end, count, _ = _spot(base, piece_row0, piece_len, k_utt, k_lab, blank, -1, k_thr, max_hits, False)
        kept, bad = [[] for _ in range(m)], [False] * m
        for q, (j, k, start) in enumerate(owner):
            if count[q] < 0:
                bad[j] = True
                continue
            for i in range(min(int(count[q]), max_hits)):
                if k == 0 or end[q, i] >= O:
                    kept[j].append((float(score[q, i]), int(begin[q, i]) + start, int(end[q, i]) + start))
        found = [None if bad[j] else _overlap_pass(sorted(kept[j], key=lambda h: (h[2], h[1])))[:max_hits] for j in range(m)]
        traces = None
    else:
        score, begin, end, count, traces = _spot(base, row0, lens, pair_utt, [labs[p] for p in pair_phrase], blank, delim,
                                                 [thr_p[p] for p in pair_phrase], max_hits, bool(trace))
        found = [None if count[j] < 0 else [(float(score[j, i]), int(begin[j, i]), int(end[j, i]))
                                            for i in range(min(int(count[j]), max_hits))] for j in range(m)]
    logps = {}
    if exact:
        from .decoding import ctc_score
        where = [(j, i) for j in range(m) if found[j] for i in range(len(found[j]))]
        if where:
            views = [base[row0[pair_utt[j]] + found[j][i][1]:row0[pair_utt[j]] + found[j][i][2] + 1] for j, i in where]
            lp = ctc_score(views, [labs[pair_phrase[j]] for j, _ in where], blank=blank)
            logps = {w: float(v) / int(x.shape[0]) for w, v, x in zip(where, lp, views)}
    hits = [None if found[j] is None else [PhraseHit(pair_phrase[j], bg, en, s, logps.get((j, i))) for i, (s, bg, en) in enumerate(found[j])]
            for j in range(m)]
    return (hits, traces) if trace else hits


def phrase_spans(hits, texts, seconds_per_frame):
    """One recording's hits of all phrases (lists of ``PhraseHit``, ``None`` for a bad pair) as ``PhraseSpan``s sorted by start:
    ``start_s = begin * seconds_per_frame``, ``end_s = (end + 1) * seconds_per_frame`` -- the alignment module's clock."""
    out = []
    for hs in hits:
        for h in hs or []:
            out.append(PhraseSpan(texts[h.phrase], h.begin * seconds_per_frame, (h.end + 1) * seconds_per_frame, h.score, h.logp))
    return sorted(out, key=lambda s: (s.start_s, s.end_s))


def search_logits(logits, phrases, tokenizer, blank, seconds_per_frame, whole_words=True, **options):
    """What the model's ``search`` / ``search_long`` do behind the forward: encode the phrases (text through ``phrase_labels``,
    id sequences as they are), ``find_phrases`` with every phrase in every recording and the tokenizer's word delimiter, and
    per recording the ``PhraseSpan``s of all phrases sorted by start."""
    from .processor import WORD_DELIMITER
    phrases = [phrases] if isinstance(phrases, str) else list(phrases)
    if any(isinstance(p, str) for p in phrases) and tokenizer is None:
        raise ValueError("a phrase is text: pass the tokenizer that encodes it")
    labs = [phrase_labels(p, tokenizer, whole_words) if isinstance(p, str) else [int(x) for x in p] for p in phrases]
    texts = [p if isinstance(p, str) else tuple(l) for p, l in zip(phrases, labs)]
    if "delimiter_id" not in options and tokenizer is not None:
        options["delimiter_id"] = tokenizer.get_vocab()[WORD_DELIMITER]
    if "utterance" in options or "trace" in options:
        raise ValueError("search pairs every phrase with every recording and returns spans: use find_phrases for `utterance` and `trace`")
    hits = find_phrases(logits, labs, blank=blank, **options)
    k = len(labs)
    return [phrase_spans(hits[i * k:(i + 1) * k], texts, seconds_per_frame) for i in range(len(hits) // k)]
