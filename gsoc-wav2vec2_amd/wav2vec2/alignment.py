"""CTC forced alignment on the GPU (w2v2_ctc_align, csrc/align.hip; whole recordings: w2v2_ctc_align_long,
csrc/align_long.hip).

``forced_align`` finds, per utterance, the single best frame-level CTC path (Viterbi) that spells a given label sequence;
``forced_align_long`` is the same path without the limit of 8191 labels, for whole recordings and their texts;
``token_spans`` and ``word_spans`` turn a path into per-token frame spans and per-word time spans; ``split_at_pauses`` cuts an
aligned recording into utterance-sized pieces; ``score_segments`` gives each piece the exact likelihood of its text.  The path and its per-frame log-probabilities are computed by HIP kernels; the
span helpers are host code over the per-frame arrays.

The star: a transcript that does not spell everything that is spoken may hold a wildcard label, the star, wherever
speech is missing from it.  Its id is the vocabulary size V = ``logits.shape[-1]`` (``star_id``), as if the logits had one more
column; it absorbs whatever is spoken there -- at least one frame -- at the cost of the frame's best token plus ``star_score``
(<= 0, nats per frame).  ``forced_align`` and ``forced_align_long`` accept it when ``star_score`` is given; ``token_spans`` yields a
``TokenSpan(token=V, ...)`` for it, ``word_spans(..., star_id=V)`` makes it a word of its own, and ``split_at_pauses(...,
star_text=...)`` cuts there.  With a star an alignment's ``score`` is the score of a path, not the log-probability of a label string.
"""

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _native as N


@dataclass
class Alignment:
    """One utterance's best path.  ``token`` (T,) int32: the path's token per frame (the blank or a label);
    ``label_index`` (T,) int32: k where the frame sits on label k, -1 on a blank; ``frame_logp`` (T,) fp32:
    log_softmax(logits[t])[token[t]]; ``score``: log-probability of the whole path (fp64).  Device tensors
    as returned by ``forced_align``."""
    token: object
    label_index: object
    frame_logp: object
    score: float


class TokenSpan(NamedTuple):
    token: int
    start: int      # first frame
    end: int        # one past the last frame
    score: float    # mean of exp(frame_logp) over the span


class WordSpan(NamedTuple):
    text: object    # the word's characters (or its token ids when no vocabulary is given)
    start_s: float
    end_s: float
    score: float    # mean of exp(frame_logp) over the frames of the word's tokens


class AlignedSegment(NamedTuple):
    text: object    # the words' texts joined by spaces (or the tuple of the words' id tuples when they carry ids)
    start_s: float  # the first word's start
    end_s: float    # the last word's end
    score: float    # mean of the words' scores
    words: list     # the piece's WordSpans


DEFAULT_LONG_WORKSPACE = 32 << 30      # w2v2_ctc_align_long's cap when max_workspace_bytes is 0
DEFAULT_STAR_SCORE = -0.5              # a convention, not a tuned value: any penalty that breaks the tie with a
                                       # correct label recovered all 200 planted cases of tests/test_align_star_cpu.py; 0.0 did not


def star_id(logits):
    """The star's label id for these logits (a tensor, an array, or a list of them): the vocabulary size ``shape[-1]``."""
    return int((logits if hasattr(logits, "shape") else logits[0]).shape[-1])


def _check_star_score(star_score):
    s = float(star_score)
    if not s <= 0.0:
        raise ValueError(f"star_score {star_score}: a log-domain penalty per frame, <= 0 and not NaN")
    return s


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def star_transcript(transcript, V, tokenizer=None, star=None, free_ends=False):
    """The label ids of one transcript of ``Wav2Vec2ForCTC.align`` (host code).  Text is encoded with ``tokenizer``; with ``star``
    (say "*") every whitespace-separated word equal to it becomes the star label ``V``, and the word delimiter next to a star is
    dropped -- the star absorbs it: "* HELLO WORLD *" is [V] + tokenizer("HELLO WORLD") + [V].  A sequence of ids is used as it
    is and may hold ``V`` directly.  ``free_ends`` puts a star before the first and after the last label where none stands yet
    (an empty transcript becomes the single star)."""
    if isinstance(transcript, str):
        if tokenizer is None:
            raise ValueError("a text transcript needs the tokenizer that encodes it")
        if star is None:
            ids = list(tokenizer(transcript))
        else:
            ids, run = [], []
            for w in transcript.split() + [star]:
                if w == star:
                    if run:
                        ids.extend(tokenizer(" ".join(run)))
                        run = []
                    ids.append(V)
                else:
                    run.append(w)
            ids.pop()                                    # (the sentinel)
    else:
        ids = [int(x) for x in transcript]
    if free_ends:
        if not ids or ids[0] != V:
            ids.insert(0, V)
        if len(ids) == 1 or ids[-1] != V:
            ids.append(V)
        if ids == [V, V]:
            ids = [V]
    return ids


def _logits_base(logits, frame_lengths):
    """(base tensor (rows, V), row offset and frame count per utterance): no copy when the list is row-contiguous views of one
    storage (what predict_packed returns) or a (B, T, V) tensor; otherwise one concatenation."""
    import torch
    if isinstance(logits, torch.Tensor):
        if logits.dim() != 3:
            raise ValueError(f"`logits` must be a list of (T_i, V) tensors or a (B, T, V) tensor, got shape {tuple(logits.shape)}")
        B, T, V = logits.shape
        lens = [T] * B if frame_lengths is None else [int(n) for n in frame_lengths]
        if len(lens) != B:
            raise ValueError(f"frame_lengths has {len(lens)} entries for a batch of {B}")
        for i, n in enumerate(lens):
            if not 1 <= n <= T:
                raise ValueError(f"utterance {i}: frame length {n} outside [1, {T}]")
        base = logits.detach()
        if base.dtype != torch.float32 or not base.is_cuda or not base.is_contiguous():
            base = base.to(device="cuda", dtype=torch.float32).contiguous()
        return base.reshape(B * T, V), [b * T for b in range(B)], lens
    if frame_lengths is not None:
        raise ValueError("frame_lengths goes with a (B, T, V) tensor; a list of (T_i, V) tensors carries its own lengths")
    parts = list(logits)
    if not parts:
        raise ValueError("`logits` is an empty list")
    for i, p in enumerate(parts):
        if not isinstance(p, torch.Tensor) or p.dim() != 2:
            raise ValueError(f"utterance {i}: logits must be a 2-D (T_i, V) tensor")
        if p.shape[1] != parts[0].shape[1]:
            raise ValueError(f"utterance {i}: vocabulary {p.shape[1]} differs from utterance 0's {parts[0].shape[1]}")
        if p.shape[0] < 1:
            raise ValueError(f"utterance {i} has no frames")
    V = int(parts[0].shape[1])
    lens = [int(p.shape[0]) for p in parts]
    first = parts[0]
    same = all(p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() and p.device == first.device
               and p.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() for p in parts)
    if same:
        lo = min(p.data_ptr() for p in parts)
        offs = [p.data_ptr() - lo for p in parts]
        if all(o % (4 * V) == 0 for o in offs):
            start = min(range(len(parts)), key=lambda i: parts[i].data_ptr())
            rows = max(o // (4 * V) + n for o, n in zip(offs, lens))
            base = parts[start].detach().as_strided((rows, V), (V, 1))
            return base, [o // (4 * V) for o in offs], lens
    base = torch.cat([p.detach().to(device="cuda", dtype=torch.float32) for p in parts]).contiguous()
    return base, list(np.cumsum([0] + lens[:-1]).tolist()), lens


def _check_labels(labels, lens, V, blank, max_labels=N.ALIGN_MAX_LABELS, star=False):
    out = []
    for i, lab in enumerate(labels):
        a = np.asarray(_host(lab) if hasattr(lab, "cpu") else list(lab), dtype=np.int64).reshape(-1)
        if star:
            if a.size and (a.min() < 0 or a.max() > V):
                raise ValueError(f"utterance {i}: labels must lie in [0, {V}] ({V} is the star), got [{a.min()}, {a.max()}]")
            if a.size > 1 and ((a[1:] == V) & (a[:-1] == V)).any():
                raise ValueError(f"utterance {i}: two stars next to each other; collapse them into one")
        elif a.size and (a.min() < 0 or a.max() >= V):
            raise ValueError(f"utterance {i}: labels must lie in [0, {V}), got [{a.min()}, {a.max()}]")
        if a.size and (a == blank).any():
            raise ValueError(f"utterance {i}: label {blank} is the blank")
        if max_labels is not None and a.size > max_labels:
            raise ValueError(f"utterance {i}: {a.size} labels; at most {max_labels} per utterance")
        repeats = int((a[1:] == a[:-1]).sum()) if a.size > 1 else 0
        if lens[i] < a.size + repeats:
            raise ValueError(f"utterance {i}: {lens[i]} frames cannot hold {a.size} labels with {repeats} repeats "
                             f"(a CTC path needs at least {a.size + repeats})")
        out.append(a.astype(np.int32))
    return out


def forced_align(logits, labels, blank=0, frame_lengths=None, star_score=None):
    """Best CTC path of each utterance's labels through its logits; one ``Alignment`` per utterance.

    ``logits``: a list of (T_i, V) tensors -- views of one storage, as ``predict_packed`` returns them, are read in place --
    or a (B, T, V) tensor with ``frame_lengths`` (default: T for every row).  ``labels``: one id sequence per utterance,
    none of them the blank.  Raises ValueError, naming the utterance, for a label outside the vocabulary, a blank label, or
    too few frames for the labels (T_i < U_i + repeated neighbours).

    ``star_score``: None is the call without a star: the label V is a ValueError.  A float <= 0 admits the star, label id V =
    ``star_id(logits)`` (w2v2_ctc_align_star): it may stand anywhere, takes at least one frame and counts as a label in the frame
    check; on its frames ``token`` is V and ``frame_logp`` is max_v log_softmax(logits[t])[v] + star_score.  Two stars next to
    each other and a star_score that is NaN or > 0 raise ValueError.  Utterances without a star get the bits of the call without
    ``star_score``.  ``score`` is then the score of the path, no longer the log-probability of a label string."""
    import torch
    star = star_score is not None
    if star:
        star_score = _check_star_score(star_score)
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    if len(labels) != n:
        raise ValueError(f"{len(labels)} label sequences for {n} utterances")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    labs = _check_labels(labels, lens, V, blank, star=star)
    dev = base.device
    flat = np.concatenate(labs + [np.zeros(1, np.int32)])      # (one spare entry: never an empty buffer)
    label0 = np.cumsum([0] + [a.size for a in labs[:-1]]).astype(np.int64)
    labels_dev = torch.from_numpy(flat).to(dev)
    total = sum(lens)
    token = torch.empty(total, dtype=torch.int32, device=dev)
    label_index = torch.empty(total, dtype=torch.int32, device=dev)
    frame_logp = torch.empty(total, dtype=torch.float32, device=dev)
    score = torch.empty(n, dtype=torch.float64, device=dev)
    row0_h = np.asarray(row0, np.int64)
    frames_h = np.asarray(lens, np.int32)
    nlab_h = np.asarray([a.size for a in labs], np.int32)
    lib = N.load()
    if star:
        N.check(lib.w2v2_ctc_align_star(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(labels_dev), N.ptr(label0),
                                        N.ptr(nlab_h), int(blank), star_score, N.ptr(token), N.ptr(label_index), N.ptr(frame_logp),
                                        N.ptr(score), N.current_stream()), "w2v2_ctc_align_star")
    else:
        N.check(lib.w2v2_ctc_align(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(labels_dev), N.ptr(label0),
                                   N.ptr(nlab_h), int(blank), N.ptr(token), N.ptr(label_index), N.ptr(frame_logp), N.ptr(score),
                                   N.current_stream()), "w2v2_ctc_align")
    scores = score.cpu().numpy()
    return [Alignment(tk, li, fl, float(sc)) for tk, li, fl, sc in
            zip(torch.split(token, lens), torch.split(label_index, lens), torch.split(frame_logp, lens), scores)]


def forced_align_long(logits, labels, blank=0, frame_lengths=None, strip_pairs=None, panel_frames=None, max_workspace_bytes=None,
                      star_score=None):
    """``forced_align`` for whole recordings: the same path, bit for bit, with any number of labels (w2v2_ctc_align_long).

    ``logits``: what ``forced_align`` accepts, read in place where it reads in place (``predict_long``'s list included), or one
    (T, V) tensor with ``labels`` one id sequence: then the result is that recording's ``Alignment`` and not a list.  The same
    ValueErrors as ``forced_align``, without the limit of 8191 labels.  ``strip_pairs`` (a multiple of 64 in [64, 8192]) and
    ``panel_frames`` (a multiple of 8) set the tile of the frames x states plane that one block sweeps; they change speed, never a
    bit of the result; None is the measured default.  The workspace holds 2 bits per frame and state, about T (U + 1) / 2 bytes
    per recording (5 GB for an hour of speech); a call that needs more than ``max_workspace_bytes`` (None: 32 GiB) raises
    MemoryError, with the shapes and the bytes, before anything is allocated.  ``star_score``: as ``forced_align``
    (w2v2_ctc_align_long_star; the workspace holds one more fp64 per frame)."""
    import torch
    star = star_score is not None
    if star:
        star_score = _check_star_score(star_score)
    single = isinstance(logits, torch.Tensor) and logits.dim() == 2
    if single:
        logits, labels = [logits], [labels]
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    if len(labels) != n:
        raise ValueError(f"{len(labels)} label sequences for {n} recordings")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    labs = _check_labels(labels, lens, V, blank, max_labels=None, star=star)
    sp = 0 if strip_pairs is None else int(strip_pairs)
    pf = 0 if panel_frames is None else int(panel_frames)
    if sp and (sp % 64 or not 64 <= sp <= 8192):
        raise ValueError(f"strip_pairs {sp}: a multiple of 64 in [64, 8192]")
    if pf and (pf % 8 or pf < 8):
        raise ValueError(f"panel_frames {pf}: a multiple of 8, at least 8")
    cap = DEFAULT_LONG_WORKSPACE if max_workspace_bytes is None else int(max_workspace_bytes)
    if cap < 1:
        raise ValueError(f"max_workspace_bytes {cap} must be positive")
    frames_h = np.asarray(lens, np.int32)
    nlab_h = np.asarray([a.size for a in labs], np.int32)
    lib = N.load()
    workspace = lib.w2v2_ctc_align_long_star_workspace if star else lib.w2v2_ctc_align_long_workspace
    need = int(workspace(n, N.ptr(frames_h), N.ptr(nlab_h), sp, pf))
    if need < 0:
        N.check(need, "w2v2_ctc_align_long_workspace")
    if need > cap:
        shapes = ", ".join(f"{t} frames x {u} labels" for t, u in zip(lens, nlab_h.tolist()))
        raise MemoryError(f"forced_align_long: {shapes} need {need} bytes of workspace; max_workspace_bytes is {cap}")
    dev = base.device
    flat = np.concatenate(labs + [np.zeros(1, np.int32)])      # (one spare entry: never an empty buffer)
    label0 = np.cumsum([0] + [a.size for a in labs[:-1]]).astype(np.int64)
    labels_dev = torch.from_numpy(flat).to(dev)
    total = sum(lens)
    token = torch.empty(total, dtype=torch.int32, device=dev)
    label_index = torch.empty(total, dtype=torch.int32, device=dev)
    frame_logp = torch.empty(total, dtype=torch.float32, device=dev)
    score = torch.empty(n, dtype=torch.float64, device=dev)
    row0_h = np.asarray(row0, np.int64)
    if star:
        N.check(lib.w2v2_ctc_align_long_star(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(labels_dev), N.ptr(label0),
                                             N.ptr(nlab_h), int(blank), star_score, N.ptr(token), N.ptr(label_index),
                                             N.ptr(frame_logp), N.ptr(score), sp, pf, cap, N.current_stream()),
                "w2v2_ctc_align_long_star")
    else:
        N.check(lib.w2v2_ctc_align_long(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(labels_dev), N.ptr(label0),
                                        N.ptr(nlab_h), int(blank), N.ptr(token), N.ptr(label_index), N.ptr(frame_logp), N.ptr(score),
                                        sp, pf, cap, N.current_stream()), "w2v2_ctc_align_long")
    scores = score.cpu().numpy()
    out = [Alignment(tk, li, fl, float(sc)) for tk, li, fl, sc in
           zip(torch.split(token, lens), torch.split(label_index, lens), torch.split(frame_logp, lens), scores)]
    return out[0] if single else out


def token_spans(alignment):
    """The U labels of an alignment as ``TokenSpan(token, start, end, score)`` in frames, ``end`` exclusive, in label
    order; ``score`` is the mean of exp(frame_logp) over the span.  An alignment without a path (-1 rows) has none."""
    li = _host(alignment.label_index).astype(np.int64)
    tok = _host(alignment.token)
    p = np.exp(_host(alignment.frame_logp).astype(np.float64))
    if li.size == 0:
        return []
    cut = np.flatnonzero(li[1:] != li[:-1]) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [li.size]))
    return [TokenSpan(int(tok[s]), int(s), int(e), float(p[s:e].mean())) for s, e in zip(starts, ends) if li[s] >= 0]


def word_spans(spans, delimiter_id, seconds_per_frame, vocab=None, star_id=None, star_text="*"):
    """Words of a token-span list: the maximal runs of spans whose token is not ``delimiter_id`` (leading, trailing and
    doubled delimiters make no empty word).  ``WordSpan(text, start_s, end_s, score)``: the first span's start and the last
    span's end times ``seconds_per_frame``; ``score`` the mean of exp(frame_logp) over the frames of the word's spans;
    ``text`` the characters ``vocab`` gives the ids (a mapping or a sequence id -> string), or the tuple of ids.  A span whose
    token is ``star_id`` (when given) closes the current word and is a ``WordSpan(star_text, start_s, end_s, score)`` of its
    own: where the unknown speech lies."""
    words, cur = [], []

    def close():
        if cur:
            nf = sum(s.end - s.start for s in cur)
            score = sum(s.score * (s.end - s.start) for s in cur) / nf
            ids = tuple(s.token for s in cur)
            text = "".join(vocab[i] for i in ids) if vocab is not None else ids
            words.append(WordSpan(text, cur[0].start * seconds_per_frame, cur[-1].end * seconds_per_frame, score))
            cur.clear()

    for s in spans:
        if star_id is not None and s.token == star_id:
            close()
            words.append(WordSpan(star_text, s.start * seconds_per_frame, s.end * seconds_per_frame, s.score))
        elif s.token == delimiter_id:
            close()
        else:
            cur.append(s)
    close()
    return words


def split_at_pauses(words, min_pause_s=0.3, max_len_s=20.0, star_text=None):
    """Utterance-sized pieces of an aligned recording (host code): ``words`` is a recording's WordSpan list in time order.
    A cut falls between words i and i + 1 wherever ``start_s[i + 1] - end_s[i] >= min_pause_s``.  A piece longer than
    ``max_len_s`` (last end minus first start) is cut again at its largest internal gap, the earliest among equal gaps, until
    every piece fits or is a single word.  Returns ``AlignedSegment(text, start_s, end_s, score, words)`` in time order: ``text``
    the words joined by spaces (the tuple of the words' id tuples when they carry ids), ``score`` the mean of the words' scores.
    ``star_text``: when given, a word whose text equals it (the star words of ``word_spans(..., star_id=...)``) always ends a piece
    and belongs to none: the pieces on its two sides are cut as if each were a recording of its own."""
    words = list(words)
    if star_text is not None:
        out, run = [], []
        for w in words + [None]:
            if w is None or (isinstance(w.text, str) and w.text == star_text):
                out.extend(split_at_pauses(run, min_pause_s, max_len_s))
                run = []
            else:
                run.append(w)
        return out
    if not words:
        return []
    pieces, first = [], 0
    for i in range(len(words) - 1):
        if words[i + 1].start_s - words[i].end_s >= min_pause_s:
            pieces.append((first, i + 1))
            first = i + 1
    pieces.append((first, len(words)))
    out, todo = [], pieces[::-1]
    while todo:
        a, b = todo.pop()
        if b - a > 1 and words[b - 1].end_s - words[a].start_s > max_len_s:
            gaps = [words[i + 1].start_s - words[i].end_s for i in range(a, b - 1)]
            cut = a + 1 + max(range(len(gaps)), key=lambda i: (gaps[i], -i))
            todo.append((cut, b))
            todo.append((a, cut))
            continue
        ws = words[a:b]
        texts = [w.text for w in ws]
        text = " ".join(texts) if all(isinstance(t, str) for t in texts) else tuple(texts)
        out.append(AlignedSegment(text, ws[0].start_s, ws[-1].end_s, sum(w.score for w in ws) / len(ws), ws))
    return out


def score_segments(logits, segments, tokenizer, seconds_per_frame, blank=0):
    """The likelihood filter for ``align_long`` followed by ``split_at_pauses``: the exact CTC log-probability PER FRAME of each
    ``AlignedSegment``'s text over its own frame range of the recording's (T, V) ``logits``, in ONE ``wav2vec2.decoding.ctc_score``
    call on views of the logits (nothing is copied).  A segment's frames are ``[round(start_s / seconds_per_frame),
    round(end_s / seconds_per_frame))``, clipped to the recording and never empty; its text is encoded with ``tokenizer`` (words
    that carry ids are joined with the tokenizer's word delimiter).  Returns one float per segment; a piece whose text does not
    belong to its audio stands out by a value far below its neighbours' (``-inf`` where the frames cannot hold the text)."""
    from .decoding import ctc_score
    from .processor import WORD_DELIMITER
    segments = list(segments)
    if not segments:
        return []
    if getattr(logits, "dim", lambda: 0)() != 2:
        raise ValueError("`logits` must be one recording's (T, V) tensor")
    T = int(logits.shape[0])
    views, ids = [], []
    for i, sg in enumerate(segments):
        f0 = min(max(int(round(sg.start_s / seconds_per_frame)), 0), T - 1)
        f1 = min(max(int(round(sg.end_s / seconds_per_frame)), f0 + 1), T)
        views.append(logits[f0:f1])
        if isinstance(sg.text, str):
            ids.append(list(tokenizer(sg.text)))
        else:
            delim = tokenizer.get_vocab()[WORD_DELIMITER]
            seq = []
            for k, w in enumerate(sg.text):
                seq.extend(([delim] if k else []) + [int(c) for c in w])
            ids.append(seq)
    logp = ctc_score(views, ids, blank=blank)
    return [float(v) / int(p.shape[0]) for v, p in zip(logp, views)]
