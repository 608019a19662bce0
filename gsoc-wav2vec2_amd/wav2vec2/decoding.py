"""CTC prefix beam search on the GPU (w2v2_ctc_beam_search, csrc/beam.hip).

``beam_search`` returns, per utterance, the n most probable transcripts with their log-probabilities; ``CharNgramLM`` is an
optional character n-gram language model, a dense table of log-probabilities that the kernel reads on the device.  The search
is a HIP kernel; the table is counted and smoothed on the host (it is built once) and uploaded on first use.
"""

from typing import NamedTuple

import numpy as np

from . import _native as N


class Hypothesis(NamedTuple):
    ids: tuple      # the transcript's label ids (no blanks)
    score: float    # CTC log-probability of the transcript over the frame paths the beam kept (a lower bound of the exact value)
    total: float    # score + language-model score: what the hypotheses are ranked by

    def text(self, tokenizer):
        """The transcript as text through a ``Wav2Vec2Processor(is_tokenizer=True)``: ids -> characters, ``|`` -> space."""
        return tokenizer.decode(self.ids, skip_special_tokens=True, group_tokens=False)


class CharNgramLM:
    """Character n-gram model as a dense table: ``table[ctx, c]`` = log P(c | the ``order - 1`` labels before it), ``ctx`` those
    labels read as digits base V, oldest first, missing history filled with the blank id (the blank never occurs in a
    transcript, so it serves as begin-of-sentence).  A new label ``c`` adds ``alpha * table[ctx, c] + beta`` to a hypothesis'
    language-model score.  ``table``: (V ** (order - 1), V), finite; a 4-gram over 32 letters is 4 MiB."""

    MAX_ORDER = 4

    def __init__(self, table, order, alpha=1.0, beta=0.0):
        order = int(order)
        if not 1 <= order <= self.MAX_ORDER:
            raise ValueError(f"language model order {order}; 1 to {self.MAX_ORDER}")
        t = np.asarray(table, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] < 1 or t.shape[0] != t.shape[1] ** (order - 1):
            raise ValueError(f"an order-{order} table has shape (V ** {order - 1}, V), got {tuple(t.shape)}")
        if t.shape[1] > N.BEAM_MAX_VOCAB:
            raise ValueError(f"vocabulary {t.shape[1]}; at most {N.BEAM_MAX_VOCAB}")
        if not np.isfinite(t).all():
            raise ValueError("the language model table must be finite (use add-k smoothing or a floor, not log 0)")
        if not (np.isfinite(alpha) and np.isfinite(beta)):
            raise ValueError("alpha and beta must be finite")
        self.table = np.ascontiguousarray(t)
        self.order = order
        self.alpha = float(alpha)
        self.beta = float(beta)
        self._dev = {}

    @property
    def vocab_size(self):
        return int(self.table.shape[1])

    def device_table(self, device):
        """the table on ``device`` (uploaded on first use, then kept)"""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.table).to(device)
        return self._dev[key]

    @classmethod
    def from_ids(cls, sequences, V, blank, order, add_k=1.0, alpha=1.0, beta=0.0):
        """Count the n-grams of id sequences (none of the ids the blank) and smooth: P(c | ctx) = (count(ctx, c) + add_k) /
        (count(ctx) + add_k (V - 1)) over the V - 1 labels; the blank's column, which the search never reads, gets the
        probability add_k / (count(ctx) + add_k (V - 1)) of an unseen label and is left out of the normalisation, so that
        each row sums to 1 over the labels."""
        V, blank, order = int(V), int(blank), int(order)
        if not 1 <= order <= cls.MAX_ORDER:
            raise ValueError(f"language model order {order}; 1 to {cls.MAX_ORDER}")
        if not 0 <= blank < V:
            raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
        if not add_k > 0:
            raise ValueError("add_k must be positive (a zero count would give log 0)")
        counts = np.zeros((V ** (order - 1), V), np.float64)
        mod = V ** (order - 1)
        start = 0
        for _ in range(order - 1):
            start = start * V + blank
        for s, seq in enumerate(sequences):
            ctx = start
            for c in seq:
                c = int(c)
                if not 0 <= c < V or c == blank:
                    raise ValueError(f"sequence {s}: id {c} is the blank or outside [0, {V})")
                counts[ctx, c] += 1.0
                ctx = (ctx * V + c) % mod
        denom = counts.sum(axis=1, keepdims=True) + add_k * (V - 1)
        return cls(np.log((counts + add_k) / denom).astype(np.float32), order, alpha, beta)

    @classmethod
    def from_text(cls, texts, tokenizer, order, add_k=1.0, alpha=1.0, beta=0.0):
        """``from_ids`` on ``tokenizer(text)`` of every text, with the tokenizer's vocabulary size and blank (``<pad>``)."""
        vocab = tokenizer.get_vocab()
        from .processor import PAD_TOKEN
        return cls.from_ids([tokenizer(t) for t in texts], max(vocab.values()) + 1, vocab[PAD_TOKEN], order, add_k, alpha, beta)


def _check_args(V, beam_width, nbest, blank, lm):
    if not 1 <= V <= N.BEAM_MAX_VOCAB:
        raise ValueError(f"vocabulary {V}; the beam search takes at most {N.BEAM_MAX_VOCAB}")
    if not 1 <= beam_width <= N.BEAM_MAX_WIDTH:
        raise ValueError(f"beam_width {beam_width}; 1 to {N.BEAM_MAX_WIDTH}")
    if not 1 <= nbest <= beam_width:
        raise ValueError(f"nbest {nbest} outside [1, beam_width {beam_width}]")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    if lm is not None:
        if not isinstance(lm, CharNgramLM):
            raise ValueError("`lm` must be a CharNgramLM")
        if lm.vocab_size != V:
            raise ValueError(f"the language model has vocabulary {lm.vocab_size}, the logits {V}")


def beam_search(logits, beam_width=16, nbest=1, blank=0, frame_lengths=None, lm=None):
    """CTC prefix beam search; per utterance a list of at most ``nbest`` ``Hypothesis(ids, score, total)``, best first.

    ``logits``: what ``forced_align`` accepts -- a list of (T_i, V) tensors (views of one storage, as ``predict_packed``
    returns them, are read in place) or a (B, T, V) tensor with ``frame_lengths``.  ``lm``: a ``CharNgramLM`` or None.

    ``score`` is the log of the summed probability of the frame paths that spell the transcript AND whose prefixes stayed in
    the beam at every frame: a LOWER bound of the transcript's exact CTC log-probability (``-ctc_loss``), equal to it only
    when nothing was pruned.  So the best beam score may lie below the exact log-probability of the greedy transcript even
    where the beam's transcript is the better one; compare hypotheses by ``total`` (= ``score`` + LM score), and re-score with
    the CTC loss where exact values are needed.  An utterance with a NaN or +inf logit returns an empty list.  Raises
    ValueError before anything is launched for a width, nbest, blank, vocabulary or language model that does not fit."""
    import torch
    from .alignment import _logits_base
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    beam_width, nbest, blank = int(beam_width), int(nbest), int(blank)
    _check_args(V, beam_width, nbest, blank, lm)
    dev = base.device
    max_len = max(lens)
    labels = torch.empty((n, nbest, max_len), dtype=torch.int32, device=dev)
    length = torch.empty((n, nbest), dtype=torch.int32, device=dev)
    score = torch.empty((n, nbest), dtype=torch.float64, device=dev)
    total = torch.empty((n, nbest), dtype=torch.float64, device=dev)
    row0_h = np.asarray(row0, np.int64)
    frames_h = np.asarray(lens, np.int32)
    table = lm.device_table(dev) if lm is not None else None
    lib = N.load()
    N.check(lib.w2v2_ctc_beam_search(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), blank, beam_width, nbest, N.ptr(table),
                                     lm.order if lm is not None else 1, lm.alpha if lm is not None else 0.0,
                                     lm.beta if lm is not None else 0.0, max_len, N.ptr(labels), N.ptr(length), N.ptr(score),
                                     N.ptr(total), N.current_stream()), "w2v2_ctc_beam_search")
    length_h = length.cpu().numpy()
    labels_h = labels.cpu().numpy()
    score_h, total_h = score.cpu().numpy(), total.cpu().numpy()
    return [[Hypothesis(tuple(int(v) for v in labels_h[i, k, :length_h[i, k]]), float(score_h[i, k]), float(total_h[i, k]))
             for k in range(nbest) if length_h[i, k] >= 0] for i in range(n)]


class Transcript(NamedTuple):
    text: str           # the best hypothesis as text
    hypotheses: list    # the n best Hypothesis, best first (greedy: one, with score = total = NaN: the argmax path has no beam score)
    texts: list         # their texts
    words: object       # WordSpan list of the best hypothesis (timestamps=True), else None
