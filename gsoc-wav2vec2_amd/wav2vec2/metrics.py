"""Word and character error rates on the GPU (w2v2_edit_distance, csrc/edit.hip).

``edit_distance`` and ``edit_distance_pairs`` score pairs of id sequences: the edit distance and its split into hits,
substitutions, deletions and insertions, many pairs per call in one HIP launch.  ``wer`` and ``cer`` put text through them;
``oracle_wer`` and ``mbr_select`` are the two standard uses of an n-best list (how good is the list; which hypothesis has the
least expected error).  Tokenising, interning and the sums are host code over short lists; every distance comes from the kernel.

The counts are those of the alignment with the fewest errors and, among those, the fewest substitutions (equally: the most
hits).  They are unique, but the substitution / deletion / insertion split can differ from tools that backtrace with a fixed
priority: ``ab`` against ``ba`` is one deletion, one insertion and one hit here, where such tools report two substitutions.
The number of errors, and with it every rate, cannot differ.
"""

from typing import NamedTuple

import numpy as np

from . import _native as N


class EditCounts(NamedTuple):
    distance: int         # substitutions + deletions + insertions
    hits: int             # reference tokens matched
    substitutions: int
    deletions: int        # reference tokens without a counterpart
    insertions: int       # hypothesis tokens without one
    ref_len: int          # hits + substitutions + deletions


class ErrorRate(NamedTuple):
    rate: float           # sum of errors / sum of reference lengths (the corpus rate, not the mean of per-utterance rates)
    errors: int
    ref_len: int
    hits: int
    substitutions: int
    deletions: int
    insertions: int
    per_utterance: list   # the EditCounts the totals were added from

    @classmethod
    def from_counts(cls, counts):
        """The totals of a list of ``EditCounts``.  Raises ValueError when the references hold no token at all."""
        counts = list(counts)
        ref_len = sum(c.ref_len for c in counts)
        if ref_len == 0:
            raise ValueError("the references are empty: an error rate needs at least one reference token")
        errors = sum(c.distance for c in counts)
        return cls(errors / ref_len, errors, ref_len, sum(c.hits for c in counts), sum(c.substitutions for c in counts),
                   sum(c.deletions for c in counts), sum(c.insertions for c in counts), counts)


class Evaluation(NamedTuple):
    wer: ErrorRate
    cer: ErrorRate
    oracle_wer: object    # ErrorRate of the best hypothesis of each n-best list (nbest > 1), else None
    transcripts: list     # what transcribe / transcribe_long returned


def _ids(seq, what):
    int32 = isinstance(seq, np.ndarray) and seq.dtype == np.int32
    a = seq.reshape(-1) if int32 else np.asarray(seq if isinstance(seq, np.ndarray) else list(seq), dtype=np.int64).reshape(-1)
    if a.size > N.EDIT_MAX_LEN:
        raise ValueError(f"{what} has {a.size} tokens; at most {N.EDIT_MAX_LEN} per sequence")
    if int32:
        return a
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError(f"{what} holds a token outside int32")
    return a.astype(np.int32)


def edit_distance_pairs(sequences, pairs):
    """``EditCounts`` of ``sequences[h]`` (the hypothesis) against ``sequences[r]`` (the reference) for every ``(h, r)`` of
    ``pairs`` (a list of index pairs or an (n, 2) array): one upload of the pool, one kernel call.  A sequence may serve any
    number of pairs, on either side.  No pair: ``[]`` without a call.  Raises ValueError before anything is launched for an
    index outside the pool or a sequence of more than 65535 tokens."""
    pairs = np.asarray(pairs if isinstance(pairs, np.ndarray) else list(pairs), dtype=np.int64).reshape(-1, 2)
    if not len(pairs):
        return []
    seqs = [_ids(s, f"sequence {i}") for i, s in enumerate(sequences)]
    out_of_pool = np.flatnonzero(((pairs < 0) | (pairs >= len(seqs))).any(axis=1))
    if out_of_pool.size:
        k = int(out_of_pool[0])
        raise ValueError(f"pair {k} = ({pairs[k, 0]}, {pairs[k, 1]}) outside the pool of {len(seqs)} sequences")
    import torch
    lens = np.asarray([s.size for s in seqs], np.int64)
    start = np.concatenate(([0], np.cumsum(lens)[:-1]))
    flat = np.concatenate(seqs + [np.zeros(1, np.int32)])       # (one spare entry: never an empty buffer)
    hi, ri = pairs[:, 0], pairs[:, 1]
    hyp0, ref0 = np.ascontiguousarray(start[hi], np.int64), np.ascontiguousarray(start[ri], np.int64)
    hyp_len, ref_len = np.ascontiguousarray(lens[hi], np.int32), np.ascontiguousarray(lens[ri], np.int32)
    tokens = torch.from_numpy(flat).to("cuda")
    out = torch.empty((len(pairs), 4), dtype=torch.int32, device=tokens.device)
    N.check(N.load().w2v2_edit_distance(N.ptr(tokens), int(flat.size - 1), len(pairs), N.ptr(hyp0), N.ptr(hyp_len), N.ptr(ref0),
                                        N.ptr(ref_len), N.ptr(out), N.current_stream()), "w2v2_edit_distance")
    res = out.cpu().numpy().astype(np.int64)
    n = ref_len.astype(np.int64)
    cols = (res[:, 0], n - res[:, 1] - res[:, 2], res[:, 1], res[:, 2], res[:, 3], n)
    return list(map(EditCounts._make, zip(*(c.tolist() for c in cols))))


def edit_distance(hyps, refs):
    """``EditCounts`` of ``hyps[k]`` against ``refs[k]``, both lists of id sequences, in one kernel call."""
    hyps, refs = list(hyps), list(refs)
    if len(hyps) != len(refs):
        raise ValueError(f"{len(hyps)} hypotheses for {len(refs)} references")
    n = len(hyps)
    return edit_distance_pairs(hyps + refs, [(k, n + k) for k in range(n)])


def _text(item):
    if isinstance(item, str):
        return item
    t = getattr(item, "text", None)
    if not isinstance(t, str):
        raise TypeError(f"expected a string or an object with a `.text` string (a Transcript, a LongTranscript), got {type(item).__name__}")
    return t


def split_words(text):
    """The words of a text: ``text.split()``."""
    return _text(text).split()


def split_chars(text):
    """The characters of a text as code points, runs of whitespace collapsed to one space and the ends trimmed."""
    return [ord(c) for c in " ".join(_text(text).split())]


def _intern(words, table):
    return [table.setdefault(w, len(table)) for w in words]


def _rate(hypotheses, references, tokens):
    hypotheses, references = list(hypotheses), list(references)
    if len(hypotheses) != len(references):
        raise ValueError(f"{len(hypotheses)} hypotheses for {len(references)} references")
    return ErrorRate.from_counts(edit_distance([tokens(h) for h in hypotheses], [tokens(r) for r in references]))


def wer(hypotheses, references):
    """Word error rate of a corpus: an ``ErrorRate`` whose ``rate`` is the summed word errors over the summed reference
    lengths.  An item is a string or an object with ``.text`` (a ``Transcript``, a ``LongTranscript``); its words are
    ``text.split()``.  The text is compared as it is: NO case folding and NO punctuation or other normalisation is done --
    normalise both sides first where the convention of a benchmark asks for it."""
    table = {}
    return _rate(hypotheses, references, lambda t: _intern(split_words(t), table))


def cer(hypotheses, references):
    """Character error rate of a corpus, as ``wer``: the characters are the code points of ``" ".join(text.split())``.
    No case or punctuation normalisation."""
    return _rate(hypotheses, references, split_chars)


def oracle_wer(nbest_texts, references):
    """How good the n-best lists are: per utterance the hypothesis with the fewest word errors (ties: the lowest index), all
    hypotheses of all utterances scored in one kernel call.  ``nbest_texts``: per utterance a list of texts (items as for
    ``wer``), or an object with ``.texts`` (a ``Transcript``).  An utterance with no hypothesis counts as the empty string
    and gets index -1.  Returns ``(ErrorRate, chosen indices)``."""
    lists = [list(u.texts) if hasattr(u, "texts") else list(u) for u in nbest_texts]
    references = list(references)
    if len(lists) != len(references):
        raise ValueError(f"{len(lists)} n-best lists for {len(references)} references")
    table = {}
    pool, pairs, spans = [], [], []
    for hyps, ref in zip(lists, references):
        r = len(pool)
        pool.append(_intern(split_words(ref), table))
        spans.append((len(pairs), max(len(hyps), 1)))
        for h in hyps or [""]:
            pairs.append((len(pool), r))
            pool.append(_intern(split_words(h), table))
    counts = edit_distance_pairs(pool, pairs)
    best, chosen = [], []
    for (p0, K), hyps in zip(spans, lists):
        errors = [c.distance for c in counts[p0:p0 + K]]
        k = errors.index(min(errors))                    # (the first of the smallest)
        best.append(counts[p0 + k])
        chosen.append(k if hyps else -1)
    return ErrorRate.from_counts(best), chosen


def _mbr_entry(h):
    if hasattr(h, "ids") and hasattr(h, "total"):
        return h.ids, float(h.total)
    ids, score = h
    return ids, float(score)


def mbr_select(hypotheses, tokenizer=None, unit="word", scale=1.0):
    """Minimum-Bayes-risk selection from n-best lists.  ``hypotheses``: per utterance a list of ``Hypothesis`` (ranked by
    ``total``) or of ``(ids, score)``.  With p_k = softmax(scale * total_k) over the list, the risk of hypothesis k is
    R_k = sum_j p_j d(h_k, h_j), d the edit distance in words (``unit="word"``: the ids split at the tokenizer's ``|``) or in
    labels (``unit="char"``: the ids as they are); the K (K - 1) / 2 pairs of all utterances are scored in one kernel call
    (d is symmetric) and the risks are formed in fp64 on the host.  Returns ``(indices, risks)``: per utterance the argmin of
    R (ties: the lowest k; -1 for an empty list) and the array of risks."""
    if unit not in ("word", "char"):
        raise ValueError(f"unit must be 'word' or 'char', got {unit!r}")
    delim = None
    if unit == "word":
        if tokenizer is None:
            raise ValueError("unit='word' splits the ids at the tokenizer's word delimiter: pass the tokenizer")
        from .processor import WORD_DELIMITER
        delim = tokenizer.get_vocab()[WORD_DELIMITER]
    table = {}

    def tokens(ids):
        ids = [int(x) for x in ids]
        if delim is None:
            return ids
        words, cur = [], []
        for x in ids + [delim]:
            if x == delim:
                if cur:
                    words.append(tuple(cur))
                cur = []
            else:
                cur.append(x)
        return _intern(words, table)

    pool, pairs, spans, probs = [], [], [], []
    npairs = 0
    for u, hyps in enumerate(hypotheses):
        entries = [_mbr_entry(h) for h in hyps]
        base, K = len(pool), len(entries)
        pool.extend(tokens(ids) for ids, _ in entries)
        z = float(scale) * np.asarray([t for _, t in entries], np.float64)
        if K and not np.isfinite(z).all():
            raise ValueError(f"utterance {u}: a hypothesis without a finite score (the greedy path has none)")
        e = np.exp(z - z.max()) if K else z
        probs.append(e / e.sum() if K else e)
        k, j = np.triu_indices(K, 1)                     # (k, j > k), row by row
        spans.append((npairs, K, k, j))
        pairs.append(np.stack([base + k, base + j], axis=1))
        npairs += k.size
    counts = edit_distance_pairs(pool, np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64))
    dist = np.asarray([c.distance for c in counts], np.float64)
    indices, risks = [], []
    for (p0, K, k, j), p in zip(spans, probs):
        D = np.zeros((K, K), np.float64)
        D[k, j] = D[j, k] = dist[p0:p0 + k.size]
        R = (D * p[None, :]).sum(axis=1) if K else np.zeros(0, np.float64)
        risks.append(R)
        indices.append(int(np.argmin(R)) if K else -1)
    return indices, risks


def evaluate_transcripts(transcripts, references, nbest):
    """``Evaluation`` of what ``transcribe`` returned against reference texts (``Wav2Vec2ForCTC.evaluate`` is transcribe plus this)."""
    oracle = None
    if nbest > 1:
        oracle = oracle_wer([t.texts if hasattr(t, "texts") else [_text(t)] for t in transcripts], references)[0]
    return Evaluation(wer(transcripts, references), cer(transcripts, references), oracle, transcripts)
