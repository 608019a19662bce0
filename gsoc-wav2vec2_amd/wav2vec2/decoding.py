"""CTC prefix beam search and exact CTC scoring on the GPU (w2v2_ctc_beam_search, csrc/beam.hip, DESIGN.md §12;
w2v2_ctc_score and its gradient, both also with a star, csrc/score.hip).

``beam_search`` returns, per utterance, the n most probable transcripts with their log-probabilities; ``CharNgramLM`` is an
optional character n-gram language model, a dense table of log-probabilities that the kernel reads on the device.  The search
is a HIP kernel; the table is counted and smoothed on the host (it is built once) and uploaded on first use.

``WordNgramLM`` is the other kind of language model: a word-level backoff n-gram (read from an ARPA file or counted from text)
with a lexicon that spells its words in the model's labels (w2v2_ctc_beam_search_words).

``ContextBias`` is a list of phrases the search should prefer (contextual biasing, "hotwords"), compiled into an automaton that
the kernel walks beside either language model or none (w2v2_ctc_beam_search_biased).

``BeamStream`` is ``beam_search`` over logits that arrive in pieces: the beams stay on the device between calls, any chunking gives
the bits of one call, and every call reports how much of the transcript can no longer change (w2v2_ctc_beam_search_stream;
DESIGN.md §25).

``ctc_score`` is the exact CTC log-probability of label sequences given logits (the sum over all frame paths, a HIP kernel);
``rescore`` replaces the beam's lower bounds in n-best lists by it; ``hypothesis_posteriors`` and ``word_confidence`` turn the
rescored lists into probabilities of the hypotheses and of the best hypothesis' words (host code over a few numbers).
"""

import math
import os
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


BOS, EOS, UNK = "<s>", "</s>", "<unk>"
_LN10 = math.log(10.0)


def _ln32(log10_value):
    """an ARPA log10 value as the model holds it: natural log in fp64, rounded to fp32 once"""
    return float(np.float32(np.float64(log10_value) * np.float64(_LN10)))


class WordNgramLM:
    """Word n-gram backoff language model with a lexicon, for ``beam_search`` / ``Wav2Vec2ForCTC.transcribe``.

    The search splits a hypothesis into words at the label ``delimiter``.  A word that ends adds ``alpha * ln P(word | the
    order - 1 words before it) + beta`` to the hypothesis' language-model score, P by the usual backoff recursion; a label
    string that is no word of the lexicon is scored as ``<unk>`` with ``unk_penalty`` (<= 0) added to its log-probability -- or,
    with ``unk_penalty = -inf`` (the CONSTRAINED mode), a hypothesis that leaves the lexicon is dropped on the spot.  After the
    last frame the open word is ended, ``alpha * ln P(</s> | .)`` is added (``score_eos``, where the model has ``</s>``) and the
    final beam is ordered by that total.  In constrained mode an utterance can end with no hypothesis at all (every entry of
    the final beam inside an unfinished word): ``beam_search`` then returns an empty list for it, ``transcribe`` an empty text.

    ``ngrams``: {tuple of words: log10 P(last | the others)}, ``backoffs``: {tuple of words: log10 backoff weight} -- the
    contents of an ARPA file, with ``<s>``, ``</s>``, ``<unk>`` as there.  Every n-gram's context must itself be an n-gram and
    every word a unigram.  Without an ``<unk>`` unigram one is added with ``unk_logp`` (log10; required then).
    ``lexicon``: {word: label ids}, the words unigrams of the model, the ids in [0, vocab_size) without the delimiter; two words
    may not share a spelling.  Words of the model outside the lexicon can still be contexts but are never recognised.

    The model is compiled on the host into a state machine (one state per context; ``states``, ``arc0``, ``arc_word``,
    ``arc_logp``, ``arc_next``, ``bo``, ``bstate``: numpy) and the lexicon into a trie (``child`` (n_nodes, V), ``word_at``);
    ``logp`` / ``backoff`` keep the n-gram dictionary in natural log (the fp32 values).  Uploaded on first use per device."""

    MAX_ORDER = N.WORDLM_MAX_ORDER

    def __init__(self, ngrams, backoffs, lexicon, vocab_size, delimiter, alpha=1.0, beta=0.0, unk_penalty=-10.0, unk_logp=None,
                 score_eos=True):
        V, delim = int(vocab_size), int(delimiter)
        if not 2 <= V <= N.BEAM_MAX_VOCAB:
            raise ValueError(f"vocabulary {V}; 2 to {N.BEAM_MAX_VOCAB}")
        if not 0 <= delim < V:
            raise ValueError(f"word delimiter {delim} outside the vocabulary [0, {V})")
        if not (np.isfinite(alpha) and np.isfinite(beta)):
            raise ValueError("alpha and beta must be finite")
        if math.isnan(unk_penalty) or unk_penalty > 0 or unk_penalty == math.inf:
            raise ValueError(f"unk_penalty {unk_penalty}: a value <= 0, or -inf for the constrained mode")
        ngrams = {tuple(g): float(v) for g, v in ngrams.items()}
        backoffs = {tuple(g): float(v) for g, v in backoffs.items()}
        if not ngrams or any(len(g) < 1 for g in ngrams):
            raise ValueError("the model has no n-grams (or an empty one)")
        order = max(len(g) for g in ngrams)
        if not 1 <= order <= self.MAX_ORDER:
            raise ValueError(f"language model order {order}; 1 to {self.MAX_ORDER}")
        if (UNK,) not in ngrams:
            if unk_logp is None:
                raise ValueError("the model has no <unk> unigram: pass unk_logp (log10)")
            ngrams[(UNK,)] = float(unk_logp)
        for g, v in ngrams.items():
            if not math.isfinite(v):
                raise ValueError(f"n-gram {' '.join(g)}: log-probability {v} is not finite")
            if len(g) > 1 and g[:-1] not in ngrams:
                raise ValueError(f"n-gram {' '.join(g)}: its context {' '.join(g[:-1])} is no n-gram of the model")
            if (g[-1],) not in ngrams:
                raise ValueError(f"n-gram {' '.join(g)}: the word {g[-1]} is no unigram of the model")
        for g, v in backoffs.items():
            if not math.isfinite(v):
                raise ValueError(f"backoff weight of {' '.join(g)} is not finite")
            if g not in ngrams:
                raise ValueError(f"backoff weight of {' '.join(g)}, which is no n-gram of the model")
        self.ngrams, self.backoffs = ngrams, backoffs
        self.order, self.vocab_size, self.delimiter = order, V, delim
        self.alpha, self.beta, self.unk_penalty, self.score_eos = float(alpha), float(beta), float(unk_penalty), bool(score_eos)
        self.logp = {g: _ln32(v) for g, v in ngrams.items()}
        self.backoff = {g: _ln32(v) for g, v in backoffs.items()}
        self.lexicon = {}
        spelled = {}
        for w in sorted(lexicon):
            ids = tuple(int(c) for c in lexicon[w])
            if w in (BOS, EOS, UNK) or (w,) not in ngrams:
                raise ValueError(f"lexicon word {w} is no word of the model")
            if not ids or any(not 0 <= c < V or c == delim for c in ids):
                raise ValueError(f"lexicon word {w}: spelling {ids} is empty, holds the delimiter or leaves [0, {V})")
            if ids in spelled:
                raise ValueError(f"lexicon words {spelled[ids]} and {w} share the spelling {ids}")
            spelled[ids] = w
            self.lexicon[w] = ids
        if not self.lexicon:
            raise ValueError("the lexicon is empty")
        self.skipped = 0            # words of the model the tokenizer could not spell (from_arpa / from_text)
        self._dev = {}
        self._compile()
        self.validate()

    # ---- compilation -----------------------------------------------------------------------------------------------------------
    def _compile(self):
        order, V = self.order, self.vocab_size
        self.words = sorted(g[0] for g in self.logp if len(g) == 1 and g[0] != BOS)
        self.word_id = {w: i for i, w in enumerate(self.words)}
        self.unk = self.word_id[UNK]
        self.eos = self.word_id.get(EOS, -1)
        ctx = {()}
        for g in self.logp:
            ctx.add(g[:-1])
            if len(g) < order and g[-1] != EOS:
                ctx.add(g)
        self.states = sorted(ctx, key=lambda h: (len(h), h))
        sid = {h: i for i, h in enumerate(self.states)}

        def longest_suffix(h):
            while h not in sid:
                h = h[1:]
            return sid[h]

        arcs = [[] for _ in self.states]
        for g, v in self.logp.items():
            if g[-1] == BOS:
                continue
            h = g[:-1]
            arcs[sid[h]].append((self.word_id[g[-1]], v, longest_suffix(g[-(order - 1):] if order > 1 else ())))
        self.arc0 = np.zeros(len(self.states) + 1, np.int32)
        for i, a in enumerate(arcs):
            a.sort()
            self.arc0[i + 1] = self.arc0[i] + len(a)
        flat = [x for a in arcs for x in a]
        self.arc_word = np.array([x[0] for x in flat], np.int32)
        self.arc_logp = np.array([x[1] for x in flat], np.float32)
        self.arc_next = np.array([x[2] for x in flat], np.int32)
        self.bo = np.array([self.backoff.get(h, 0.0) for h in self.states], np.float32)
        self.bstate = np.array([longest_suffix(h[1:]) if h else 0 for h in self.states], np.int32)
        self.start_state = sid.get((BOS,), 0)
        # the lexicon trie
        child, word_at = [[-1] * V], [-1]
        for w, ids in self.lexicon.items():
            node = 0
            for c in ids:
                if child[node][c] < 0:
                    child[node][c] = len(child)
                    child.append([-1] * V)
                    word_at.append(-1)
                node = child[node][c]
            word_at[node] = self.word_id[w]
        self.child = np.array(child, np.int32).reshape(-1, V)
        self.word_at = np.array(word_at, np.int32)

    def validate(self):
        """The compiled arrays are what the kernel trusts: check them (ValueError)."""
        ns, na, nw, nn, V = len(self.bo), len(self.arc_word), len(self.words), len(self.word_at), self.vocab_size
        a0 = self.arc0
        if self.child.shape != (nn, V) or nn * V >= 2 ** 31:
            raise ValueError(f"the lexicon's child table has shape {self.child.shape}; ({nn}, {V}) with fewer than 2^31 entries")
        if len(a0) != ns + 1 or a0[0] != 0 or a0[-1] != na or (np.diff(a0) < 0).any() or len(self.bstate) != ns:
            raise ValueError("the arc offsets do not partition the arcs")
        if len(self.arc_logp) != na or len(self.arc_next) != na:
            raise ValueError("the arc arrays differ in length")
        if not (np.isfinite(self.arc_logp).all() and np.isfinite(self.bo).all()):
            raise ValueError("the model holds a non-finite value")
        if na and (self.arc_word.min() < 0 or self.arc_word.max() >= nw):
            raise ValueError("an arc's word id is out of range")
        if na and (self.arc_next.min() < 0 or self.arc_next.max() >= ns):
            raise ValueError("an arc's next state is out of range")
        if (self.bstate < 0).any() or (self.bstate >= np.maximum(np.arange(ns), 1)).any():
            raise ValueError("a backoff state does not precede its state")          # (states are sorted by context length)
        inner = np.ones(na, bool)
        inner[a0[1:-1][a0[1:-1] < na]] = False
        inner[0] = False
        if (np.diff(self.arc_word)[inner[1:]] <= 0).any():
            raise ValueError("the arcs of a state are not sorted by word id")
        if a0[1] != nw or not np.array_equal(self.arc_word[:nw], np.arange(nw)):
            raise ValueError("state 0 does not hold every word in order")
        if not (0 <= self.start_state < ns and 0 <= self.unk < nw and -1 <= self.eos < nw):
            raise ValueError("start state, unk or eos out of range")
        c = self.child
        if (c < -1).any() or (c >= nn).any() or (c[:, self.delimiter] >= 0).any() or (c == 0).any():
            raise ValueError("the lexicon's child table holds a bad node")
        if (self.word_at < -1).any() or (self.word_at >= nw).any() or self.word_at[0] != -1:
            raise ValueError("the lexicon's word table holds a bad word id")

    # ---- lookups on the host (tests, tools) ------------------------------------------------------------------------------------
    def lookup(self, state, word):
        """(ln P(word id | state) with the backoff weights added in order, next state): what the kernel computes"""
        acc, s = 0.0, int(state)
        while True:
            lo, hi = int(self.arc0[s]), int(self.arc0[s + 1])
            k = lo + int(np.searchsorted(self.arc_word[lo:hi], word))
            if k < hi and self.arc_word[k] == word:
                return acc + float(self.arc_logp[k]), int(self.arc_next[k])
            acc = acc + float(self.bo[s])
            s = int(self.bstate[s])

    def uses_label(self, c):
        return bool((self.child[:, int(c)] >= 0).any())

    def device_arrays(self, device):
        """(struct w2v2_word_lm, the tensors it points to) on ``device`` (uploaded on first use, then kept)"""
        import torch
        key = str(device)
        if key not in self._dev:
            self.validate()
            t = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                 for k in ("child", "word_at", "arc0", "arc_word", "arc_logp", "arc_next", "bo", "bstate")}
            st = N.W2V2WordLM()
            for k, v in t.items():
                setattr(st, k, v.data_ptr())
            st.n_nodes, st.n_states, st.n_arcs, st.n_words = len(self.word_at), len(self.bo), len(self.arc_word), len(self.words)
            st.order, st.start_state, st.unk, st.eos = self.order, self.start_state, self.unk, self.eos
            self._dev[key] = (st, t)
        return self._dev[key]

    # ---- ARPA ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def read_arpa(path_or_text):
        """(ngrams, backoffs) of an ARPA file (a path, or the text itself when it holds a line break): the \\data\\ header with
        its counts, one \\N-grams: section per order (log10 probability, N words, optional log10 backoff weight), \\end\\.
        ValueError naming the line on malformed input, a count mismatch, or an n-gram whose context is missing."""
        text = path_or_text
        if "\n" not in text:
            with open(os.fspath(path_or_text), "r", encoding="utf-8") as f:
                text = f.read()
        ngrams, backoffs, counts, seen = {}, {}, {}, {}
        section, ended, header = None, False, False

        def close(ln):
            if section and seen.get(section, 0) != counts[section]:
                raise ValueError(f"line {ln}: the {section}-grams section holds {seen.get(section, 0)} n-grams, the header says "
                                 f"{counts[section]}")

        ln = 0
        for ln, raw in enumerate(text.split("\n"), 1):
            line = raw.strip()
            if not line:
                continue
            if ended:
                raise ValueError(f"line {ln}: text after \\end\\")
            if line == "\\data\\":
                if header:
                    raise ValueError(f"line {ln}: a second \\data\\ header")
                header = True
            elif not header:
                raise ValueError(f"line {ln}: expected \\data\\, got `{line}`")
            elif line.startswith("ngram ") and section is None:
                try:
                    n, c = line[6:].split("=")
                    n, c = int(n), int(c)
                except ValueError:
                    raise ValueError(f"line {ln}: malformed count line `{line}`") from None
                if n != len(counts) + 1 or c < 0:
                    raise ValueError(f"line {ln}: count of order {n} out of sequence, or negative")
                counts[n] = c
            elif line == "\\end\\":
                close(ln)
                if section != len(counts) or not counts:
                    raise ValueError(f"line {ln}: \\end\\ before the {len(counts)}-grams section")
                ended = True
            elif line.startswith("\\") and line.endswith("-grams:"):
                close(ln)
                try:
                    n = int(line[1:-7])
                except ValueError:
                    raise ValueError(f"line {ln}: malformed section header `{line}`") from None
                if n != (section or 0) + 1 or n not in counts:
                    raise ValueError(f"line {ln}: section {n}-grams out of sequence or missing from the header")
                section = n
            elif section is None:
                raise ValueError(f"line {ln}: expected a count or a section, got `{line}`")
            else:
                f = line.split()
                if len(f) not in (section + 1, section + 2):
                    raise ValueError(f"line {ln}: a {section}-gram line has {section + 1} or {section + 2} fields, got {len(f)}")
                try:
                    p = float(f[0])
                    b = float(f[section + 1]) if len(f) == section + 2 else None
                except ValueError:
                    raise ValueError(f"line {ln}: `{line}` holds a number that does not parse") from None
                if not math.isfinite(p) or (b is not None and not math.isfinite(b)):
                    raise ValueError(f"line {ln}: non-finite value")
                g = tuple(f[1:section + 1])
                if g in ngrams:
                    raise ValueError(f"line {ln}: n-gram `{' '.join(g)}` occurs twice")
                if section > 1 and g[:-1] not in ngrams:
                    raise ValueError(f"line {ln}: the context `{' '.join(g[:-1])}` of `{' '.join(g)}` is no n-gram")
                if section > 1 and (g[-1],) not in ngrams:
                    raise ValueError(f"line {ln}: the word `{g[-1]}` of `{' '.join(g)}` is no unigram")
                ngrams[g] = p
                if b is not None:
                    backoffs[g] = b
                seen[section] = seen.get(section, 0) + 1
        if not ended:
            raise ValueError(f"line {ln}: the file ends without \\end\\")
        return ngrams, backoffs

    @staticmethod
    def spell(word, tokenizer):
        """the label ids of a word, or None where the tokenizer cannot spell it (a character it drops, maps to <unk> or to the
        word delimiter)"""
        from .processor import PAD_TOKEN, UNK_TOKEN, WORD_DELIMITER
        vocab = tokenizer.get_vocab()
        ids = tuple(int(c) for c in tokenizer(word))
        bad = (vocab[PAD_TOKEN], vocab[UNK_TOKEN], vocab[WORD_DELIMITER])
        return ids if ids and len(ids) == len(word) and not any(c in bad for c in ids) else None

    @classmethod
    def _with_tokenizer(cls, ngrams, backoffs, tokenizer, lexicon, **kw):
        from .processor import WORD_DELIMITER
        vocab = tokenizer.get_vocab()
        words = sorted(g[0] for g in ngrams if len(g) == 1) if lexicon is None else list(lexicon)
        lex, spelled, skipped = {}, set(), 0
        for w in words:
            if w in (BOS, EOS, UNK):
                continue
            ids = lexicon[w] if isinstance(lexicon, dict) else cls.spell(w, tokenizer)
            if ids is None or tuple(ids) in spelled:             # unspellable, or spelled as an earlier word (case): skipped, counted
                skipped += 1
                continue
            spelled.add(tuple(ids))
            lex[w] = tuple(ids)
        lm = cls(ngrams, backoffs, lex, max(vocab.values()) + 1, vocab[WORD_DELIMITER], **kw)
        lm.skipped = skipped
        return lm

    @classmethod
    def from_arpa(cls, path_or_text, tokenizer, alpha=1.0, beta=0.0, unk_penalty=-10.0, unk_logp=None, lexicon=None, score_eos=True):
        """The model of an ARPA file (``read_arpa``).  ``lexicon``: None = the model's unigrams without <s>, </s>, <unk>, spelled
        by ``tokenizer``; or a list of words to spell; or {word: ids}.  Words the tokenizer cannot spell are skipped and counted
        (``skipped``).  ``unk_logp`` (log10): the <unk> unigram to add where the file has none."""
        ngrams, backoffs = cls.read_arpa(path_or_text)
        return cls._with_tokenizer(ngrams, backoffs, tokenizer, lexicon, alpha=alpha, beta=beta, unk_penalty=unk_penalty,
                                   unk_logp=unk_logp, score_eos=score_eos)

    @staticmethod
    def count_ngrams(sentences, order, discount=0.75):
        """(ngrams, backoffs), log10, of word sequences by absolute discounting with backoff.  With c the counts over
        <s> w1 .. wn </s>: P(w | h) = (c(h w) - D) / c(h) for a seen h w; the mass D |seen(h)| / c(h) left over goes to the
        unseen words in proportion to P(w | h without its oldest word), i.e. bo(h) = that mass / (1 - sum over seen w of
        P(w | shorter h)).  Unigrams: the left-over mass is <unk>'s.  So sum_w P(w | h) = 1 for every context, <unk> included."""
        order = int(order)
        if not 1 <= order <= WordNgramLM.MAX_ORDER:
            raise ValueError(f"language model order {order}; 1 to {WordNgramLM.MAX_ORDER}")
        if not 0 < discount < 1:
            raise ValueError(f"discount {discount} outside (0, 1)")
        c = {}
        for sent in sentences:
            seq = [BOS] + list(sent) + [EOS]
            for w in sent:
                if w in (BOS, EOS, UNK) or not w or any(ch.isspace() for ch in w):
                    raise ValueError(f"`{w}` cannot be a word of the text")
            for i in range(1, len(seq)):
                for n in range(1, order + 1):
                    if i - n + 1 >= 0:
                        g = tuple(seq[i - n + 1:i + 1])
                        c[g] = c.get(g, 0) + 1
        if not any(len(g) == 1 and g[0] != EOS for g in c):
            raise ValueError("the text holds no word")
        by_ctx = {}
        for g, k in c.items():
            by_ctx.setdefault(g[:-1], {})[g[-1]] = k
        P, BO = {}, {}

        def prob(h, w):
            while True:
                if h + (w,) in P:
                    return P[h + (w,)]
                if not h:
                    return P[(UNK,)] if (w,) not in P else P[(w,)]
                return BO.get(h, 1.0) * prob(h[1:], w)

        for h in sorted(by_ctx, key=len):
            seen = by_ctx[h]
            tot = float(sum(seen.values()))
            for w, k in seen.items():
                P[h + (w,)] = (k - discount) / tot
            left = discount * len(seen) / tot
            if not h:
                P[(UNK,)] = left
            else:
                BO[h] = left / (1.0 - sum(prob(h[1:], w) for w in seen))
        ngrams = {g: math.log10(p) for g, p in P.items()}
        ngrams[(BOS,)] = -99.0
        backoffs = {h: math.log10(b) for h, b in BO.items()}
        return ngrams, backoffs

    @classmethod
    def from_text(cls, texts, tokenizer, order, discount=0.75, alpha=1.0, beta=0.0, unk_penalty=-10.0, lexicon=None, score_eos=True):
        """Count the word n-grams of ``texts`` (one sentence each; upper-cased, split at blanks and hyphens, as the tokenizer
        reads them) and smooth them with ``count_ngrams``; the lexicon as in ``from_arpa``."""
        sents = [t.upper().replace("-", " ").split() for t in texts]
        ngrams, backoffs = cls.count_ngrams(sents, order, discount)
        return cls._with_tokenizer(ngrams, backoffs, tokenizer, lexicon, alpha=alpha, beta=beta, unk_penalty=unk_penalty,
                                   score_eos=score_eos)

    def to_arpa(self, path=None):
        """The model as ARPA text (written to ``path`` if given): values in log10 with every digit, so that reading it back
        gives the same model."""
        out = ["\\data\\"]
        by_n = [sorted(g for g in self.ngrams if len(g) == n) for n in range(1, self.order + 1)]
        out += [f"ngram {n}={len(gs)}" for n, gs in enumerate(by_n, 1)]
        for n, gs in enumerate(by_n, 1):
            out += ["", f"\\{n}-grams:"]
            for g in gs:
                line = f"{self.ngrams[g]!r}\t{' '.join(g)}"
                if g in self.backoffs:
                    line += f"\t{self.backoffs[g]!r}"
                out.append(line)
        out += ["", "\\end\\", ""]
        text = "\n".join(out)
        if path is not None:
            with open(os.fspath(path), "w", encoding="utf-8") as f:
                f.write(text)
        return text


class ContextBias:
    """Phrase boosting (contextual biasing, "hotwords") for ``beam_search``: a list of phrases the search should prefer, compiled
    into an Aho-Corasick automaton with resolved failure links that the kernel reads as dense tables (exact
    definition in csrc/beam.hip, third part of its header; tests/bias_reference.py computes it from the prefix alone).

    A phrase ``h`` is a label string with a boost ``b_h`` >= 0 in nats per COUNTED label, weight ``w_h = b_h * counted(h)``.
    ``whole_words`` wraps every phrase in one leading and one trailing ``delimiter`` (not counted), so that it matches whole words
    only; the start and the end of the utterance count as delimiters.  The bias of a prefix ``p`` is ``B(p) = C(p) + phi(state(p))``:
    ``C`` the summed weights of EVERY occurrence of every phrase in ``p`` (overlapping and nested phrases all count: with the
    phrases NEW YORK and YORK the string NEW YORK earns both), ``state(p)`` the longest suffix of ``p`` that begins a phrase and
    ``phi(s) = partial * counted(s) * max{b_h : s a proper prefix of h}`` a look-ahead credit that keeps a phrase under way in the
    beam (``partial`` in [0, 1]; the default 1.0 is a convention -- the full per-label boost in advance -- not a tuned value; 0
    rewards completed phrases only).  Credit for a phrase that is not finished is taken back, at the label that leaves it or at
    the end of the utterance.

    ``next`` (n_states, V) int32, ``delta`` (n_states, V) fp32, ``final`` (n_states) fp32, ``start_state``: the compiled tables
    (numpy; state 0 the root; the blank's column is ``next = s``, ``delta = 0``).  ``delta`` and ``final`` are formed in fp64 --
    ``(sum of w_h in phrase order + phi(s')) - phi(s)`` and ``E(s) - phi(s)`` -- and rounded to fp32 once."""

    MAX_STATES = N.BIAS_MAX_STATES

    def __init__(self, phrases, vocab_size, blank, delimiter=None, partial=1.0, whole_words=False):
        """``phrases``: [(label ids, boost)]; see ``from_ids`` / ``from_phrases``"""
        V, blank = int(vocab_size), int(blank)
        if V < 2:
            raise ValueError(f"vocabulary {V}; the blank and at least one label")
        if not 0 <= blank < V:
            raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
        if delimiter is not None and (not 0 <= int(delimiter) < V or int(delimiter) == blank):
            raise ValueError(f"word delimiter {delimiter} outside the vocabulary [0, {V}) or the blank")
        if whole_words and delimiter is None:
            raise ValueError("whole_words needs a word delimiter")
        partial = float(partial)
        if not 0.0 <= partial <= 1.0:                        # (NaN fails too)
            raise ValueError(f"partial {partial} outside [0, 1]")
        phrases = list(phrases)
        if not phrases:
            raise ValueError("the bias holds no phrase")
        self.vocab_size, self.blank, self.partial, self.whole_words = V, blank, partial, bool(whole_words)
        self.delimiter = None if delimiter is None else int(delimiter)
        self.lead = 1 if self.whole_words else 0             # uncounted boundary labels at either end of a phrase
        self.phrases, self.boosts = [], []
        for i, (ids, b) in enumerate(phrases):
            ids, b = tuple(int(c) for c in ids), float(b)
            if not ids:
                raise ValueError(f"phrase {i} has an empty spelling")
            if any(not 0 <= c < V or c == blank for c in ids):
                raise ValueError(f"phrase {i}: labels {ids} hold the blank or leave [0, {V})")
            if not math.isfinite(b) or b < 0:
                raise ValueError(f"phrase {i}: boost {b} is not a finite value >= 0")
            self.phrases.append((self.delimiter,) * self.lead + ids + (self.delimiter,) * self.lead)
            self.boosts.append(b)
        self._dev = {}
        self._compile()
        self.validate()

    @classmethod
    def from_ids(cls, id_sequences, V, blank, delimiter=None, boost=2.0, partial=1.0, whole_words=False):
        """The model-free form: ``id_sequences`` holds label sequences or ``(sequence, boost)`` pairs (``boost``: the others')."""
        items = []
        for x in id_sequences:
            pair = isinstance(x, (tuple, list)) and len(x) == 2 and hasattr(x[0], "__len__")
            items.append((x[0], x[1]) if pair else (x, boost))
        return cls(items, V, blank, delimiter, partial, whole_words)

    @classmethod
    def from_phrases(cls, phrases, tokenizer, boost=2.0, partial=1.0, whole_words=True):
        """``phrases``: strings or ``(string, boost)`` pairs, read as the tokenizer reads text (upper-cased, split at blanks and
        hyphens); every word is spelled as ``WordNgramLM.spell`` spells it and the words are joined by the tokenizer's word
        delimiter.  A phrase with a word the tokenizer cannot spell is a ValueError."""
        from .processor import PAD_TOKEN, WORD_DELIMITER
        vocab = tokenizer.get_vocab()
        delim = vocab[WORD_DELIMITER]
        items = []
        for x in phrases:
            text, b = (x, boost) if isinstance(x, str) else (x[0], x[1])
            ids = []
            for w in text.upper().replace("-", " ").split():
                sp = WordNgramLM.spell(w, tokenizer)
                if sp is None:
                    raise ValueError(f"phrase `{text}`: the tokenizer cannot spell `{w}`")
                ids += ([delim] if ids else []) + list(sp)
            if not ids:
                raise ValueError(f"phrase `{text}` has an empty spelling")
            items.append((ids, b))
        return cls(items, max(vocab.values()) + 1, vocab[PAD_TOKEN], delim, partial, whole_words)

    # ---- compilation -----------------------------------------------------------------------------------------------------------
    def _compile(self):
        V, lead = self.vocab_size, self.lead
        goto, depth, own = {}, [0], [[]]                     # the trie: (state, label) -> state; phrases that end at a state
        for i, h in enumerate(self.phrases):
            s = 0
            for c in h:
                nx = goto.get((s, c))
                if nx is None:
                    nx = len(depth)
                    if nx + 1 > self.MAX_STATES:
                        raise ValueError(f"the phrases need more than {self.MAX_STATES} automaton states")
                    if (nx + 1) * V >= 2 ** 31:
                        raise ValueError(f"the phrases need {nx + 1} or more states: states * vocabulary {V} reaches 2^31")
                    goto[(s, c)] = nx
                    depth.append(depth[s] + 1)
                    own.append([])
                s = nx
            own[s].append(i)
        ns = len(depth)
        # best boost among the phrases a state is a PROPER prefix of
        maxb = np.full(ns, -1.0)
        for i, h in enumerate(self.phrases):
            s = 0
            for c in h:
                maxb[s] = max(maxb[s], self.boosts[i])
                s = goto[(s, c)]
        counted = np.maximum(np.asarray(depth, np.float64) - lead, 0.0)
        phi = np.where(maxb >= 0, (self.partial * counted) * np.maximum(maxb, 0.0), 0.0)
        phi[0] = 0.0
        # breadth first (states are numbered by insertion, so sort by depth): failure links resolved into the dense table
        kids = [[] for _ in range(ns)]
        for (s, c), nx in goto.items():
            kids[s].append((c, nx))
        nxt = np.zeros((ns, V), np.int32)
        fail = np.zeros(ns, np.int64)
        outs = [None] * ns                                   # phrase indices that end at the state's string, ascending
        outs[0] = []
        order = sorted(range(ns), key=lambda s: depth[s])
        for s in order:
            if s:
                nxt[s] = nxt[fail[s]]
                f = outs[fail[s]]
                outs[s] = sorted(own[s] + f) if own[s] and f else (own[s] or f)
            for c, k in kids[s]:
                fail[k] = nxt[fail[s], c] if s else 0
                nxt[s, c] = k
        w = [b * float(len(h) - 2 * lead) for h, b in zip(self.phrases, self.boosts)]
        osum = np.zeros(ns)
        for s in range(ns):
            acc = 0.0
            for i in outs[s]:
                acc = acc + w[i]
            osum[s] = acc
        delta = ((osum[nxt] + phi[nxt]) - phi[:, None]).astype(np.float32)
        rows = np.arange(ns, dtype=np.int32)
        nxt[:, self.blank] = rows
        delta[:, self.blank] = 0.0
        if self.whole_words:
            final = (osum[nxt[:, self.delimiter]] - phi).astype(np.float32)
            self.start_state = int(nxt[0, self.delimiter])
        else:
            final = (0.0 - phi).astype(np.float32)
            self.start_state = 0
        self.next, self.delta, self.final = np.ascontiguousarray(nxt), np.ascontiguousarray(delta), final
        self.weights = w
        self.n_states = ns
        self._outs = outs

    def validate(self):
        """The compiled tables are what the kernel trusts: check them (ValueError)."""
        ns, V = self.n_states, self.vocab_size
        if not 1 <= ns <= self.MAX_STATES or ns * V >= 2 ** 31:
            raise ValueError(f"{ns} automaton states; 1 to {self.MAX_STATES}, and states * vocabulary below 2^31")
        if self.next.shape != (ns, V) or self.delta.shape != (ns, V) or self.final.shape != (ns,):
            raise ValueError(f"the bias tables have shapes {self.next.shape}, {self.delta.shape}, {self.final.shape}; ({ns}, {V}) and ({ns},)")
        if self.next.dtype != np.int32 or self.delta.dtype != np.float32 or self.final.dtype != np.float32:
            raise ValueError("the bias tables must be int32 (next) and float32 (delta, final)")
        if (self.next < 0).any() or (self.next >= ns).any():
            raise ValueError("a next state is out of range")
        if not (np.isfinite(self.delta).all() and np.isfinite(self.final).all()):
            raise ValueError("the bias holds a non-finite value")
        if not np.array_equal(self.next[:, self.blank], np.arange(ns)) or (self.delta[:, self.blank] != 0).any():
            raise ValueError("the blank's column must stay in place and add nothing")
        if not 0 <= self.start_state < ns:
            raise ValueError(f"start state {self.start_state} outside [0, {ns})")

    def uses_label(self, c):
        return any(int(c) in h for h in self.phrases)

    def device_arrays(self, device):
        """(struct w2v2_ctc_bias, the tensors it points to) on ``device`` (uploaded on first use, then kept)"""
        import torch
        key = str(device)
        if key not in self._dev:
            self.validate()
            t = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device) for k in ("next", "delta", "final")}
            st = N.W2V2CtcBias()
            for k, v in t.items():
                setattr(st, k, v.data_ptr())
            st.n_states, st.start_state = self.n_states, self.start_state
            self._dev[key] = (st, t)
        return self._dev[key]

    def score(self, ids):
        """(the bias of the transcript ``ids`` at the end of an utterance -- the table values along it and ``final``, summed in
        fp64 in the search's order: what the search adds to ``total`` beside the language model -- and the matches: a list of
        (phrase index, position of its first counted label in ``ids``, position of its last), by last position, then phrase)"""
        s, acc, matches = self.start_state, 0.0, []
        lead = self.lead

        def fired(state, end):                               # `end`: position of the phrase's last label, a boundary delimiter included
            for i in self._outs[state]:
                n = len(self.phrases[i])
                matches.append((i, end - n + 1 + lead, end - lead))

        for k, c in enumerate(ids):
            c = int(c)
            if not 0 <= c < self.vocab_size or c == self.blank:
                raise ValueError(f"label {c} at position {k} is the blank or outside [0, {self.vocab_size})")
            acc = acc + float(self.delta[s, c])
            s = int(self.next[s, c])
            fired(s, k)
        if self.whole_words:
            fired(int(self.next[s, self.delimiter]), len(ids))
        return acc + float(self.final[s]), matches


def _check_args(V, beam_width, nbest, blank, lm, bias=None):
    if bias is not None:
        if not isinstance(bias, ContextBias):
            raise ValueError("`bias` must be a ContextBias")
        if bias.vocab_size != V:
            raise ValueError(f"the bias has vocabulary {bias.vocab_size}, the logits {V}")
        if bias.blank != blank or bias.uses_label(blank):
            raise ValueError(f"blank {blank} is a label of the bias' phrases (the bias was built with blank {bias.blank})")
        if isinstance(lm, WordNgramLM) and bias.delimiter is not None and bias.delimiter != lm.delimiter:
            raise ValueError(f"the bias has word delimiter {bias.delimiter}, the language model {lm.delimiter}")
    if not 1 <= V <= N.BEAM_MAX_VOCAB:
        raise ValueError(f"vocabulary {V}; the beam search takes at most {N.BEAM_MAX_VOCAB}")
    if not 1 <= beam_width <= N.BEAM_MAX_WIDTH:
        raise ValueError(f"beam_width {beam_width}; 1 to {N.BEAM_MAX_WIDTH}")
    if not 1 <= nbest <= beam_width:
        raise ValueError(f"nbest {nbest} outside [1, beam_width {beam_width}]")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    if isinstance(lm, WordNgramLM):
        if lm.vocab_size != V:
            raise ValueError(f"the language model has vocabulary {lm.vocab_size}, the logits {V}")
        if lm.delimiter == blank or lm.uses_label(blank):
            raise ValueError(f"blank {blank} is the language model's word delimiter or a letter of its lexicon")
    elif lm is not None:
        if not isinstance(lm, CharNgramLM):
            raise ValueError("`lm` must be a CharNgramLM or a WordNgramLM")
        if lm.vocab_size != V:
            raise ValueError(f"the language model has vocabulary {lm.vocab_size}, the logits {V}")


def beam_search(logits, beam_width=16, nbest=1, blank=0, frame_lengths=None, lm=None, bias=None):
    """CTC prefix beam search; per utterance a list of at most ``nbest`` ``Hypothesis(ids, score, total)``, best first.

    ``logits``: what ``forced_align`` accepts -- a list of (T_i, V) tensors (views of one storage, as ``predict_packed``
    returns them, are read in place) or a (B, T, V) tensor with ``frame_lengths``.  ``lm``: a ``CharNgramLM``, a
    ``WordNgramLM`` (whose word delimiter and weights are the object's; see there for the constrained mode, in which an
    utterance may return an empty list) or None.  ``bias``: a ``ContextBias`` (phrases to prefer, with any ``lm``; its bonuses are
    part of ``total``, and the final beam is ordered by ``total`` after the end-of-utterance term) or None, which takes exactly the
    search without one.

    ``score`` is the log of the summed probability of the frame paths that spell the transcript AND whose prefixes stayed in
    the beam at every frame: a LOWER bound of the transcript's exact CTC log-probability (``-ctc_loss``), equal to it only
    when nothing was pruned.  So the best beam score may lie below the exact log-probability of the greedy transcript even
    where the beam's transcript is the better one; compare hypotheses by ``total`` (= ``score`` + LM score), and pass the lists
    through ``rescore`` where exact values are needed.  An utterance with a NaN or +inf logit returns an empty list.  Raises
    ValueError before anything is launched for a width, nbest, blank, vocabulary or language model that does not fit."""
    import torch
    from .alignment import _logits_base
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    beam_width, nbest, blank = int(beam_width), int(nbest), int(blank)
    _check_args(V, beam_width, nbest, blank, lm, bias)
    dev = base.device
    max_len = max(lens)
    labels = torch.empty((n, nbest, max_len), dtype=torch.int32, device=dev)
    length = torch.empty((n, nbest), dtype=torch.int32, device=dev)
    score = torch.empty((n, nbest), dtype=torch.float64, device=dev)
    total = torch.empty((n, nbest), dtype=torch.float64, device=dev)
    row0_h = np.asarray(row0, np.int64)
    frames_h = np.asarray(lens, np.int32)
    lib = N.load()
    if bias is not None:
        import ctypes
        word = isinstance(lm, WordNgramLM)
        bst, _keep_bias = bias.device_arrays(dev)
        st, _keep = lm.device_arrays(dev) if word else (None, None)
        table = lm.device_table(dev) if lm is not None and not word else None
        N.check(lib.w2v2_ctc_beam_search_biased(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), blank, beam_width, nbest, N.ptr(table),
                                                1 if lm is None or word else lm.order, ctypes.byref(st) if word else None,
                                                lm.delimiter if word else 0, lm.alpha if lm is not None else 0.0,
                                                lm.beta if lm is not None else 0.0, lm.unk_penalty if word else 0.0,
                                                int(lm.score_eos) if word else 0, ctypes.byref(bst), max_len, N.ptr(labels), N.ptr(length),
                                                N.ptr(score), N.ptr(total), N.current_stream()), "w2v2_ctc_beam_search_biased")
        return _hypotheses(n, nbest, labels, length, score, total)
    if isinstance(lm, WordNgramLM):
        import ctypes
        st, _keep = lm.device_arrays(dev)
        N.check(lib.w2v2_ctc_beam_search_words(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), blank, beam_width, nbest,
                                               ctypes.byref(st), lm.delimiter, lm.alpha, lm.beta, lm.unk_penalty, int(lm.score_eos),
                                               max_len, N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.current_stream()),
                "w2v2_ctc_beam_search_words")
        return _hypotheses(n, nbest, labels, length, score, total)
    table = lm.device_table(dev) if lm is not None else None
    N.check(lib.w2v2_ctc_beam_search(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), blank, beam_width, nbest, N.ptr(table),
                                     lm.order if lm is not None else 1, lm.alpha if lm is not None else 0.0,
                                     lm.beta if lm is not None else 0.0, max_len, N.ptr(labels), N.ptr(length), N.ptr(score),
                                     N.ptr(total), N.current_stream()), "w2v2_ctc_beam_search")
    return _hypotheses(n, nbest, labels, length, score, total)


def _hypotheses(n, nbest, labels, length, score, total):
    length_h = length.cpu().numpy()
    labels_h = labels.cpu().numpy()
    score_h, total_h = score.cpu().numpy(), total.cpu().numpy()
    return [[Hypothesis(tuple(int(v) for v in labels_h[i, k, :length_h[i, k]]), float(score_h[i, k]), float(total_h[i, k]))
             for k in range(nbest) if length_h[i, k] >= 0] for i in range(n)]


class StreamStep(NamedTuple):
    hypotheses: object  # the stream's n best Hypothesis so far, best first (None when the call asked for no results)
    stable_len: int     # leading labels that every entry of the beam shares: no later call can change them
    frames_done: int    # frames of the stream searched so far


class BeamStream:
    """The beam search of ``beam_search`` over logits that arrive in pieces (w2v2_ctc_beam_search_stream): ``n``
    independent streams, each with its beam kept on the device between calls.  Feeding a stream's frames in any chunking -- empty
    chunks included -- gives, bit for bit, what one ``beam_search`` call over all of them gives.

    ``lm``, ``bias``, ``beam_width``, ``nbest``, ``blank`` and ``vocab_size`` are fixed for the object's life (the kernel trusts
    that they do not change within a stream).  The object owns per stream a state slab, a trie buffer and the count of frames
    done.  A trie buffer starts with room for ``initial_frames`` frames and doubles, by allocate-and-copy on the current torch
    stream, when the next call would not fit; should the buffers of all streams then exceed ``max_workspace_bytes`` (None: 8 GiB)
    the call raises MemoryError before anything is allocated.  A stream that meets a NaN or +inf logit is dead: it returns no
    hypothesis from then on, until ``reset``."""

    DEFAULT_MAX_WORKSPACE = 8 << 30

    def __init__(self, n, vocab_size, beam_width=16, nbest=1, blank=0, lm=None, bias=None, max_workspace_bytes=None, initial_frames=256):
        import torch
        n, V = int(n), int(vocab_size)
        beam_width, nbest, blank, initial_frames = int(beam_width), int(nbest), int(blank), int(initial_frames)
        if n < 1:
            raise ValueError(f"{n} streams; at least one")
        _check_args(V, beam_width, nbest, blank, lm, bias)
        if initial_frames < 1:
            raise ValueError(f"initial_frames {initial_frames}: at least one")
        cap = self.DEFAULT_MAX_WORKSPACE if max_workspace_bytes is None else int(max_workspace_bytes)
        if cap < 1:
            raise ValueError(f"max_workspace_bytes {cap} must be positive")
        self.n, self.vocab_size, self.beam_width, self.nbest, self.blank, self.lm, self.bias = n, V, beam_width, nbest, blank, lm, bias
        self.max_workspace_bytes = cap
        self._cap_frames = [initial_frames] * n
        if 8 * sum(self._entries(c) for c in self._cap_frames) > cap:
            raise MemoryError(f"BeamStream: {n} streams of {initial_frames} frames at width {beam_width} need "
                              f"{8 * sum(self._entries(c) for c in self._cap_frames)} bytes of trie; max_workspace_bytes is {cap}")
        self._lib = N.load()
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._state = torch.zeros((n, int(self._lib.w2v2_ctc_beam_stream_state_bytes())), dtype=torch.uint8, device=self.device)
        self._nodes = [torch.zeros(self._entries(c), dtype=torch.int64, device=self.device) for c in self._cap_frames]
        self._stable = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._empty = torch.zeros((1, V), dtype=torch.float32, device=self.device)
        self.frames_done = np.zeros(n, np.int64)

    def _entries(self, frames):
        return int(frames) * self.beam_width + 1

    def reset(self, i):
        """Start stream ``i`` again from the empty prefix (its buffers are kept)."""
        if not 0 <= int(i) < self.n:
            raise ValueError(f"stream {i} outside [0, {self.n})")
        self.frames_done[int(i)] = 0

    def _grow(self, need_frames):
        """trie room for ``need_frames[i]`` frames of stream i: doubled until it fits, the nodes written so far copied"""
        import torch
        new = list(self._cap_frames)
        for i, f in enumerate(need_frames):
            while new[i] < f:
                new[i] *= 2
        if new == self._cap_frames:
            return
        total = 8 * sum(self._entries(c) for c in new)
        if total > self.max_workspace_bytes:
            grown = ", ".join(f"stream {i}: {f} frames" for i, f in enumerate(need_frames) if new[i] != self._cap_frames[i])
            raise MemoryError(f"BeamStream: {grown} at width {self.beam_width} need {total} bytes of trie in all; "
                              f"max_workspace_bytes is {self.max_workspace_bytes}")
        for i, c in enumerate(new):
            if c != self._cap_frames[i]:
                buf = torch.zeros(self._entries(c), dtype=torch.int64, device=self.device)
                used = self._entries(min(int(self.frames_done[i]), self._cap_frames[i]))
                buf[:used].copy_(self._nodes[i][:used])
                self._nodes[i], self._cap_frames[i] = buf, c

    def advance(self, logits, results=True):
        """Search the next frames of every stream: ``logits`` holds one (T_i, V) tensor or None (no new frame) per stream, read in
        place where ``beam_search`` would read them in place.  Returns one ``StreamStep(hypotheses, stable_len, frames_done)`` per
        stream; the hypotheses are those of everything searched so far, as ``beam_search`` would return them had the utterance
        ended here (an empty list for a dead stream or one without a hypothesis).  ``results=False`` only advances the beams
        (``hypotheses`` is None): the call skips the walk that writes the transcripts."""
        import ctypes
        import torch
        from .alignment import _logits_base
        if isinstance(logits, torch.Tensor) and logits.dim() == 2 and self.n == 1:
            logits = [logits]
        logits = list(logits)
        if len(logits) != self.n:
            raise ValueError(f"{len(logits)} entries for {self.n} streams")
        n, V = self.n, self.vocab_size
        for i, l in enumerate(logits):
            if l is not None and (not isinstance(l, torch.Tensor) or l.dim() != 2 or int(l.shape[1]) != V):
                raise ValueError(f"stream {i}: logits must be a (T_i, {V}) tensor or None")
        have = [i for i, l in enumerate(logits) if l is not None and int(l.shape[0]) > 0]
        row0_h, frames_h = np.zeros(n, np.int64), np.zeros(n, np.int32)
        base = self._empty
        if have:
            base, row0, lens = _logits_base([logits[i] for i in have], None)
            if base.device != self.device:
                raise ValueError(f"the logits live on {base.device}, the streams on {self.device}")
            row0_h[have], frames_h[have] = row0, lens
        after = self.frames_done + frames_h
        if int((after * self.beam_width).max()) >= 2 ** 31 - 1:
            raise ValueError(f"a stream would reach {int(after.max())} frames: frames * beam_width must stay below 2^31 - 1")
        self._grow(after.tolist())
        lo = min(t.data_ptr() for t in self._nodes)
        node0_h = np.asarray([(t.data_ptr() - lo) // 8 for t in self._nodes], np.int64)
        cap_h = np.asarray([t.numel() for t in self._nodes], np.int64)
        done_h = np.ascontiguousarray(self.frames_done)
        lm, bias = self.lm, self.bias
        word = isinstance(lm, WordNgramLM)
        bst, _keep_bias = bias.device_arrays(self.device) if bias is not None else (None, None)
        st, _keep = lm.device_arrays(self.device) if word else (None, None)
        table = lm.device_table(self.device) if lm is not None and not word else None
        labels = length = score = total = None
        max_len = max(1, int(after.max()))
        if results:
            labels = torch.empty((n, self.nbest, max_len), dtype=torch.int32, device=self.device)
            length = torch.empty((n, self.nbest), dtype=torch.int32, device=self.device)
            score = torch.empty((n, self.nbest), dtype=torch.float64, device=self.device)
            total = torch.empty((n, self.nbest), dtype=torch.float64, device=self.device)
        N.check(self._lib.w2v2_ctc_beam_search_stream(
            N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), N.ptr(done_h), self.blank, self.beam_width, self.nbest, N.ptr(table),
            1 if lm is None or word else lm.order, ctypes.byref(st) if word else None, lm.delimiter if word else 0,
            lm.alpha if lm is not None else 0.0, lm.beta if lm is not None else 0.0, lm.unk_penalty if word else 0.0,
            int(lm.score_eos) if word else 0, ctypes.byref(bst) if bias is not None else None, N.ptr(self._state), ctypes.c_void_p(lo),
            N.ptr(node0_h), N.ptr(cap_h), max_len, N.ptr(labels), N.ptr(length), N.ptr(score), N.ptr(total), N.ptr(self._stable),
            N.current_stream()), "w2v2_ctc_beam_search_stream")
        self.frames_done = after
        stable = self._stable.cpu().numpy()
        hyps = _hypotheses(n, self.nbest, labels, length, score, total) if results else [None] * n
        return [StreamStep(hyps[i], int(stable[i]), int(after[i])) for i in range(n)]


class Transcript(NamedTuple):
    text: str           # the best hypothesis as text
    hypotheses: list    # the n best Hypothesis, best first (greedy: one, with score = total = NaN: the argmax path has no beam score)
    texts: list         # their texts
    words: object       # WordSpan list of the best hypothesis (timestamps=True), else None


class ScoredTranscript(NamedTuple):
    text: str               # the best hypothesis as text
    hypotheses: list        # the n best Hypothesis with exact scores, best first
    texts: list             # their texts
    words: list             # WordSpan list of the best hypothesis
    confidence: float       # posterior of the best hypothesis among the list (NaN for an utterance without hypotheses)
    posteriors: list        # posterior of every hypothesis, parallel to ``hypotheses``
    word_confidence: list   # per word of ``words``: the summed posterior of the hypotheses that hold the word at its place


def _check_score_labels(labels, V, blank, star=False):
    """The label sequences of ``ctc_score`` / ``ctc_score_grad`` as int32 arrays, checked (host code).  ``star``: the label V is
    admitted (the star), two of them next to each other are not."""
    from .alignment import _host
    labs = []
    for j, lab in enumerate(labels):
        a = np.asarray(_host(lab) if hasattr(lab, "cpu") else list(lab), dtype=np.int64).reshape(-1)
        if star:
            if a.size and (a.min() < 0 or a.max() > V):
                raise ValueError(f"pair {j}: labels must lie in [0, {V}] ({V} is the star), got [{a.min()}, {a.max()}]")
            if a.size > 1 and ((a[1:] == V) & (a[:-1] == V)).any():
                raise ValueError(f"pair {j}: two stars next to each other; collapse them into one")
        elif a.size and (a.min() < 0 or a.max() >= V):
            raise ValueError(f"pair {j}: labels must lie in [0, {V}), got [{a.min()}, {a.max()}]")
        if a.size and (a == blank).any():
            raise ValueError(f"pair {j}: label {blank} is the blank")
        if a.size > N.SCORE_MAX_LABELS:
            raise ValueError(f"pair {j}: {a.size} labels; at most {N.SCORE_MAX_LABELS} per pair")
        labs.append(a.astype(np.int32))
    return labs


def _score_pairs(logits, labels, blank, frame_lengths, utterance, star=False):
    """The arguments ``ctc_score`` and ``ctc_score_grad`` share, checked: (base, V, row0, frames, utt, labels_dev, label0, nlabels,
    blank) with the host arrays in the dtypes of the C ABI.  ``star``: the label V is admitted (the star), two of them next to each
    other are not."""
    import torch
    from .alignment import _logits_base
    base, row0, lens = _logits_base(logits, frame_lengths)
    n, V = len(lens), int(base.shape[1])
    labels = list(labels)
    m = len(labels)
    if utterance is None:
        if m != n:
            raise ValueError(f"{m} label sequences for {n} utterances (pass `utterance` to score several per utterance)")
        utt = np.arange(n, dtype=np.int32)
    else:
        utt = np.asarray(list(utterance), dtype=np.int64).reshape(-1)
        if utt.size != m:
            raise ValueError(f"{m} label sequences with {utt.size} entries of `utterance`")
        if m and (utt.min() < 0 or utt.max() >= n):
            raise ValueError(f"`utterance` must lie in [0, {n}), got [{utt.min()}, {utt.max()}]")
        utt = utt.astype(np.int32)
    if m < 1:
        raise ValueError("no label sequence to score")
    blank = int(blank)
    if V < 2:
        raise ValueError(f"vocabulary {V}; the blank and at least one label")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary [0, {V})")
    labs = _check_score_labels(labels, V, blank, star)
    flat = np.concatenate(labs + [np.zeros(1, np.int32)])      # (one spare entry: never an empty buffer)
    label0 = np.cumsum([0] + [a.size for a in labs[:-1]]).astype(np.int64)
    nlab_h = np.asarray([a.size for a in labs], np.int32)
    labels_dev = torch.from_numpy(flat).to(base.device)
    return base, V, np.asarray(row0, np.int64), np.asarray(lens, np.int32), utt, labels_dev, label0, nlab_h, blank


def ctc_score(logits, labels, blank=0, frame_lengths=None, utterance=None, star_score=None):
    """Exact CTC log-probability of each label sequence given its utterance's logits (``-ctc_loss`` in fp64; w2v2_ctc_score):
    a float64 numpy array with one entry per pair.

    ``logits``: what ``forced_align`` accepts, read in place.  ``labels``: one id sequence per pair, none of them the blank, at
    most 8191 ids.  ``utterance[j]`` is the utterance pair j scores (default: j, which needs one label sequence per utterance);
    several pairs may score the same utterance, whose logits are read where they lie.  Too few frames for the labels
    (T < U + repeated neighbours) is no error: that pair's result is ``-inf``.  An utterance with a NaN or +inf logit gives NaN.
    Raises ValueError, naming the pair, for a label outside the vocabulary, a blank label or more than 8191 labels.

    ``star_score``: None is the call without a star: the label V is a ValueError.  A float <= 0 admits the star, label id V =
    ``alignment.star_id(logits)`` (w2v2_ctc_score_star): it may stand anywhere, takes at least one frame, counts as
    a label in the frame check and emits, per frame, max_v log_softmax(logits[t])[v] + star_score.  The result is then the score of
    a set of paths, not a log-probability: it may exceed 0, and it is never below ``forced_align(..., star_score=...)``'s score.
    Two stars next to each other and a star_score that is NaN or > 0 raise ValueError.  Pairs without a star get the bits of the
    call without ``star_score``."""
    import torch
    star = star_score is not None
    if star:
        from .alignment import _check_star_score
        star_score = _check_star_score(star_score)
    base, V, row0_h, frames_h, utt, labels_dev, label0, nlab_h, blank = _score_pairs(logits, labels, blank, frame_lengths, utterance, star)
    m = len(nlab_h)
    logp = torch.empty(m, dtype=torch.float64, device=base.device)
    if star:
        N.check(N.load().w2v2_ctc_score_star(N.ptr(base), V, len(frames_h), N.ptr(row0_h), N.ptr(frames_h), m, N.ptr(utt),
                                             N.ptr(labels_dev), N.ptr(label0), N.ptr(nlab_h), blank, star_score, N.ptr(logp),
                                             N.current_stream()), "w2v2_ctc_score_star")
        return logp.cpu().numpy()
    N.check(N.load().w2v2_ctc_score(N.ptr(base), V, len(frames_h), N.ptr(row0_h), N.ptr(frames_h), m, N.ptr(utt), N.ptr(labels_dev),
                                    N.ptr(label0), N.ptr(nlab_h), blank, N.ptr(logp), N.current_stream()), "w2v2_ctc_score")
    return logp.cpu().numpy()


def ctc_score_grad(logits, labels, coef, blank=0, frame_lengths=None, utterance=None, max_workspace_bytes=8 << 30, star_score=None):
    """The gradient of a weighted sum of exact CTC log-probabilities (w2v2_ctc_score_grad): ``(logp, grad)`` with
    ``logp`` what ``ctc_score`` returns for the same pairs, bit for bit, and ``grad`` = d (sum_j coef_j logp_j) / d logits in fp32.

    ``logits``, ``labels``, ``utterance`` and the ValueErrors are those of ``ctc_score``.  ``coef``: one float per pair, on the host
    or as a device float64 tensor.  ``grad`` has the form of ``logits``: a padded (B, T, V) tensor with zero rows beyond each
    length, or a list with one (T_i, V) tensor per utterance.  A pair whose ``logp`` is ``-inf`` or NaN contributes nothing; an
    utterance none of whose pairs contributes gets zeros.  ``coef = -1`` on one pair per utterance is the CTC loss in fp64 log space
    with its gradient, for any frame counts and up to 8191 labels.  The workspace holds ``T (2 U + 2)`` fp64 per pair; above
    ``max_workspace_bytes`` the utterances run in groups that fit, with identical results, and MemoryError is raised, before
    anything is allocated, when one utterance's pairs alone need more.

    ``star_score``: as ``ctc_score`` (w2v2_ctc_score_grad_star).  In the gradient a star state emits the frame's top token: its
    occupancy goes to the lowest column that holds the frame's maximum, so on star frames a loss built on this sharpens the
    model's own top token in proportion to the star's occupancy and does not supervise which token.  The workspace holds one more
    fp64 and one int32 per frame."""
    import torch
    star = star_score is not None
    if star:
        from .alignment import _check_star_score
        star_score = _check_star_score(star_score)
    base, V, row0_h, frames_h, utt, labels_dev, label0, nlab_h, blank = _score_pairs(logits, labels, blank, frame_lengths, utterance, star)
    n, m = len(frames_h), len(nlab_h)
    dev = base.device
    if isinstance(coef, torch.Tensor):
        coef_dev = coef.detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    else:
        coef_dev = torch.from_numpy(np.asarray(list(coef), dtype=np.float64).reshape(-1)).to(dev)
    if coef_dev.numel() != m:
        raise ValueError(f"{m} label sequences with {coef_dev.numel()} coefficients")
    cap = int(max_workspace_bytes)
    if cap <= 0:
        raise ValueError(f"max_workspace_bytes {cap} must be positive")
    lib = N.load()
    for i in range(n):                                           # one utterance's pairs must fit on their own
        mine = np.flatnonzero(utt == i)
        if not mine.size:
            continue
        one, zero, nl = frames_h[i:i + 1].copy(), np.zeros(mine.size, np.int32), np.ascontiguousarray(nlab_h[mine])     # (alive over the call)
        workspace = lib.w2v2_ctc_score_grad_star_workspace if star else lib.w2v2_ctc_score_grad_workspace
        need = int(workspace(1, N.ptr(one), int(mine.size), N.ptr(zero), N.ptr(nl), V))
        if need < 0:
            N.check(need, "w2v2_ctc_score_grad_star_workspace" if star else "w2v2_ctc_score_grad_workspace")
        if need > cap:
            raise MemoryError(f"ctc_score_grad: utterance {i} ({int(frames_h[i])} frames, {mine.size} pairs) needs {need} bytes of "
                              f"workspace; max_workspace_bytes is {cap}")
    grad_base = torch.zeros((int(base.shape[0]), V), dtype=torch.float32, device=dev)     # (rows outside the utterances stay zero)
    logp = torch.empty(m, dtype=torch.float64, device=dev)
    if star:
        N.check(lib.w2v2_ctc_score_grad_star(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), m, N.ptr(utt), N.ptr(labels_dev),
                                             N.ptr(label0), N.ptr(nlab_h), blank, star_score, N.ptr(coef_dev), N.ptr(logp),
                                             N.ptr(grad_base), cap, N.current_stream()), "w2v2_ctc_score_grad_star")
    else:
        N.check(lib.w2v2_ctc_score_grad(N.ptr(base), V, n, N.ptr(row0_h), N.ptr(frames_h), m, N.ptr(utt), N.ptr(labels_dev),
                                        N.ptr(label0), N.ptr(nlab_h), blank, N.ptr(coef_dev), N.ptr(logp), N.ptr(grad_base), cap,
                                        N.current_stream()), "w2v2_ctc_score_grad")
    logp_h = logp.cpu().numpy()
    if isinstance(logits, torch.Tensor):
        return logp_h, grad_base.reshape(logits.shape)
    return logp_h, [grad_base[int(r):int(r) + int(t)] for r, t in zip(row0_h, frames_h)]


def rescore(logits, hypotheses, blank=0, frame_lengths=None):
    """The n-best lists of ``beam_search`` (one list of ``Hypothesis`` per utterance of ``logits``) with exact scores: ONE
    ``ctc_score`` call over every hypothesis of every utterance.  ``score`` becomes the exact CTC log-probability; ``total``
    keeps its language-model part, ``exact + (old total - old score)`` -- with a ``ContextBias`` that part holds the bonuses of the
    completed phrases and the end-of-utterance term, so biased lists need nothing else here --; a hypothesis without a beam score (NaN: the greedy
    path) gets ``score = total = exact``.  Each list is sorted again by ``total``, best first, equal totals in their old order.
    Exact scores are comparable across a list and across utterances; the beam's were lower bounds, each pruned differently."""
    lists = [list(h) for h in hypotheses]
    flat = [(i, x) for i, h in enumerate(lists) for x in h]
    if not flat:
        return lists
    exact = ctc_score(logits, [list(x.ids) for _, x in flat], blank=blank, frame_lengths=frame_lengths, utterance=[i for i, _ in flat])
    out = [[] for _ in lists]
    for (i, x), e in zip(flat, exact):
        e = float(e)
        lm = 0.0 if math.isnan(x.score) else x.total - x.score
        out[i].append(Hypothesis(x.ids, e, e + lm))
    return [sorted(h, key=lambda x: -x.total) if not any(math.isnan(x.total) for x in h) else h for h in out]


def hypothesis_posteriors(totals, scale=1.0):
    """Posterior of each hypothesis of ONE list: the fp64 softmax of ``scale * total`` (max-subtracted), a float64 numpy array.
    Meaningful on rescored lists, whose totals are exact; ``scale`` below 1 flattens the distribution (the usual acoustic scale
    of confidence estimation), 0 gives the uniform one.  An empty list gives an empty array."""
    t = np.asarray(list(totals), dtype=np.float64).reshape(-1) * np.float64(scale)
    if not t.size:
        return t
    e = np.exp(t - t.max())
    return e / e.sum()


def word_confidence(word_frames_per_hypothesis, posteriors):
    """Confidence of each word of the best hypothesis: the summed posterior of the hypotheses that hold the same word at the same
    place.  ``word_frames_per_hypothesis[k]``: the words of hypothesis k as ``(text, start, end)`` in whole frames, ``end``
    exclusive (hypothesis 0 is the best).  Hypothesis k supports the word ``(text, s, e)`` of hypothesis 0 iff it has a word of
    the same text whose frames ``[s', e')`` overlap at least half of it: ``2 (min(e, e') - max(s, s')) >= e - s``, in integers.
    Hypothesis 0 supports its own words, so every value lies in ``[posteriors[0], 1]``."""
    lists = [list(w) for w in word_frames_per_hypothesis]
    post = [float(p) for p in posteriors]
    if len(post) != len(lists):
        raise ValueError(f"{len(lists)} hypotheses with {len(post)} posteriors")
    if not lists:
        return []
    out = []
    for text, s, e in lists[0]:
        s, e = int(s), int(e)
        conf = 0.0
        for k, words in enumerate(lists):
            if k == 0 or any(t2 == text and 2 * (min(e, int(e2)) - max(s, int(s2))) >= e - s for t2, s2, e2 in words):
                conf += post[k]
        out.append(conf)
    return out


def score_transcripts(logits, hypotheses, tokenizer, blank, delimiter_id, seconds_per_frame, posterior_scale=1.0, vocab=None):
    """``ScoredTranscript`` of each utterance from its (rescored) n-best list: ONE ``forced_align`` call over every non-empty
    hypothesis of every utterance (the pairs of an utterance share its rows), then ``hypothesis_posteriors`` over each list and
    ``word_confidence`` over its word spans.  An utterance without hypotheses gets NaN and empty lists."""
    from .alignment import forced_align, token_spans, word_spans
    lists = [list(h) for h in hypotheses]
    flat = [(i, k) for i, h in enumerate(lists) for k, x in enumerate(h) if x.ids]
    spans = {}
    if flat:
        alignments = forced_align([logits[i] for i, _ in flat], [list(lists[i][k].ids) for i, k in flat], blank=blank)
        for key, a in zip(flat, alignments):
            spans[key] = token_spans(a)
    out = []
    for i, h in enumerate(lists):
        texts = [x.text(tokenizer) if tokenizer is not None else None for x in h]
        if not h:
            out.append(ScoredTranscript("", [], [], [], float("nan"), [], []))
            continue
        post = hypothesis_posteriors([x.total for x in h], posterior_scale)
        frames = [[(w.text, w.start_s, w.end_s) for w in word_spans(spans.get((i, k), []), delimiter_id, 1, vocab)] for k in range(len(h))]
        words = word_spans(spans.get((i, 0), []), delimiter_id, seconds_per_frame, vocab)
        out.append(ScoredTranscript(texts[0], h, texts, words, float(post[0]), [float(p) for p in post], word_confidence(frames, post)))
    return out
