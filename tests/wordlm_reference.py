"""fp64 numpy reference of the CTC prefix beam search with a word n-gram language model and a lexicon (csrc/beam.hip, second part of
its header; w2v2_ctc_beam_search_words): the search of tests/beam_reference.py with prefixes as tuples, and a candidate's language
model term computed FROM THE PREFIX ALONE: the prefix is split at the delimiter, every word is looked up by its spelling, and
log P(word | history) walks the n-gram DICTIONARY (``lm.logp`` / ``lm.backoff``, keyed by tuples of word strings) with the backoff
recursion, the weights added in the kernel's order.  Neither the compiled state machine nor any per-entry state is used, so a bug
in the compiler or in the kernel's state update shows as a mismatch.  (``Scorer`` keeps a cache of the score of a word SEQUENCE: a
pure function's values, computed from scratch on first use.)

    lookup(history, w): acc = 0; h = the last order - 1 words; (h, w) an n-gram: acc + logp; else acc = acc + backoff(h) (0 where h
                        has none), h = h without its oldest word, again.
    a word ends       : lm' = (lm + alpha lookup(history, word)) + beta;  no word of the lexicon: the same with <unk> and
                        lookup + unk_penalty -- or, unk_penalty = -inf (constrained), the prefix is dropped: as soon as its open word
                        is no prefix of a lexicon word, or at the delimiter where it is no whole word.
    final             : the open word ended as above (dropped where that drops it), + alpha lookup(history, </s>) with score_eos
                        where the model has </s>; total = score + that; descending total, equal totals by beam rank.
``search`` returns what beam_reference.search returns; the margin includes the gaps between the final totals (up to the first
hypothesis not returned), kmax the final totals."""

import itertools
import math

import numpy as np

import beam_reference as BR

NEG = -math.inf
lse2 = BR.lse2
BOS, EOS, UNK = "<s>", "</s>", "<unk>"


class Scorer:
    """the language model term of a label prefix, from the prefix alone; None = dropped"""

    def __init__(self, lm):
        self.lm = lm
        self.d = bytes([lm.delimiter])
        self.word_of = {bytes(ids): w for w, ids in lm.lexicon.items()}
        self.open = {bytes(ids[:k]) for ids in lm.lexicon.values() for k in range(len(ids) + 1)}
        self.alpha, self.beta = float(np.float32(lm.alpha)), float(np.float32(lm.beta))
        self.constrained = lm.unk_penalty == NEG
        self.pen = 0.0 if self.constrained else float(np.float32(lm.unk_penalty))
        self.eos = lm.score_eos and (EOS,) in lm.logp
        self.start = (BOS,) if (BOS,) in lm.logp else ()
        self.cache = {}

    def lookup(self, hist, w):
        lm = self.lm
        h = tuple(hist[-(lm.order - 1):]) if lm.order > 1 else ()
        acc = 0.0
        while True:
            g = h + (w,)
            if g in lm.logp:
                return acc + lm.logp[g]
            acc = acc + lm.backoff.get(h, 0.0)
            h = h[1:]

    def words(self, spelled):
        """(lm, history) after the complete words `spelled` (a tuple of byte strings), from scratch; None = dropped"""
        got = self.cache.get(spelled, 0)
        if got != 0:
            return got
        l, hist = 0.0, list(self.start)
        for b in spelled:
            w = self.word_of.get(b)
            if w is None:
                if self.constrained:
                    l = None
                    break
                v = self.lookup(hist, UNK) + self.pen
                w = UNK
            else:
                v = self.lookup(hist, w)
            l = (l + self.alpha * v) + self.beta
            hist.append(w)
        got = None if l is None else (l, tuple(hist))
        self.cache[spelled] = got
        return got

    def score(self, prefix, final=False):
        parts = bytes(prefix).split(self.d)
        tail = parts[-1]
        if final and tail:
            parts.append(b"")
            tail = b""
        got = self.words(tuple(p for p in parts[:-1] if p))
        if got is None or (self.constrained and tail not in self.open):
            return None
        l, hist = got
        if final and self.eos:
            l = l + self.alpha * self.lookup(hist, EOS)
        return l


def search(x, beam_width, nbest, blank, lm, scorer=None):
    x = np.asarray(x, np.float32)
    T, V = x.shape
    lp, lse = BR.log_probs(x)
    if not np.isfinite(lse).all():
        return BR.Result([], math.inf, 0.0, bad=True)
    sc = scorer or Scorer(lm)
    W = int(beam_width)
    beam = [((), 0.0, NEG, 0.0)]
    margin, kmax = math.inf, 0.0
    cols = np.arange(V)
    for t in range(T):
        row = lp[t]
        nb = len(beam)
        rank = {e[0]: j for j, e in enumerate(beam)}
        tots = [lse2(e[1], e[2]) for e in beam]
        PB = np.full((nb, V), NEG)
        PNB = np.full((nb, V), NEG)
        LM = np.full((nb, V), NEG)
        with np.errstate(invalid="ignore"):
            for j, (p, pb, pnb, l) in enumerate(beam):
                last = p[-1] if p else -1
                PNB[j] = np.where(cols == last, pb, tots[j]) + row
                for c in range(V):
                    if c != blank:
                        v = sc.score(p + (c,))
                        LM[j, c] = NEG if v is None else v
                PB[j, blank] = tots[j] + row[blank]
                PNB[j, blank] = pnb + row[last] if p else NEG
                LM[j, blank] = l
        for q, (p, pb, pnb, l) in enumerate(beam):
            i = rank.get(p[:-1]) if p else None
            if i is not None:
                PNB[q, blank] = lse2(PNB[q, blank], PNB[i, p[-1]])
                PNB[i, p[-1]] = NEG
        key = np.full(nb * V, NEG)
        for j in range(nb):
            key[j * V + blank] = lse2(PB[j, blank], PNB[j, blank]) + LM[j, blank]
        ext = np.ones((nb, V), bool)
        ext[:, blank] = False
        flat = ext.ravel()
        kk = PNB.ravel() + LM.ravel()                        # (-inf + -inf = -inf; no +inf occurs)
        key[flat] = kk[flat]
        key = key + 0.0
        order_ = np.argsort(-key, kind="stable")
        nvalid = int((key > NEG).sum())
        keep = order_[:min(W, nvalid)]
        if nvalid > W:
            margin = min(margin, float(key[order_[W - 1]] - key[order_[W]]))
        if nvalid:
            kmax = max(kmax, abs(float(key[keep[0]])), abs(float(key[keep[-1]])))
        nxt = []
        for idx in keep:
            j, c = divmod(int(idx), V)
            p = beam[j][0] if c == blank else beam[j][0] + (c,)
            nxt.append((p, float(PB[j, c]), float(PNB[j, c]), float(LM[j, c])))
        beam = nxt
    fin = []
    for r, (p, pb, pnb, l) in enumerate(beam):
        f = sc.score(p, final=True)
        if f is not None:
            s = lse2(pb, pnb)
            fin.append((p, s, s + f, r))
    fin.sort(key=lambda z: (-z[2], z[3]))
    for a, b in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[2] - b[2])
    for z in fin[:nbest]:
        kmax = max(kmax, abs(z[2]))
    res = BR.Result([z[:3] for z in fin[:nbest]], margin, kmax)
    res.final_beam = len(beam)
    return res


def brute_force(x, blank, lm):
    """every one of the V^T frame paths collapsed by the CTC rule, every transcript scored from scratch: [(labels, score, total)] by
    descending total; transcripts the model drops are left out"""
    lp, _ = BR.log_probs(x)
    T, V = lp.shape
    sc = Scorer(lm)
    d = {}
    for path in itertools.product(range(V), repeat=T):
        s = 0.0
        for t, c in enumerate(path):
            s += lp[t, c]
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        k = tuple(out)
        d[k] = lse2(d.get(k, NEG), s)
    res = []
    for k, s in d.items():
        f = sc.score(k, final=True)
        if f is not None:
            res.append((k, s, s + f))
    res.sort(key=lambda z: -z[2])
    return res


# ---- seeded models and logits, shared by the CPU and the GPU tests ------------------------------------------------------------------
def random_model(rng, V, blank, delim, nwords, order, maxlen=4, bos=True, eos=True, **kw):
    """a random backoff model over `nwords` random spellings of 1..maxlen letters (not normalised: the search does not need it),
    every n-gram's context an n-gram, about half of the contexts extended by 3 words; values in log10 as in an ARPA file"""
    from wav2vec2.decoding import WordNgramLM
    letters = [c for c in range(V) if c not in (blank, delim)]
    spell = set()
    while len(spell) < nwords:
        spell.add(tuple(int(v) for v in rng.choice(letters, int(rng.integers(1, maxlen + 1)))))
    lexicon = {f"w{i:04d}": s for i, s in enumerate(sorted(spell))}
    pred = sorted(lexicon) + [UNK] + ([EOS] if eos else [])
    ngrams, backoffs = {}, {}
    p = np.log10(rng.dirichlet(np.ones(len(pred))))
    for w, v in zip(pred, p):
        ngrams[(w,)] = float(v)
        if w != EOS:
            backoffs[(w,)] = float(-rng.uniform(0.05, 0.9))
    if bos:
        ngrams[(BOS,)] = -99.0
        backoffs[(BOS,)] = float(-rng.uniform(0.05, 0.9))
    prev = [g for g in ngrams if g[0] != EOS]
    for n in range(2, order + 1):
        cur = []
        for h in sorted(prev):
            if rng.random() < 0.5:
                for i in rng.choice(len(pred), 3, replace=False):
                    g = h + (pred[int(i)],)
                    ngrams[g] = float(-rng.uniform(0.05, 2.6))
                    if n < order and g[-1] != EOS:
                        if rng.random() < 0.8:
                            backoffs[g] = float(-rng.uniform(0.05, 0.9))
                        cur.append(g)
        prev = cur
    return WordNgramLM(ngrams, backoffs, lexicon, V, delim, **kw)


def make_logits(rng, T, V, blank, peaky):
    x = rng.standard_normal((T, V)).astype(np.float32)
    if peaky:                                                # a target per frame (runs of 3) raised by 2-8, half of them the blank
        tgt = np.repeat(rng.integers(0, V, T // 3 + 1), 3)[:T]
        tgt[rng.random(T) < 0.5] = blank
        x[np.arange(T), tgt] += rng.uniform(2, 8, T).astype(np.float32)
    return x


def word_logits(rng, lm, nwords, blank, cut=0):
    """frames that spell `nwords` lexicon words with noise: each label on 1-3 frames, blanks between; `cut` frames taken off the end
    (so that the utterance ends inside a word)"""
    spellings = sorted(lm.lexicon.values())
    seq = []
    for _ in range(nwords):
        for c in spellings[int(rng.integers(len(spellings)))]:
            seq += [c] * int(rng.integers(1, 4)) + [blank] * int(rng.integers(0, 3))
        seq += [lm.delimiter] * int(rng.integers(1, 3)) + [blank] * int(rng.integers(0, 2))
    seq = seq[:len(seq) - cut] if cut else seq
    T = len(seq)
    x = rng.standard_normal((T, lm.vocab_size)).astype(np.float32) * 1.5
    x[np.arange(T), seq] += rng.uniform(1, 5, T).astype(np.float32)
    return x


# (V, blank, delim, lexicon words, order): V in {6, 32, 64}, orders 1-3 and one 5-gram; each case open (unk_penalty -2) and constrained
CASES = [(6, 0, 1, 12, 2), (32, 0, 4, 200, 3), (32, 31, 4, 200, 1), (64, 0, 5, 500, 3), (32, 0, 4, 100, 5)]
# (beam width, nbest, frame counts of the flat and of the peaky utterances); two word-spelling utterances are added to each
SETS = [(1, 1, [1, 2, 50, 120]), (4, 1, [7, 60]), (4, 4, [3, 90]), (16, 8, [1, 2, 33, 100]), (16, 1, [64]), (64, 8, [1, 3, 40]), (64, 1, [25])]


def case_inputs(V, blank, delim, nwords, order, constrained):
    rng = np.random.default_rng(1000 * V + 10 * order + blank + (5 if constrained else 0))
    lm = random_model(rng, V, blank, delim, nwords, order, alpha=0.8, beta=0.3 if order % 2 else -0.2,
                      unk_penalty=NEG if constrained else -2.0)
    sets = []
    for W, nbest, Ts in SETS:
        xs = [make_logits(rng, T, V, blank, pk) for T in Ts for pk in (False, True)]
        xs += [word_logits(rng, lm, k, blank) for k in (2, 6)]
        sets.append((W, nbest, xs))
    return lm, sets


# ---- a worked example ----------------------------------------------------------------------------------------------------------------
def two_word_model(**kw):
    """labels: 0 blank, 1 the delimiter, 2 = a, 3 = b; the words `ab` and `ba`"""
    from wav2vec2.decoding import WordNgramLM
    ngrams = {("<unk>",): -2.0, ("ab",): -0.3, ("ba",): -0.5, ("</s>",): -0.6, ("ab", "ba"): -0.1}
    return WordNgramLM(ngrams, {("ab",): -0.2, ("ba",): -0.3}, {"ab": (2, 3), "ba": (3, 2)}, 4, 1, **kw)


def pick_logits():
    """frames a, a|b, blank, delimiter, b, a: acoustically `aa b...` beats `ab`; the second frame prefers a by a little"""
    p = np.full((6, 4), 0.02)
    for t, c in enumerate([2, 2, 0, 1, 3, 2]):
        p[t, c] = 0.94
    p[1] = [0.02, 0.02, 0.55, 0.41]
    return np.log(p).astype(np.float32)
