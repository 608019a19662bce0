"""fp64 numpy reference of phrase boosting (contextual biasing) in the CTC prefix beam search (csrc/beam.hip, third part of its
header; w2v2_ctc_beam_search_biased; wav2vec2.decoding.ContextBias).  ``Definition`` computes every quantity of the bias FROM LABEL
STRINGS ALONE, by brute force over the phrase list: there is no trie, no failure link and no state number, so a bug in the host
compiler or in the kernel's state update shows as a mismatch.  ``search`` is the search of tests/beam_reference.py /
tests/wordlm_reference.py with prefixes as tuples and the bias term of a candidate taken from its prefix.

The definition.  A bias is a list of phrases; phrase h is a label string (no blank) with a boost b_h >= 0 in nats per COUNTED label
and the weight w_h = b_h * counted(h).  ``whole_words`` wraps every phrase in one leading and one trailing delimiter, which are
not counted (delimiters between the words of a phrase are), and puts one delimiter in front of the first label of every prefix.
  state(p)    the longest suffix of p that is a prefix of some phrase, proper or whole; () is the root
  C(p)        the sum of w_h over all i <= len(p) and all phrases h that p[:i] ends with: EVERY occurrence counts, overlapping and
              nested ones included (with the phrases NEW YORK and YORK, the string NEW YORK earns both)
  phi(s)      (partial * counted(s)) * max{b_h : s is a PROPER prefix of h}; 0 where there is no such h, and at the root; counted(s)
              = len(s) without the leading boundary delimiter.  partial in [0, 1]; 0 rewards completed phrases only
  B(p)        C(p) + phi(state(p))
  delta(s, c) with s' = state(s + c): ([the sum of w_h, in phrase order, over the phrases h that s + c ends with] + phi(s')) - phi(s),
              every operation fp64, the result rounded to fp32 ONCE
  final(s)    E(s) - phi(s), rounded to fp32 once; E(s) = 0 without whole_words, else the sum of w_h (in phrase order) over the phrases
              that s + delimiter ends with: the end of the utterance closes a word; credit for an unfinished phrase is given back
In the search (every product or sum one fp64 operation, in this order), with tv the character table's value (0 without a table):
  character / no table   lm(p + c) = ((lm(p) + alpha tv) + beta) + (double)delta(state(p), c)
  word model             lm(p + c) = [the lm' of the word rules of wordlm_reference, c == d and c != d alike] + (double)delta(state(p), c)
  final                  fin = lm (word model: after the open word and eos) + (double)final(state(p)); total = score + fin; the
                         final beam in descending total, equal totals by beam rank; the first nbest are returned
Keys, the -inf drop, ties, merging and bad rows are the unbiased search's.
"""

import math

import numpy as np

import beam_reference as BR
import wordlm_reference as WR

NEG = -math.inf
lse2 = BR.lse2


def f32(v):
    return float(np.float32(v))


class Definition:
    """the bias of label strings by brute force; ``phrases``: [(ids, boost)] as given to ContextBias (before any wrapping)"""

    def __init__(self, phrases, V, blank, delimiter=None, partial=1.0, whole_words=False):
        self.V, self.blank, self.delim, self.partial, self.whole = int(V), int(blank), delimiter, float(partial), bool(whole_words)
        self.lead = (int(delimiter),) if whole_words else ()
        self.phrases = [self.lead + tuple(int(c) for c in ids) + self.lead for ids, _ in phrases]
        self.boosts = [float(b) for _, b in phrases]
        self.w = [b * float(len(h) - 2 * len(self.lead)) for h, b in zip(self.phrases, self.boosts)]
        self.maxlen = max(len(h) for h in self.phrases)
        self.best = {}                                       # string -> best boost among the phrases it is a proper prefix of
        self.prefixes = set()                                # every prefix of every phrase, proper or whole
        for h, b in zip(self.phrases, self.boosts):
            for k in range(len(h) + 1):
                self.prefixes.add(h[:k])
                if k < len(h):
                    self.best[h[:k]] = max(self.best.get(h[:k], 0.0), b)
        self.by_last = {}                                    # last label -> [(phrase index, phrase)] in phrase order
        for i, h in enumerate(self.phrases):
            self.by_last.setdefault(h[-1], []).append((i, h))
        self._state, self._row, self._final = {}, {}, {}

    def ext(self, p):
        """the prefix as the bias sees it: with whole_words, behind one delimiter"""
        return self.lead + tuple(p)

    def state_of(self, s):
        """the longest suffix of the string s that is a prefix of some phrase"""
        s = tuple(s)[-self.maxlen:] if self.maxlen else ()
        got = self._state.get(s)
        if got is None:
            got = next(s[k:] for k in range(len(s) + 1) if s[k:] in self.prefixes)
            self._state[s] = got
        return got

    def state(self, p):
        return self.state_of(self.ext(p))

    def ended(self, s):
        """the sum, in phrase order, of w_h over the phrases the string s ends with"""
        acc = 0.0
        for i, h in self.by_last.get(s[-1], []) if s else []:
            if len(h) <= len(s) and s[len(s) - len(h):] == h:
                acc = acc + self.w[i]
        return acc

    def phi(self, s):
        if not s or s not in self.best:
            return 0.0
        return (self.partial * float(len(s) - len(self.lead))) * self.best[s]

    def delta(self, s, c):
        """fp32 value (as a Python float) of the transition from the state string s by the label c"""
        s2 = self.state_of(s + (c,))
        return f32((self.ended(s + (c,)) + self.phi(s2)) - self.phi(s))

    def delta_row(self, s):
        """delta(s, c) for every c as fp64 numpy (the blank's entry 0)"""
        row = self._row.get(s)
        if row is None:
            row = np.array([0.0 if c == self.blank else self.delta(s, c) for c in range(self.V)])
            self._row[s] = row
        return row

    def final(self, s):
        got = self._final.get(s)
        if got is None:
            e = self.ended(s + self.lead) if self.whole else 0.0
            got = f32(e - self.phi(s))
            self._final[s] = got
        return got

    def completed(self, p, at_end=False):
        """C(p); ``at_end``: with whole_words the end of the utterance counts as one more delimiter"""
        s = self.ext(p) + (self.lead if at_end else ())
        acc = 0.0
        for i in range(1, len(s) + 1):
            acc = acc + self.ended(s[max(0, i - self.maxlen):i])
        return acc

    def matches(self, p):
        """[(phrase index, first counted position in p, last)] of the transcript p at the end of an utterance, by last position, then
        phrase"""
        s = self.ext(p) + self.lead
        n0 = len(self.lead)
        out = []
        for i in range(1, len(s) + 1):                       # h = s[i - len(h):i]; position in p = position in s - n0
            for k, h in enumerate(self.phrases):
                if len(h) <= i and s[i - len(h):i] == h:
                    out.append((k, (i - len(h) + n0) - n0, (i - 1 - n0) - n0))
        return out


class WordRules:
    """the word model's term of a candidate, from the prefix alone (the rules of wordlm_reference, which scores a whole prefix; here
    the increment, because the bias terms are added in between): ``step(p, l, c)`` = the lm' of p + c given lm(p) = l, None = dropped"""

    def __init__(self, lm):
        self.sc = WR.Scorer(lm)
        self.d = lm.delimiter
        self._allowed = {}

    def _split(self, p):
        parts = bytes(p).split(self.sc.d)
        return tuple(x for x in parts[:-1] if x), parts[-1]

    def allowed(self, p):
        """constrained mode: the labels (other than the delimiter) that keep the open word inside the lexicon; None = all"""
        if not self.sc.constrained:
            return None
        tail = self._split(p)[1]
        if tail not in self._allowed:
            self._allowed[tail] = {c for c in range(self.sc.lm.vocab_size) if tail + bytes([c]) in self.sc.open}
        return self._allowed[tail]

    def end_word(self, p, l):
        """(lm', history) after the open word of p is ended; None = dropped"""
        sc = self.sc
        done, tail = self._split(p)
        got = sc.words(done)
        if got is None:
            return None
        hist = got[1]
        if not tail:
            return l, hist
        w = sc.word_of.get(tail)
        if w is None:
            if sc.constrained:
                return None
            v = sc.lookup(hist, WR.UNK) + sc.pen
            w = WR.UNK
        else:
            v = sc.lookup(hist, w)
        return (l + sc.alpha * v) + sc.beta, hist + (w,)

    def finish(self, p, l):
        got = self.end_word(p, l)
        if got is None:
            return None
        fin, hist = got
        if self.sc.eos:
            fin = fin + self.sc.alpha * self.sc.lookup(hist, WR.EOS)
        return fin


def search(x, beam_width, nbest, blank, bias, lm=None, rules=None):
    """``bias``: a Definition; ``lm``: None, a CharNgramLM or a WordNgramLM (``rules``: its WordRules, to share the caches).  Returns
    what beam_reference.search returns; the margin includes the gaps between the final totals, kmax the final totals;
    ``before_final``: the final beam's (prefix, score + lm) in beam order, before the end-of-utterance terms"""
    from wav2vec2.decoding import WordNgramLM
    x = np.asarray(x, np.float32)
    T, V = x.shape
    lp, lse = BR.log_probs(x)
    if not np.isfinite(lse).all():
        return BR.Result([], math.inf, 0.0, bad=True)
    word = isinstance(lm, WordNgramLM)
    if word:
        rules = rules or WordRules(lm)
        d = lm.delimiter
    table, order, alpha, beta = None, 1, 0.0, 0.0
    if lm is not None and not word:
        table, order = lm.table.astype(np.float64).reshape(-1, V), lm.order
        alpha, beta = float(np.float32(lm.alpha)), float(np.float32(lm.beta))
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
                dl = bias.delta_row(bias.state(p))
                if word:
                    base = np.full(V, l)
                    ok = rules.allowed(p)
                    if ok is not None:
                        base[[c for c in range(V) if c not in ok]] = NEG
                    got = rules.end_word(p, l)
                    base[d] = NEG if got is None else got[0]
                else:
                    tv = 0.0 if table is None else table[BR.lm_context(p, V, blank, order)]
                    base = (l + alpha * tv) + beta
                LM[j] = base + dl
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
        f = rules.finish(p, l) if word else l
        if f is not None:
            s = lse2(pb, pnb)
            fin.append((p, s, s + (f + bias.final(bias.state(p))), r))
    fin.sort(key=lambda z: (-z[2], z[3]))
    for a, b in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[2] - b[2])
    for z in fin[:nbest]:
        kmax = max(kmax, abs(z[2]))
    res = BR.Result([z[:3] for z in fin[:nbest]], margin, kmax)
    res.before_final = [(p, lse2(pb, pnb) + l) for p, pb, pnb, l in beam]
    return res


# ---- seeded biases and logits, shared by the CPU and the GPU tests ------------------------------------------------------------------
def make_bias(phrases, V, blank, delimiter=None, partial=1.0, whole_words=False):
    """(ContextBias, Definition) of the same phrase list [(ids, boost)]"""
    from wav2vec2.decoding import ContextBias
    return (ContextBias(phrases, V, blank, delimiter, partial, whole_words), Definition(phrases, V, blank, delimiter, partial, whole_words))


def random_phrases(rng, V, blank, delim, n, maxlen=6, words=False):
    """about n distinct random phrases of 1..maxlen labels with boosts that are multiples of 0.25 in [0.25, 3]; ``words``: no
    delimiter at either end and no doubled one (phrases of words); among them a one-label phrase, a doubled label, a phrase nested
    in another and one whose suffix is another's prefix"""
    letters = [c for c in range(V) if c not in (blank, delim)]
    a, b, c = (int(v) for v in rng.choice(letters, 3, replace=False)) if len(letters) >= 3 else (letters * 3)[:3]
    out = {(a,): 0, (a, b, b, a): 0, (b, b): 0, (c, a, b): 0, (a, b, c, c): 0}
    tries = 0
    while len(out) < n and tries < 20 * n:
        tries += 1
        k = int(rng.integers(1, maxlen + 1))
        h = [int(v) for v in rng.choice(letters, k)]
        if words and k >= 3 and rng.random() < 0.3:
            h[int(rng.integers(1, k - 1))] = delim
        out.setdefault(tuple(h), 0)
    return [(h, 0.25 * int(rng.integers(1, 13))) for h in out]


def phrase_logits(rng, bias, V, blank, nphrases, cut=0):
    """frames that spell `nphrases` phrases of the Definition `bias` (as wrapped) with noise: each label on 1-3 frames, blanks between;
    `cut` frames taken off the end"""
    seq = []
    for _ in range(nphrases):
        h = bias.phrases[int(rng.integers(len(bias.phrases)))]
        for c in h:
            if seq and seq[-1] == c:
                seq.append(blank)
            seq += [c] * int(rng.integers(1, 4)) + [blank] * int(rng.integers(0, 3))
    seq = seq[:len(seq) - cut] if cut else seq
    T = len(seq)
    x = rng.standard_normal((T, V)).astype(np.float32) * 1.5
    x[np.arange(T), seq] += rng.uniform(1, 5, T).astype(np.float32)
    return x


# (V, blank, delim, lexicon words, word model order) as wordlm_reference.CASES; forms: no LM, character 3-gram, word model open / constrained
VOCABS = [(6, 0, 1, 12, 2), (32, 31, 4, 200, 3), (64, 0, 5, 500, 3)]
FORMS = ["none", "char3", "word", "word_constrained"]
# (beam width, nbest, frame counts of the flat and of the peaky utterances); two phrase-spelling utterances are added to each
SETS = [(1, 1, [1, 5, 40, 120]), (4, 4, [5, 40]), (16, 8, [1, 5, 40, 120]), (16, 1, [40]), (64, 8, [1, 5, 40]), (64, 4, [5])]
SIZES = [8, 2000]


def case_inputs(vocab, form, size):
    """(lm, ContextBias, Definition, [(W, nbest, [logits])]) of one case, seeded"""
    from wav2vec2.decoding import CharNgramLM
    V, blank, delim, nwords, order = vocab
    rng = np.random.default_rng(7000 + 100 * V + 10 * FORMS.index(form) + (size > 100))
    lm = None
    if form == "char3":
        lm = CharNgramLM(np.log(rng.dirichlet(np.ones(V), V ** 2)).astype(np.float32), 3, alpha=0.8, beta=-0.2)
    elif form != "none":
        lm = WR.random_model(rng, V, blank, delim, nwords, order, alpha=0.8, beta=0.3,
                             unk_penalty=NEG if form == "word_constrained" else -2.0)
    whole = form in ("word", "char3")
    phrases = random_phrases(rng, V, blank, delim, size, maxlen=6 if V > 6 else 7, words=whole)
    if lm is not None and form.startswith("word"):           # half of the phrases made of lexicon words, so that they survive the lexicon
        sp = sorted(lm.lexicon.values())
        for k in range(0, len(phrases), 2):
            ws = [sp[int(i)] for i in rng.integers(len(sp), size=int(rng.integers(1, 3)))]
            ids = ws[0] + tuple(c for w in ws[1:] for c in (delim,) + w)
            phrases[k] = (ids, phrases[k][1])
        phrases = list({h: b for h, b in phrases}.items())
    cb, df = make_bias(phrases, V, blank, delim, partial=1.0 if size == 8 else 0.5, whole_words=whole)
    sets = []
    for W, nbest, Ts in SETS:
        xs = [WR.make_logits(rng, T, V, blank, pk) for T in Ts for pk in (False, True)]
        xs += [phrase_logits(rng, df, V, blank, k) for k in (2, 5)]
        sets.append((W, nbest, xs))
    return lm, cb, df, sets


# ---- worked examples: labels 0 blank, 1 delimiter, 2 = a, 3 = n, 4 = o, 5 = x ---------------------------------------------------------
ANNA = (2, 3, 3, 2)


def frames(rows, V=6):
    """log of per-frame probabilities: `rows[t]` = {label: probability}; every other entry a small value of its own (no exact ties)"""
    p = np.empty((len(rows), V))
    for t in range(len(rows)):
        for c in range(V):
            p[t, c] = 0.01 * (1.0 + 0.07 * c + 0.013 * t)
    for t, r in enumerate(rows):
        for c, v in r.items():
            p[t, c] = v
    return np.log(p).astype(np.float32)


def pick_logits():
    """a, n, (n | blank), n, a, blank: `ana` beats `anna`, whose second n needs the weaker blank of the third frame"""
    return frames([{2: .95}, {3: .95}, {0: .30, 3: .66}, {3: .95}, {2: .95}, {0: .95}])


def cut_logits():
    """a, then x a little better than n: the utterance ends inside `anna`"""
    return frames([{2: .95}, {3: .3, 5: .6, 0: .05}])


def nested_logits():
    """spells `annao`: with the phrases anna, nn and nao, all three occur (nested and overlapping)"""
    return frames([{2: .9}, {3: .9}, {0: .9}, {3: .9}, {2: .9}, {4: .9}])


def lookahead_logits():
    """a, then x, o and n in that order of probability, then blank, n, a: at width 2 the prefix `an` survives the second frame only
    with credit in advance"""
    return frames([{2: .95}, {3: .2, 5: .5, 4: .25, 0: .03}, {0: .9}, {3: .9}, {2: .9}, {0: .9}])
