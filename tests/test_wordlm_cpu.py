"""The word n-gram language model and its lexicon without a GPU: the fp64 reference search (tests/wordlm_reference.py) against a
brute-force enumeration of all V^T frame paths, the ARPA reader, the compiler against the dictionary recursion, from_text's
normalisation, the to_arpa round trip, the lexicon trie, a worked example, every ValueError -- and, from the reference alone, the
share of fragile utterances among the inputs of tests/test_wordlm_gpu.py."""

import math
import os

import numpy as np
import pytest

import beam_reference as BR
import wordlm_reference as WR
from wav2vec2.decoding import CharNgramLM, WordNgramLM, _check_args
from wav2vec2.processor import Wav2Vec2Processor

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab.json")
NEG = -math.inf
LN10 = math.log(10.0)

# a hand-written model: 3-gram, <s> and </s>, no <unk> (added by unk_logp), a bigram without backoff weight
ARPA = """
\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-0.6 THE -0.4
-0.7 CAT -0.3
-0.9 SAT -0.2

\\2-grams:
-0.2 <s> THE -0.1
-0.3 THE CAT -0.25
-0.4 CAT SAT
-0.5 SAT </s>

\\3-grams:
-0.05 <s> THE CAT
-0.15 THE CAT SAT

\\end\\
"""


def tok():
    return Wav2Vec2Processor(is_tokenizer=True, vocab_path=VOCAB)


def f32ln(x):
    return float(np.float32(np.float64(x) * np.float64(LN10)))


# ---- the reference against brute force --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("constrained", [False, True])
def test_reference_equals_brute_force(order, constrained):
    """V = 4 (blank, delimiter, two letters), T = 1 .. 6, a beam wide enough that nothing is pruned: every transcript, total and rank"""
    rng = np.random.default_rng(100 + 10 * order + constrained)
    for trial in range(4):
        lm = WR.random_model(rng, 4, 0, 1, 4, order, maxlen=3, bos=trial % 2 == 0, eos=trial < 3, alpha=0.7, beta=0.25,
                             unk_penalty=NEG if constrained else -0.8)
        for T in (1, 2, 3, 4, 5, 6):
            x = WR.make_logits(rng, T, 4, 0, trial % 2 == 1)
            want = WR.brute_force(x, 0, lm)
            got = WR.search(x, 4096, 4096, 0, lm).hyps
            assert [k for k, _, _ in got] == [k for k, _, _ in want]
            for (_, s, tot), (_, s2, tot2) in zip(got, want):
                assert abs(s - s2) <= 1e-12 and abs(tot - tot2) <= 1e-12
            if not constrained:
                assert len(got) == len({k for k in want})
            assert len(want) >= 1


def test_pruning_reference_keeps_the_best_prefixes():
    """at width 3 the reference's hypotheses are transcripts of the brute force with scores that do not exceed the exact ones"""
    rng = np.random.default_rng(3)
    lm = WR.random_model(rng, 4, 0, 1, 4, 2, maxlen=3, alpha=0.7, beta=0.25, unk_penalty=-0.8)
    for _ in range(5):
        x = WR.make_logits(rng, 6, 4, 0, True)
        exact = {k: (s, tot) for k, s, tot in WR.brute_force(x, 0, lm)}
        for k, s, tot in WR.search(x, 3, 3, 0, lm).hyps:
            assert s <= exact[k][0] + 1e-12 and abs((tot - s) - (exact[k][1] - exact[k][0])) <= 1e-12


# ---- the ARPA reader and the compiler --------------------------------------------------------------------------------------------------
def test_arpa_reader_hand_computed():
    lm = WordNgramLM.from_arpa(ARPA, tok(), unk_logp=-2.5)
    assert lm.order == 3 and lm.words == ["</s>", "<unk>", "CAT", "SAT", "THE"] and lm.skipped == 0
    assert lm.ngrams[("<unk>",)] == -2.5 and lm.backoffs[("THE", "CAT")] == -0.25 and ("CAT", "SAT") not in lm.backoffs
    assert lm.states[0] == () and lm.states[lm.start_state] == ("<s>",)
    wid, sid = lm.word_id, {h: i for i, h in enumerate(lm.states)}
    # a trigram hit
    assert lm.lookup(sid[("<s>", "THE")], wid["CAT"]) == (f32ln(-0.05), sid[("THE", "CAT")])
    # one backoff: (THE CAT) THE -> bo(THE CAT) + miss in (CAT) -> bo(CAT) + P(THE)
    v, s = lm.lookup(sid[("THE", "CAT")], wid["THE"])
    assert v == (0.0 + f32ln(-0.25)) + f32ln(-0.3) + f32ln(-0.6) and s == sid[("THE",)]
    # (CAT SAT) has no backoff weight (0) and is a state (it is an n-gram below the top order)
    v, s = lm.lookup(sid[("CAT", "SAT")], wid["</s>"])
    assert v == 0.0 + f32ln(-0.5) and lm.bo[sid[("CAT", "SAT")]] == 0.0
    # the start: <s> CAT -> bo(<s>) + P(CAT); the next state is (CAT), the longest suffix that is a state
    v, s = lm.lookup(lm.start_state, wid["CAT"])
    assert v == f32ln(-0.5) + f32ln(-0.7) and s == sid[("CAT",)]
    # <unk> from a bigram state: all the way down; the next state is the context <unk> (a unigram is a state below order 2 .. 3)
    v, s = lm.lookup(sid[("THE", "CAT")], lm.unk)
    assert v == (f32ln(-0.25) + f32ln(-0.3)) + f32ln(-2.5) and s == sid[("<unk>",)] and lm.bo[s] == 0.0
    assert lm.eos == wid["</s>"] and lm.bstate[sid[("THE", "CAT")]] == sid[("CAT",)] and lm.bstate[sid[("CAT",)]] == 0
    # a file is read as the text is
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.arpa")
        with open(path, "w") as f:
            f.write(ARPA)
        lm2 = WordNgramLM.from_arpa(path, tok(), unk_logp=-2.5)
    assert lm2.ngrams == lm.ngrams and lm2.backoffs == lm.backoffs


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_compiled_lookup_equals_dictionary_recursion(order):
    """every (history, word) of a random model: every history of up to order - 1 words that is a state, plus random longer and
    unseen histories walked word by word through the state machine"""
    rng = np.random.default_rng(40 + order)
    lm = WR.random_model(rng, 32, 0, 4, 30, order, bos=order != 2, unk_penalty=-1.0)
    sc = WR.Scorer(lm)
    for s, h in enumerate(lm.states):
        for w, i in lm.word_id.items():
            v, nxt = lm.lookup(s, i)
            assert v == sc.lookup(list(h), w)
            want = (h + (w,))[-(order - 1):] if order > 1 else ()
            while want not in lm.states:
                want = want[1:]
            assert lm.states[nxt] == want
    pred = [w for w in lm.words if w != "</s>"]
    for _ in range(300):
        s, hist = lm.start_state, list(sc.start)
        for _ in range(7):
            lo, hi = int(lm.arc0[s]), int(lm.arc0[s + 1])
            seen = [lm.words[k] for k in lm.arc_word[lo:hi] if lm.words[k] != "</s>"]
            w = seen[int(rng.integers(len(seen)))] if s and seen and rng.random() < 0.7 else pred[int(rng.integers(len(pred)))]
            v, s = lm.lookup(s, lm.word_id[w])
            assert v == sc.lookup(hist, w)
            hist.append(w)
    lm.validate()


def test_from_text_is_normalised():
    texts = ["the cat sat on the mat", "the dog sat", "a cat and a dog", "the cat sat on a dog", "on the mat the cat sat"]
    for order in (1, 2, 3, 4):
        lm = WordNgramLM.from_text(texts, tok(), order)
        assert lm.order == order and "<unk>" in lm.word_id and lm.eos >= 0
        for s, h in enumerate(lm.states):
            total = sum(math.exp(lm.lookup(s, w)[0]) for w in range(len(lm.words)))
            assert abs(total - 1.0) < 2e-6 * len(lm.words), (h, total)
        # a seen n-gram is more probable than an unseen one in the same context
        sid = {h: i for i, h in enumerate(lm.states)}
        if order >= 2:
            assert lm.lookup(sid[("THE",)], lm.word_id["CAT"])[0] > lm.lookup(sid[("THE",)], lm.word_id["AND"])[0]
    ng, bo = WordNgramLM.count_ngrams([["A", "B"], ["A"]], 2, discount=0.5)
    # c(A) = 2, c(B) = 1, c(</s>) = 2: 5 tokens, 3 types; <unk> gets 0.5 * 3 / 5
    assert abs(10 ** ng[("A",)] - 1.5 / 5) < 1e-12 and abs(10 ** ng[("<unk>",)] - 0.3) < 1e-12
    # context A: B once, </s> once -> (1 - 0.5) / 2 each, left 0.5; bo = 0.5 / (1 - P(B) - P(</s>))
    assert abs(10 ** ng[("A", "B")] - 0.25) < 1e-12 and abs(10 ** bo[("A",)] - 0.5 / (1 - 0.5 / 5 - 1.5 / 5)) < 1e-12


def test_to_arpa_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    t = tok()
    a = WordNgramLM.from_text(["the quick brown fox", "jumps over the lazy dog", "the dog jumps"], t, 3, alpha=0.4, beta=0.1)
    path = tmp_path / "lm.arpa"
    text = a.to_arpa(path)
    assert path.read_text() == text and text.startswith("\\data\\\nngram 1=") and text.rstrip().endswith("\\end\\")
    for b in (WordNgramLM.from_arpa(str(path), t), WordNgramLM.from_arpa(text, t)):
        assert b.ngrams == a.ngrams and b.backoffs == a.backoffs and b.lexicon == a.lexicon and b.states == a.states
        for k in ("arc0", "arc_word", "arc_logp", "arc_next", "bo", "bstate", "child", "word_at"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
    # a random (unnormalised) model with and without <s> / </s>
    for bos, eos in ((True, True), (False, False)):
        m = WR.random_model(rng, 32, 0, 4, 20, 3, bos=bos, eos=eos)
        ng, bo = WordNgramLM.read_arpa(m.to_arpa())
        assert ng == m.ngrams and bo == m.backoffs


def test_lexicon_trie():
    t = tok()
    v = t.get_vocab()
    lm = WordNgramLM.from_arpa(ARPA, t, unk_logp=-2.5)
    T, H, E, C, A, S = (v[c] for c in "THECAS")
    assert lm.vocab_size == 32 and lm.delimiter == v["|"] == 4
    assert lm.lexicon == {"THE": (T, H, E), "CAT": (C, A, T), "SAT": (S, A, T)}
    assert lm.child.shape == (10, 32) and lm.child.dtype == np.int32 and (lm.child >= 0).sum() == 9
    for w, ids in lm.lexicon.items():
        node = 0
        for c in ids:
            assert lm.word_at[node] == -1
            node = lm.child[node, c]
            assert node > 0
        assert lm.word_at[node] == lm.word_id[w]
    assert (lm.word_at >= 0).sum() == 3 and lm.child[0, H] == -1 and not lm.uses_label(v["<pad>"]) and lm.uses_label(A)
    # words the tokenizer cannot spell are skipped and counted; an explicit word list; an explicit spelling
    arpa = ARPA.replace("ngram 1=5", "ngram 1=7").replace("-0.9 SAT -0.2", "-0.9 SAT -0.2\n-1.5 C3PO\n-1.6 cat")
    lm = WordNgramLM.from_arpa(arpa, t, unk_logp=-2.5)
    assert lm.skipped == 2 and sorted(lm.lexicon) == ["CAT", "SAT", "THE"] and "C3PO" in lm.word_id      # (cat is spelled as CAT)
    lm = WordNgramLM.from_arpa(ARPA, t, unk_logp=-2.5, lexicon=["CAT", "THE"])
    assert sorted(lm.lexicon) == ["CAT", "THE"]
    lm = WordNgramLM.from_arpa(ARPA, t, unk_logp=-2.5, lexicon={"CAT": (C, A, T, T)})
    assert lm.lexicon == {"CAT": (C, A, T, T)} and lm.word_at[lm.child[lm.child[lm.child[lm.child[0, C], A], T], T]] == lm.word_id["CAT"]


# ---- a worked example -------------------------------------------------------------------------------------------------------------------
def test_lm_picks_the_word():
    """labels 0 blank, 1 delimiter, 2 = a, 3 = b; words ab, ba.  Acoustically `a|ba` wins (a is no word); the model picks `ab|ba`."""
    x = WR.pick_logits()
    assert BR.search(x, 16, 1).hyps[0][0] == (2, 1, 3, 2)
    assert BR.brute_force(x)[0][0] == (2, 1, 3, 2)
    for pen in (-3.0, NEG):
        lm = WR.two_word_model(unk_penalty=pen)
        ref = WR.search(x, 16, 2, 0, lm)
        assert ref.hyps[0][0] == (2, 3, 1, 3, 2) == WR.brute_force(x, 0, lm)[0][0]
        assert ref.margin > 1e-3
    # the total by hand: score + [ln P(ab) + bo(ab)... no: (ab, ba) is a bigram] + ln P(ba | ab) + ln P(</s> | ba)
    lm = WR.two_word_model(unk_penalty=NEG, alpha=1.0, beta=0.0)
    k, s, tot = WR.search(x, 16, 1, 0, lm).hyps[0]
    want = (f32ln(-0.3) + f32ln(-0.1)) + (f32ln(-0.3) + f32ln(-0.6))          # ... and </s> after ba: bo(ba) + P(</s>)
    assert abs((tot - s) - want) < 1e-12
    # an utterance that ends inside a word: one frame of `a`; constrained: nothing is left at width 1
    y = np.log(np.array([[0.01, 0.01, 0.97, 0.01]])).astype(np.float32)
    assert WR.search(y, 1, 1, 0, lm).hyps == []
    assert [k for k, _, _ in WR.search(y, 2, 2, 0, lm).hyps] == [()]
    open_lm = WR.two_word_model(unk_penalty=-1.0, alpha=1.0, beta=0.5)
    k, s, tot = WR.search(y, 1, 1, 0, open_lm).hyps[0]
    assert k == (2,) and abs((tot - s) - (((f32ln(-2.0) + -1.0) + 0.5) + f32ln(-0.6))) < 1e-12


# ---- the GPU tests' inputs: the share of fragile utterances, from the reference alone -------------------------------------------------------
def test_gpu_inputs_are_not_fragile():
    """tests/test_wordlm_gpu.py compares labels only where the reference's smallest decision margin is at least tau, and lets at most
    5 % of a test's utterances fall below.  On its seeds: 480 utterances, none fragile (smallest margin 1.3e-5, largest tau
    2.3e-10); 4 constrained utterances end without a hypothesis."""
    tot = frag = nohyp = 0
    mm, tm = math.inf, 0.0
    for case in WR.CASES:
        for constrained in (False, True):
            lm, sets = WR.case_inputs(*case, constrained)
            sc = WR.Scorer(lm)
            n = f = 0
            for W, nbest, xs in sets:
                for x in xs:
                    r = WR.search(x, W, nbest, case[1], lm, sc)
                    t = BR.tau(x.shape[0], r.kmax)
                    n += 1
                    f += r.margin < t
                    mm, tm = min(mm, r.margin), max(tm, t)
                    nohyp += not r.hyps
            assert f <= 0.05 * n, (case, constrained, f, n)
            tot += n
            frag += f
    print(f"{tot} utterances, {frag} fragile, min margin {mm:.3g}, max tau {tm:.3g}, {nohyp} without a hypothesis")
    assert tot == 480 and frag == 0 and nohyp >= 1


# ---- every ValueError ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit,msg", [
    (lambda s: s.replace("\\data\\", "\\dat\\"), "line 2: expected"),
    (lambda s: s.replace("ngram 2=4", "ngram 2=five"), "line 4: malformed count"),
    (lambda s: s.replace("ngram 2=4", "ngram 3=4"), "line 4: count of order 3"),
    (lambda s: s.replace("ngram 2=4", "ngram 2=3"), "line 20: the 2-grams section holds 4"),
    (lambda s: s.replace("ngram 3=2", "ngram 3=3"), "line 24: the 3-grams section holds 2"),
    (lambda s: s.replace("\\2-grams:", "\\3-grams:", 1), "line 14: section 3-grams out of sequence"),
    (lambda s: s.replace("-0.3 THE CAT -0.25", "-0.3 THE CAT -0.25 7"), "line 16: a 2-gram line"),
    (lambda s: s.replace("-0.3 THE CAT -0.25", "-0.3 THE"), "line 16: a 2-gram line"),
    (lambda s: s.replace("-0.3 THE CAT", "-0.3x THE CAT"), "line 16: .* does not parse"),
    (lambda s: s.replace("-0.3 THE CAT", "nan THE CAT"), "line 16: non-finite"),
    (lambda s: s.replace("-0.4 CAT SAT", "-0.4 THE CAT"), "line 17: n-gram `THE CAT` occurs twice"),
    (lambda s: s.replace("-0.4 CAT SAT", "-0.4 DOG SAT"), "line 17: the context `DOG`"),
    (lambda s: s.replace("-0.4 CAT SAT", "-0.4 CAT DOG"), "line 17: the word `DOG`"),
    (lambda s: s.replace("-0.15 THE CAT SAT", "-0.15 SAT CAT SAT"), "line 22: the context `SAT CAT`"),
    (lambda s: s.replace("\\end\\", ""), "ends without"),
    (lambda s: s + "more\n", "after \\\\end"),
    (lambda s: s.replace("\\3-grams:\n-0.05 <s> THE CAT\n-0.15 THE CAT SAT\n", ""), "before the 3-grams section"),
    (lambda s: s.replace("ngram 1=5", "stuff"), "line 3: expected a count"),
])
def test_arpa_errors_name_the_line(edit, msg):
    with pytest.raises(ValueError, match=msg):
        WordNgramLM.read_arpa(edit(ARPA))


def test_value_errors():
    t = tok()
    with pytest.raises(ValueError, match="no <unk> unigram"):
        WordNgramLM.from_arpa(ARPA, t)
    ng, bo = WordNgramLM.read_arpa(ARPA)
    ng[("<unk>",)] = -2.0
    lex = {"CAT": (5, 6, 7)}

    def make(ngrams=ng, backoffs=bo, lexicon=lex, V=32, delim=4, **kw):
        return WordNgramLM(ngrams, backoffs, lexicon, V, delim, **kw)

    make()
    for kw, msg in [(dict(V=65), "vocabulary 65"), (dict(V=1), "vocabulary 1"), (dict(delim=32), "delimiter 32"), (dict(delim=-1), "delimiter"),
                    (dict(alpha=math.nan), "finite"), (dict(beta=math.inf), "finite"), (dict(unk_penalty=0.5), "unk_penalty"),
                    (dict(unk_penalty=math.nan), "unk_penalty"), (dict(ngrams={}), "no n-grams"),
                    (dict(ngrams={**ng, ("A", "B", "C", "D", "E", "F"): -1.0}), "order 6"),
                    (dict(ngrams={**ng, ("DOG", "CAT"): -1.0}), "context DOG"), (dict(ngrams={**ng, ("CAT", "DOG"): -1.0}), "word DOG is no unigram"),
                    (dict(ngrams={**ng, ("CAT",): -math.inf}), "not finite"), (dict(backoffs={**bo, ("CAT",): math.nan}), "not finite"),
                    (dict(backoffs={**bo, ("DOG",): -0.1}), "no n-gram"), (dict(lexicon={}), "lexicon is empty"),
                    (dict(lexicon={"DOG": (5,)}), "no word of the model"), (dict(lexicon={"<unk>": (5,)}), "no word of the model"),
                    (dict(lexicon={"CAT": ()}), "spelling"), (dict(lexicon={"CAT": (5, 4)}), "spelling"), (dict(lexicon={"CAT": (32,)}), "spelling"),
                    (dict(lexicon={"CAT": (5, 6), "SAT": (5, 6)}), "share the spelling")]:
        with pytest.raises(ValueError, match=msg):
            make(**kw)
    with pytest.raises(ValueError, match="no <unk> unigram"):
        make(ngrams={k: v for k, v in ng.items() if k != ("<unk>",)})
    for kw, msg in [(dict(order=0), "order 0"), (dict(order=6), "order 6"), (dict(order=2, discount=1.0), "discount"), (dict(order=2, discount=0.0), "discount")]:
        with pytest.raises(ValueError, match=msg):
            WordNgramLM.from_text(["a b"], t, **kw)
    with pytest.raises(ValueError, match="no word"):
        WordNgramLM.from_text(["", "  "], t, 2)
    with pytest.raises(ValueError, match="cannot be a word"):
        WordNgramLM.count_ngrams([["A", "<s>"]], 2)
    with pytest.raises(ValueError, match="lexicon is empty"):
        WordNgramLM.from_text(["123 456"], t, 2)
    # the compiled arrays are validated (again before every first upload)
    for corrupt, msg in [(lambda m: m.arc_word.__setitem__(slice(0, 2), m.arc_word[1::-1].copy()), "sorted|state 0"),
                         (lambda m: m.arc_next.__setitem__(3, len(m.bo)), "next state"), (lambda m: m.arc_word.__setitem__(-1, 99), "word id"),
                         (lambda m: m.arc_logp.__setitem__(0, np.nan), "non-finite"), (lambda m: m.bo.__setitem__(1, -np.inf), "non-finite"),
                         (lambda m: m.bstate.__setitem__(2, 2), "backoff state"), (lambda m: m.arc0.__setitem__(1, 0), "state 0|partition|sorted"),
                         (lambda m: m.child.__setitem__((0, 9), 77), "bad node"), (lambda m: m.child.__setitem__((0, 4), 1), "bad node"),
                         (lambda m: m.word_at.__setitem__(0, 1), "bad word id"), (lambda m: setattr(m, "start_state", 99), "out of range"),
                         (lambda m: setattr(m, "arc_next", m.arc_next[:-1]), "differ in length")]:
        m = make()
        corrupt(m)
        with pytest.raises(ValueError, match=msg):
            m.validate()
    # beam_search's host checks (no device needed)
    m = make()
    _check_args(32, 16, 1, 0, m)
    for args, msg in [((31, 16, 1, 0, m), "vocabulary 32"), ((32, 16, 1, 4, m), "delimiter"), ((32, 16, 1, 5, m), "letter of its lexicon"),
                      ((32, 65, 1, 0, m), "beam_width"), ((32, 16, 1, 0, "arpa"), "CharNgramLM or a WordNgramLM")]:
        with pytest.raises(ValueError, match=msg):
            _check_args(*args)
    _check_args(4, 4, 1, 0, CharNgramLM(np.zeros((1, 4), np.float32), 1))
