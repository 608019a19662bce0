"""split_at_pauses (wav2vec2.alignment): an aligned recording cut into utterance-sized pieces.  Host code only."""

import pytest

from wav2vec2.alignment import AlignedSegment, WordSpan, split_at_pauses


def words(*spans):
    """WordSpans from (text, start, end) or (text, start, end, score)"""
    return [WordSpan(s[0], float(s[1]), float(s[2]), s[3] if len(s) > 3 else 1.0) for s in spans]


def texts(pieces):
    return [p.text for p in pieces]


def test_empty_list():
    assert split_at_pauses([]) == []


def test_no_gap_reaches_the_threshold():
    ws = words(("A", 0.0, 0.5), ("B", 0.6, 1.0), ("C", 1.29, 2.0))
    (piece,) = split_at_pauses(ws, min_pause_s=0.3)
    assert piece == AlignedSegment("A B C", 0.0, 2.0, 1.0, ws)
    assert isinstance(piece, AlignedSegment) and piece.words == ws


def test_a_cut_at_every_gap():
    ws = words(("A", 0.0, 0.5), ("B", 1.0, 1.5), ("C", 2.0, 2.5), ("D", 2.75, 3.0))
    pieces = split_at_pauses(ws, min_pause_s=0.25)              # every gap (0.5, 0.5, 0.25) reaches it: >= counts
    assert texts(pieces) == ["A", "B", "C", "D"]
    assert [(p.start_s, p.end_s) for p in pieces] == [(0.0, 0.5), (1.0, 1.5), (2.0, 2.5), (2.75, 3.0)]
    assert texts(split_at_pauses(ws, min_pause_s=0.5)) == ["A", "B", "C D"]


def test_scores_and_texts_of_the_pieces():
    ws = words(("SO", 0.0, 0.4, 0.9), ("IT", 0.5, 0.8, 0.5), ("GOES", 2.0, 2.5, 0.25), ("ON", 2.6, 3.0, 0.75))
    a, b = split_at_pauses(ws, min_pause_s=1.0)
    assert (a.text, a.start_s, a.end_s) == ("SO IT", 0.0, 0.8) and a.score == pytest.approx(0.7)
    assert (b.text, b.start_s, b.end_s) == ("GOES ON", 2.0, 3.0) and b.score == pytest.approx(0.5)
    assert a.words == ws[:2] and b.words == ws[2:]
    # words that carry ids keep them: the piece's text is the tuple of the words' id tuples
    ids = [w._replace(text=(i, i + 1)) for i, w in enumerate(ws)]
    assert texts(split_at_pauses(ids, min_pause_s=1.0)) == [((0, 1), (1, 2)), ((2, 3), (3, 4))]


def test_an_over_long_piece_is_cut_at_its_largest_gap():
    # gaps 0.25, 0.5, 0.25: none reaches the pause threshold; 4.0 s in all
    ws = words(("A", 0.0, 0.75), ("B", 1.0, 1.75), ("C", 2.25, 3.0), ("D", 3.25, 4.0))
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=4.0)) == ["A B C D"]       # exactly max_len_s fits
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=3.0)) == ["A B", "C D"]
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=1.0)) == ["A", "B", "C", "D"]


def test_the_earliest_of_equal_gaps_and_down_to_single_words():
    # equal gaps of 0.25 (exact in binary): each over-long piece loses its FIRST word
    ws = words(("A", 0.0, 1.0), ("B", 1.25, 2.25), ("C", 2.5, 3.5), ("D", 3.75, 4.75))
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=4.0)) == ["A", "B C D"]
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=3.0)) == ["A", "B", "C D"]
    # a single word longer than the limit stays a piece of its own
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=0.5)) == ["A", "B", "C", "D"]
    long_word = words(("LONG", 0.0, 30.0))
    assert texts(split_at_pauses(long_word, max_len_s=20.0)) == ["LONG"]


def test_pause_cuts_come_first_then_the_length():
    ws = words(("A", 0.0, 1.0), ("B", 1.125, 2.0), ("C", 2.5, 3.0), ("D", 5.0, 6.0), ("E", 6.25, 7.0))
    # the pause before D cuts; A B C (3.0 s) is then over 2.5 s and loses C at its largest gap (0.5)
    assert texts(split_at_pauses(ws, min_pause_s=1.0, max_len_s=2.5)) == ["A B", "C", "D E"]
    assert texts(split_at_pauses(ws)) == ["A B", "C", "D E"]                                  # defaults: 0.3 s, 20 s
