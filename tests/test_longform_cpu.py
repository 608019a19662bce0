"""Long recordings, host side (wav2vec2.longform): the window plan against a brute force over the frame grid,
the numpy reference of the pause cuts on hand-built cases, the choice of cuts, and the property the whole layer rests on: the
greedy decode of the pieces, concatenated, is the greedy decode of the whole."""

import numpy as np
import pytest

import longform_reference as R
from wav2vec2 import Wav2Vec2Config
from wav2vec2.longform import Window, choose_cuts, group_windows, seconds_to_samples, window_plan

CFG = Wav2Vec2Config()
A = 320


def check_plan(L, window, margin):
    plan = window_plan(L, window, margin, CFG)
    F = CFG.num_frames(L)
    H, m = window - 2 * margin, margin // A
    h = H // A
    K = 1
    while (K - 1) * H + window < L:
        K += 1
    nxt = 0
    for w in plan:
        assert w.keepn > 0
        assert w.sample0 % H == 0 and w.samples == min(window, L - w.sample0) and w.sample0 + w.samples <= L
        k = w.sample0 // H
        nf = CFG.num_frames(w.samples)
        assert 0 <= w.keep0 and w.keep0 + w.keepn <= nf
        assert w.out0 == nxt == k * h + w.keep0            # in order, no gap, no overlap; local j is global k h + j
        for g in (w.out0, w.out0 + w.keepn - 1):           # the owner rule, at both ends of the kept range
            assert k == min(max((g - m) // h, 0), K - 1)
        # context: m frames (margin samples) of the window on each side of every kept frame's hop [A j, A j + A), unless the
        # recording starts / ends there.  Counted in whole frames that is m before and m - 1 behind: a window of window / A
        # hops holds window / A - 1 frames, the last hop being short of a receptive field (400 samples for a hop of 320)
        assert (w.keep0 >= m and A * w.keep0 >= margin) or w.out0 == 0
        last = w.keep0 + w.keepn - 1
        assert (w.samples - A * (last + 1) >= margin and nf - 1 - last >= m - 1) or w.out0 + w.keepn == F
        nxt += w.keepn
    assert nxt == F
    if L <= window:
        assert plan == [Window(0, L, 0, F, 0)]
    return plan


# window in {640, 960, 6400} x margin in {320, 640}, where legal (window >= 2 margin + A): 640 admits neither margin (see
# test_window_plan_illegal_combination_is_refused), 960 only 320
@pytest.mark.parametrize("window,margin", [(960, 320), (6400, 320), (6400, 640)])
def test_window_plan_tiles_the_frames(window, margin):
    lengths = list(range(400, 3 * window + 801)) + [40000, 250000]
    dropped = 0
    for L in lengths:
        plan = check_plan(L, window, margin)
        K = 1
        while (K - 1) * (window - 2 * margin) + window < L:
            K += 1
        dropped += len(plan) < K
    # the sweep meets recordings whose last window owns no frame -- with a margin of one frame only: the last window exists from
    # 2 margin + 1 samples past the one before and owns a frame from margin + 400 on, so margin >= 400 leaves no such length
    assert (dropped > 0) == (margin == 320)


def test_window_plan_illegal_combination_is_refused():
    for window, margin in [(640, 320), (640, 640), (960, 640)]:
        assert window < 2 * margin + A
        with pytest.raises(ValueError):
            window_plan(5000, window, margin, CFG)


def test_window_plan_argument_errors():
    for window, margin in [(6401, 640), (6400, 641), (6400, 0), (6400, 160), (1280, 640), (320, 320)]:
        with pytest.raises(ValueError):
            window_plan(10000, window, margin, CFG)
    with pytest.raises(ValueError):
        window_plan(399, 6400, 640, CFG)
    assert seconds_to_samples(20.0, 2.0, CFG) == (320000, 32000)
    assert seconds_to_samples(0.0301, 0.0199, CFG) == (640, 320)


def test_group_windows():
    ws = [Window(0, 6400, 0, 17, 0), Window(5120, 6400, 2, 16, 17), Window(10240, 401, 2, 1, 33)]
    assert group_windows(ws, 10 ** 9, CFG) == [(0, 3)]
    assert group_windows(ws, 6400 + 6400, CFG) == [(0, 2), (2, 3)]
    assert group_windows(ws, 1, CFG) == [(0, 1), (1, 2), (2, 3)]      # a window longer than the budget is a call of its own


# ---- the numpy reference of the pause cuts, on cases small enough to read ----

def rows(path, V=4, lead=5.0):
    x = np.zeros((len(path), V), np.float32)
    x[np.arange(len(path)), path] = lead
    return x


def cuts(x, blank=0, delim=-1, margin=2.0, min_pause=2):
    c, p = R.pause_cuts(x, blank, delim, margin, min_pause)
    return c.tolist(), p.tolist()


def test_reference_plain_pause_and_its_cut():
    assert cuts(rows([1, 0, 0, 0, 2])) == ([2], [3])
    assert cuts(rows([1, 0, 0, 0, 0, 2])) == ([3], [4])
    assert cuts(rows([1, 0, 2]), min_pause=2) == ([], [])
    assert cuts(rows([1, 0, 2]), min_pause=1) == ([1], [1])
    assert cuts(rows([1, 0, 0, 2, 0, 0, 0, 3])) == ([2, 5], [2, 3])


def test_reference_pause_at_the_start_or_the_end_is_no_pause():
    assert cuts(rows([0, 0, 0, 1, 2])) == ([], [])
    assert cuts(rows([1, 2, 0, 0, 0])) == ([], [])
    assert cuts(rows([0, 0, 0])) == ([], [])
    assert cuts(rows([0, 0, 1, 0, 0, 2, 0, 0])) == ([4], [2])


def test_reference_tie_takes_the_lowest_index():
    x = rows([1, 0, 0, 0, 2])
    x[2, 3] = 5.0                  # ties the blank: the argmax stays the blank (index 0), but the lead is 0 < margin
    assert cuts(x) == ([], [])
    assert cuts(x, margin=0.0) == ([2], [3])
    x = rows([1, 3, 3, 3, 2])
    x[1:4, 0] = 5.0                # the blank ties label 3 and wins as the lower index
    assert cuts(x, margin=0.0) == ([2], [3])
    assert cuts(x, blank=3, margin=0.0) == ([], [])      # ... and with blank = 3 the argmax is 0: not the blank


def test_reference_nan_frame_is_not_quiet_and_is_a_label():
    x = rows([1, 0, 0, 0, 0, 2])
    x[3, 2] = np.nan
    assert cuts(x, min_pause=2) == ([2], [2])             # [1, 3) ends at the NaN frame; [4, 5) is too short
    assert cuts(x, min_pause=1) == ([2, 4], [2, 1])
    assert cuts(x, delim=1, min_pause=1) == ([2], [2])    # the NaN frame (a_t = -1) is the last non-blank before [4, 5)


def test_reference_margin_met_with_equality():
    x = rows([1, 0, 0, 2], lead=0.0)
    x[[0, 3], [1, 2]] = 5.0
    x[1:3, 0] = np.float32(2.5)
    x[1:3, 1] = np.float32(0.5)
    assert cuts(x, margin=2.0) == ([2], [2])
    assert cuts(x, margin=np.nextafter(np.float32(2.0), np.float32(3.0))) == ([], [])


def test_reference_delimiter_rule():
    D = 3
    assert cuts(rows([1, D, 0, 0, 2]), delim=D) == ([3], [2])
    assert cuts(rows([1, D, 0, 0, 2]), delim=-1) == ([3], [2])
    assert cuts(rows([1, 2, 0, 0, 2]), delim=D) == ([], [])
    x = rows([1, D, 0, 0, 0, 0, 2])
    x[2, 1] = 4.0                  # a blank frame that is not quiet between the delimiter and the pause: the label carries over it
    assert cuts(x, delim=D) == ([4], [3])
    assert cuts(rows([0, 0, 1, 0, 0, 2]), delim=D) == ([], [])
    x = rows([0, 0, 0, 0, 2])
    x[0, 1] = 4.0                  # a pause with no label before it at all
    assert cuts(x, delim=D) == ([], [])
    assert cuts(x, delim=-1) == ([2], [3])


def test_reference_single_label_vocabulary_and_minus_infinity():
    assert cuts(np.zeros((5, 1), np.float32), blank=0) == ([], [])      # all quiet: one run from start to end
    x = rows([1, 0, 0, 2])
    x[1:3, 1:] = -np.inf
    assert cuts(x) == ([2], [2])
    x[1:3, 0] = -np.inf            # a row of -inf only: argmax 0 = blank, lead NaN: not quiet
    assert cuts(x, margin=-1.0) == ([], [])


# ---- choose_cuts ----

def test_choose_cuts():
    assert choose_cuts([], [], 1000) == []
    assert choose_cuts([100, 200, 300, 1400, 1600], [9] * 5, 5000, 250, 1500) == [1400]
    assert choose_cuts([100, 300, 500, 700], [9] * 4, 800, 250, 400) == [300, 700]
    assert choose_cuts([250, 251], [9, 9], 800, 250, 400) == [251]                 # (last + min_frames, ...]: 250 is too early
    assert choose_cuts([400, 401], [9, 9], 2000, 250, 400) == [400]                # ..., last + max_frames]: 400 is still in
    # nothing in range: the first candidate beyond max_frames, however far
    assert choose_cuts([100, 3000, 3100, 3400], [9] * 4, 5000, 250, 1500) == [3000, 3400]
    assert choose_cuts([100, 200], [9, 9], 5000, 250, 1500) == []
    with pytest.raises(ValueError):
        choose_cuts([5, 5], [1, 1], 100)
    with pytest.raises(ValueError):
        choose_cuts([5], [1, 1], 100)
    with pytest.raises(ValueError):
        choose_cuts([100], [1], 100)
    with pytest.raises(ValueError):
        choose_cuts([5], [1], 100, 50, 50)


# ---- the property: greedy of the pieces, concatenated, is greedy of the whole ----

def test_greedy_concatenation_equals_greedy_of_the_whole():
    rng = np.random.default_rng(20240)
    V, blank, delim, min_pause = 32, 0, 4, 8
    for i in range(200):
        T = int(rng.integers(600, 1400))
        x, path = R.peaky_logits(rng, T, V, blank, delim, min_pause, n_pauses=4)
        assert (np.argmax(x, axis=1) == path).all()
        c, p = R.pause_cuts(x, blank, delim if i % 2 else -1, 2.0, min_pause)
        assert (p >= min_pause).all()
        chosen = choose_cuts(c, p, T, min_frames=100, max_frames=400)
        assert len(chosen) + 1 >= 2, f"sequence {i}: no cut"
        b = [0] + chosen + [T]
        pieces = [R.greedy(x[s:e], blank) for s, e in zip(b, b[1:])]
        assert sum(pieces, []) == R.greedy(x, blank)
        for s in chosen:                                  # a cut lies strictly inside a run of blank-argmax frames
            assert path[s - 1] == blank and path[s] == blank
