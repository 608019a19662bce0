"""Streaming, host side (wav2vec2.streaming): the windows ``stream_plan`` hands out while a recording grows are, in
any chunking, exactly ``window_plan`` of the finished recording, and none is handed out before its samples are in; the argument
checks of ``BeamStream`` that need no device."""

import numpy as np
import pytest

from wav2vec2 import Wav2Vec2Config
from wav2vec2.longform import window_plan
from wav2vec2.streaming import stream_plan

CFG = Wav2Vec2Config()
A = 320


def feed_in_chunks(N, window, margin, chunks):
    """the windows stream_plan returns while `chunks` (summing to N) arrive, then with final=True; each checked against what was received"""
    got, received = [], 0
    for c in chunks:
        received += c
        new = stream_plan(received, len(got), window, margin, CFG)
        for w in new:
            assert received >= w.sample0 + w.samples, (N, window, margin, received, w)
        got += new
    assert received == N
    last = stream_plan(N, len(got), window, margin, CFG, final=True)
    for w in last:
        assert N >= w.sample0 + w.samples
    return got + last


def chunkings(rng, N, window, margin):
    """random chunk sizes; one sample at a time around every k H + window; everything at once; a fixed size"""
    H = window - 2 * margin
    yield [N]
    yield [min(1600, N - s) for s in range(0, N, 1600)]
    sizes = []
    while sum(sizes) < N:
        sizes.append(min(int(rng.integers(1, 2 * window)), N - sum(sizes)))
    yield sizes
    # up to each boundary k H + window - 2 in one chunk, then four chunks of one sample across it
    cuts, k = [], 0
    while k * H + window - 2 < N:
        b = k * H + window
        cuts += [p for p in (b - 2, b - 1, b, b + 1, b + 2) if 0 < p < N]
        k += 1
    cuts = sorted(set(cuts)) + [N]
    yield [b - a for a, b in zip([0] + cuts[:-1], cuts) if b > a]


@pytest.mark.parametrize("window,margin", [(960, 320), (6400, 640), (6400, 320), (3200, 1280)])
def test_stream_plan_under_any_chunking(window, margin):
    rng = np.random.default_rng(window + margin)
    H = window - 2 * margin
    lengths = [400, 401, window - 1, window, window + 1, 3 * H + window - 1, 3 * H + window, 3 * H + window + 1, 2 * H + window + 719]
    lengths += [int(v) for v in rng.integers(400, 6 * window, 40)]
    ncases = 0
    for N in lengths:
        want = window_plan(N, window, margin, CFG)
        for chunks in chunkings(rng, N, window, margin):
            assert sum(chunks) == N and min(chunks) >= 1
            got = feed_in_chunks(N, window, margin, chunks)
            assert got == want, (N, window, margin, chunks[:8])
            ncases += 1
    assert ncases >= 4 * 49


def test_window_ending_the_recording_is_held_back():
    """a recording of exactly k H + window samples: window k is its last and keeps rows to the end, so it must not be handed out
    before one more sample (or the end) has come"""
    window, margin = 6400, 640
    H = window - 2 * margin
    N = 3 * H + window
    assert len(window_plan(N, window, margin, CFG)) == 4
    assert len(stream_plan(N, 0, window, margin, CFG)) == 3
    assert len(stream_plan(N + 1, 0, window, margin, CFG)) == 4
    assert stream_plan(N, 3, window, margin, CFG, final=True) == window_plan(N, window, margin, CFG)[3:]
    assert stream_plan(N + 1, 0, window, margin, CFG)[3] != window_plan(N, window, margin, CFG)[3]


def test_too_few_samples_give_no_window():
    assert stream_plan(0, 0, 6400, 640, CFG) == []
    assert stream_plan(399, 0, 6400, 640, CFG) == []
    assert stream_plan(399, 0, 6400, 640, CFG, final=True) == []
    assert stream_plan(400, 0, 6400, 640, CFG) == []
    assert stream_plan(400, 0, 6400, 640, CFG, final=True) == window_plan(400, 6400, 640, CFG)
    with pytest.raises(ValueError):
        stream_plan(100, 0, 6400, 100, CFG)
    with pytest.raises(ValueError):
        stream_plan(10000, -1, 6400, 640, CFG)


def test_beam_stream_refuses_before_touching_a_device():
    from wav2vec2.decoding import BeamStream, CharNgramLM
    with pytest.raises(ValueError, match="streams"):
        BeamStream(0, 32)
    with pytest.raises(ValueError, match="beam_width"):
        BeamStream(1, 32, beam_width=65)
    with pytest.raises(ValueError, match="nbest"):
        BeamStream(1, 32, beam_width=4, nbest=5)
    with pytest.raises(ValueError, match="vocabulary"):
        BeamStream(1, 32, lm=CharNgramLM(np.zeros((1, 5), np.float32), 1))
    with pytest.raises(ValueError, match="initial_frames"):
        BeamStream(1, 32, initial_frames=0)
    with pytest.raises(MemoryError, match="max_workspace_bytes"):
        BeamStream(4, 32, beam_width=64, initial_frames=1000, max_workspace_bytes=1 << 20)
