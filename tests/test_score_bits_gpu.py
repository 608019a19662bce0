"""The bits of exact CTC scoring, pinned: every logp, every gradient row and the workspace sizes of the six forms of csrc/score.hip
(w2v2_ctc_score, w2v2_ctc_score_star and w2v2_ctc_score_grad_star without and with stars, w2v2_ctc_score_grad) must EQUAL what
tests/golden/score_bits.json recorded from the three separate scorer files that score.hip replaced (tests/golden/make_score_bits.py:
the sets, what is stored, and how to record again).  No tolerance: the star, the plane store and the grouping are template
parameters and host loops around one sequence of fp64 operations per state, and a change to that sequence has to show here.

The fixture depends on the compiler's exp and log; it names the toolchain it was recorded under."""

import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_score_bits as MB                                     # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("score", "score_star", "score_star_planted", "grad", "grad_star", "grad_star_planted")


@pytest.fixture(scope="module")
def recorded():
    with open(MB.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    import torch
    from wav2vec2 import _native as N
    torch.cuda.set_device(0)
    return MB.run_all(N.load(), N, torch)


@pytest.mark.parametrize("name", ["layouts", "mixed", "nonfinite", "wide"])
def test_same_bits_as_recorded(recorded, got, name):
    want, have = recorded["sets"][name], got[name]
    print(f"{name}: recorded from {recorded['recorded_from']} under {recorded['toolchain']}")
    assert have["workspace"] == want["workspace"], (name, "workspace bytes", have["workspace"], want["workspace"])
    for form in FORMS:
        diff = [j for j, (a, b) in enumerate(zip(have[form]["logp"], want[form]["logp"])) if a != b]
        assert len(have[form]["logp"]) == len(want[form]["logp"]) and not diff, (name, form, "logp of pairs", diff)
        if "rows" in want[form]:
            diff = [i for i, (a, b) in enumerate(zip(have[form]["rows"], want[form]["rows"])) if a != b]
            assert len(have[form]["rows"]) == len(want[form]["rows"]) and not diff, (name, form, "gradient rows of utterances", diff)
    # what the fixture itself must show: the star entry points on star-free labels carry the star-free bits
    assert want["score_star"] == want["score"] and want["grad_star"] == want["grad"], name
    assert want["grad"]["logp"] == want["score"]["logp"] and want["grad_star_planted"]["logp"] == want["score_star_planted"]["logp"], name


def test_groups_change_no_bit(recorded, got):
    """the layout set once more with max_workspace_bytes just above what the largest utterance needs alone"""
    want, have = recorded["sets"]["layouts_grouped"], got["layouts_grouped"]
    for form in FORMS[3:]:
        assert have[form] == want[form], form
        assert want[form] == recorded["sets"]["layouts"][form], form
