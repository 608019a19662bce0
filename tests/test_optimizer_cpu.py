"""Host side of the extended optimizer: the learning-rate schedules and the Trainer's argument validation.
No GPU: the stub model below raises on any attribute but `_with_lm_head`, so a validation that came after a native call
(or any other use of the model) would show up as an AttributeError instead of the ValueError."""

import numpy as np
import pytest

import wav2vec2
from wav2vec2.training import Trainer, linear_schedule, tri_stage_schedule


# ---- schedules -------------------------------------------------------------------------------
def test_linear_schedule_values():
    peak, W, T, final = 3e-4, 10, 100, 1e-6
    f = linear_schedule(peak, W, T, final_lr=final)
    assert f(0) == pytest.approx(peak / W, rel=1e-15)
    assert f(W - 1) == pytest.approx(peak, rel=1e-15)          # the last warm-up step runs at the peak
    warm = [f(i) for i in range(W)]
    assert all(b > a for a, b in zip(warm, warm[1:]))
    assert f(W) < peak
    tail = [f(i) for i in range(W - 1, T + 1)]
    assert all(b < a for a, b in zip(tail, tail[1:]))
    mid = (W - 1 + T) / 2                                       # linear: half way down in the middle of the decay
    assert f(mid) == pytest.approx((peak + final) / 2, rel=1e-12)
    assert f(T) == final and f(T + 1000) == final


def test_linear_schedule_without_warmup_and_bad_arguments():
    f = linear_schedule(1e-3, 0, 50)
    assert f(0) == 1e-3 and f(25) == pytest.approx(5e-4, rel=1e-12) and f(50) == 0.0
    for bad in ((1e-3, 11, 10), (1e-3, -1, 10), (1e-3, 0, 0)):
        with pytest.raises(ValueError):
            linear_schedule(*bad)


def test_tri_stage_schedule_values():
    peak, T = 5e-5, 1000
    f = tri_stage_schedule(peak, T)
    warm, hold = 100, 400                                       # phase_ratio (0.1, 0.4, 0.5)
    assert f(0) == pytest.approx(peak * 0.01, rel=1e-15)
    ramp = [f(i) for i in range(warm + 1)]
    assert all(b > a for a, b in zip(ramp, ramp[1:]))
    assert f(warm - 1) == pytest.approx(peak * (0.01 + 0.99 * (warm - 1) / warm), rel=1e-14)
    assert f(warm) == peak and f(warm + hold - 1) == peak      # held
    assert f(warm + hold) == pytest.approx(peak, rel=1e-15)    # the decay starts at the peak ...
    assert f(warm + hold + 1) < peak
    # ... is exponential: equal ratios between consecutive steps ...
    r = [f(i + 1) / f(i) for i in (warm + hold, warm + hold + 100, T - 2)]
    assert np.allclose(r, r[0], rtol=1e-12, atol=0) and r[0] == pytest.approx(0.05 ** (1 / 500), rel=1e-12)
    # ... and ends at peak * final_scale
    assert abs(f(T) - peak * 0.05) <= 1e-12 * peak
    assert abs(f(T - 1) * r[0] - peak * 0.05) <= 1e-12 * peak
    assert f(T + 7) == f(T)


def test_tri_stage_schedule_other_phases_and_bad_arguments():
    f = tri_stage_schedule(1.0, 10, phase_ratio=(0.0, 0.5, 0.5), init_scale=0.1, final_scale=0.5)
    assert f(0) == 1.0 and f(4) == 1.0 and f(5) == pytest.approx(1.0) and abs(f(10) - 0.5) <= 1e-12
    with pytest.raises(ValueError):
        tri_stage_schedule(1.0, 10, phase_ratio=(0.5, 0.4, 0.5))
    with pytest.raises(ValueError):
        tri_stage_schedule(1.0, 10, phase_ratio=(0.5, 0.5))
    with pytest.raises(ValueError):
        tri_stage_schedule(1.0, 10, final_scale=0.0)


def test_schedules_are_exported():
    assert wav2vec2.linear_schedule is linear_schedule and wav2vec2.tri_stage_schedule is tri_stage_schedule


# ---- constructor validation -------------------------------------------------------------------
class _Stub:
    """A model of which only `_with_lm_head` may be read."""
    _with_lm_head = True

    def __getattr__(self, name):
        raise AssertionError(f"Trainer touched model.{name} before validating its arguments")


@pytest.mark.parametrize("kwargs", [dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(weight_decay=-0.01),
                                    dict(accumulation_steps=0), dict(accumulation_steps=-2),
                                    dict(accumulation_steps=2, collective="native"),
                                    dict(accumulation_steps=4, collective="native-rs")])
def test_trainer_rejects_invalid_optimizer_arguments(kwargs):
    with pytest.raises(ValueError):
        Trainer(_Stub(), loss=None, **kwargs)


def test_valid_optimizer_arguments_pass_validation():
    """The same stub with valid arguments gets past the validation: it is the first use of the model that fails."""
    with pytest.raises(AssertionError, match="touched model"):
        Trainer(_Stub(), loss=None, max_grad_norm=1.0, weight_decay=0.01, accumulation_steps=2, skip_nonfinite=True)
