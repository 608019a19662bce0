"""MI355X-native drop-in for the reference's ``wav2vec2`` package surface
(src/wav2vec2/__init__.py:1-4): the same six names, and the long-recording layer on top
(wav2vec2.longform: window_plan, decode_long, LongTranscript) and the sampling rates (wav2vec2.audio: Resampler, resample,
resampled_length, speed_perturb) and the waveform augmentation for fine-tuning (wav2vec2.audio: reverberate, add_noise, Augment,
rir_delay, trim_rir) and the error rates (wav2vec2.metrics: wer, cer, oracle_wer, mbr_select, edit_distance) and
the Trainer's learning-rate schedules (wav2vec2.training: linear_schedule, tri_stage_schedule)."""

from .audio import Augment, Resampler, add_noise, resample, resampled_length, reverberate, rir_delay, speed_perturb, trim_rir
from .config import RobustWav2Vec2Config, Wav2Vec2Config
from .longform import LongTranscript, ScoredLongTranscript, decode_long, window_plan
from .losses import CTCLoss, MWERLoss, StarCTCLoss, expected_risk, star_labels
from .metrics import (EditCounts, ErrorRate, Evaluation, cer, edit_distance, edit_distance_pairs, mbr_select, oracle_wer,
                      wer)
from .modeling import Wav2Vec2ForCTC, Wav2Vec2Model
from .processor import Wav2Vec2Processor
from .training import Trainer, linear_schedule, tri_stage_schedule

__all__ = ["Wav2Vec2Config", "RobustWav2Vec2Config", "CTCLoss", "MWERLoss", "StarCTCLoss", "expected_risk", "star_labels", "Wav2Vec2ForCTC", "Wav2Vec2Model",
           "Wav2Vec2Processor", "Trainer", "window_plan", "decode_long", "LongTranscript", "ScoredLongTranscript", "Resampler", "resample",
           "resampled_length", "speed_perturb", "reverberate", "add_noise", "Augment", "rir_delay", "trim_rir", "EditCounts", "ErrorRate", "Evaluation", "wer", "cer", "oracle_wer", "mbr_select",
           "edit_distance", "edit_distance_pairs", "linear_schedule", "tri_stage_schedule"]
