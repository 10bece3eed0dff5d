"""Front end of batches that carry raw audio (an audio store, data/store.py, or the dummy audio
source of data/synthetic.py): per step, on the device, waveform augmentation (training only),
then the featurizer, so the trainer and the evaluation see the [N, T, 161] frames they expect.

A batch's ``feats`` is [N, R, 160]: R rows of one 160-sample hop each, ``seq_lens`` [N] in rows.
Flattened, that is pcm [N, R * 160] with ``seq_lens * 160`` valid samples per utterance (the
store's zero padding to whole rows included, so a row count maps to a frame count whatever the
utterance: ``rows - 1`` frames for ``rows >= 3``, both feature kinds).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..ops.featurize import AudioFeaturizer
from .store import AUDIO_HOP


def is_audio_batch(feats: torch.Tensor) -> bool:
    return feats.dim() == 3 and feats.shape[2] == AUDIO_HOP


class AudioFrontEnd:
    """``front(batch, step, first_utt, training)`` -> the batch with ``feats`` [N, T, 161] and
    ``seq_lens`` [N] frames in place of the audio rows. ``wave_aug`` (ops/waveaug.py WaveAugment)
    runs in training only. On a GPU: the augmentation's launches, then the featurizer's two, no
    host synchronisation; on a CPU device both take their reference paths."""

    def __init__(self, kind: str = "mfcc", device=None, wave_aug=None):
        self.featurizer = AudioFeaturizer(kind, device=device, normalize="utterance")
        self.device = self.featurizer.device
        self.kind = kind
        self.wave_aug = wave_aug

    @torch.no_grad()
    def __call__(self, batch: Dict[str, torch.Tensor], step: int = 0, first_utt: int = 0,
                 training: bool = False) -> Dict[str, torch.Tensor]:
        rows = batch["feats"]
        if not is_audio_batch(rows):
            raise ValueError("AudioFrontEnd: feats must be [N, R, %d] audio rows, got %s"
                             % (AUDIO_HOP, tuple(rows.shape)))
        N, R, _ = rows.shape
        pcm = rows.to(self.device).contiguous().view(N, R * AUDIO_HOP)
        lens = (batch["seq_lens"].to(self.device) * AUDIO_HOP).to(torch.int32)
        if training and self.wave_aug is not None:
            pcm = self.wave_aug(pcm, lens, step, first_utt=first_utt)
        feats, frames = self.featurizer(pcm, lens)
        return dict(batch, feats=feats, seq_lens=frames)


def front_end_for(feats_width: int, kind: str, device, wave_aug=None) -> Optional[AudioFrontEnd]:
    """The front end of a source whose rows are ``feats_width`` wide: None for feature frames."""
    return AudioFrontEnd(kind, device, wave_aug) if feats_width == AUDIO_HOP else None
