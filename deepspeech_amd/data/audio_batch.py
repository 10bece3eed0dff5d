"""Front end of batches that carry raw audio (an audio store, data/store.py, or the dummy audio
source of data/synthetic.py): per step, on the device, waveform augmentation (training only:
speed perturbation, then additive noise), then the featurizer, so the trainer and the evaluation
see the [N, T, 161] frames they expect.

A batch's ``feats`` is [N, R, 160]: R rows of one 160-sample hop each, ``seq_lens`` [N] in rows.
Flattened, that is pcm [N, R * 160] with ``seq_lens * 160`` valid samples per utterance (the
store's zero padding to whole rows included, so a row count maps to a frame count whatever the
utterance: ``rows - 1`` frames for ``rows >= 3``, both feature kinds).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..ops.featurize import FRAME_LEN, AudioFeaturizer
from .store import AUDIO_HOP


def is_audio_batch(feats: torch.Tensor) -> bool:
    return feats.dim() == 3 and feats.shape[2] == AUDIO_HOP


def samples_for_frames(frames, kind: str):
    """The fewest samples whose frame count (ops/featurize.py num_frames) reaches ``frames`` (an
    int or an integer tensor): 0 for one frame or fewer, else L + 160 (frames - 2) + 1."""
    need = FRAME_LEN[kind] + AUDIO_HOP * (frames - 2) + 1
    if isinstance(frames, torch.Tensor):
        return torch.where(frames <= 1, torch.zeros_like(need), need)
    return 0 if frames <= 1 else int(need)


def max_samples_for_frames(frames: int, kind: str) -> int:
    """The most samples whose frame count stays within ``frames`` >= 1."""
    return FRAME_LEN[kind] + AUDIO_HOP * (int(frames) - 1)


def ctc_min_samples(labels: torch.Tensor, label_lens: torch.Tensor, kind: str) -> torch.Tensor:
    """int32 [N]: the fewest samples that keep each utterance's CTC feasible, i.e. whose frame
    count reaches 4 (label_len + repeats) + 34, the rule of data/store.py min_frames. ``labels``
    [N, Lmax] (padding of any value), ``label_lens`` [N], on any device, no synchronisation."""
    ll = label_lens.long()
    if labels.shape[1] > 1:
        pos = torch.arange(1, labels.shape[1], device=labels.device)[None, :]
        rep = ((labels[:, 1:] == labels[:, :-1]) & (pos < ll[:, None])).sum(1)
    else:
        rep = torch.zeros_like(ll)
    return samples_for_frames(4 * (ll + rep) + 34, kind).to(torch.int32)


class AudioFrontEnd:
    """``front(batch, step, first_utt, training)`` -> the batch with ``feats`` [N, T, 161] and
    ``seq_lens`` [N] frames in place of the audio rows. ``speed`` (ops/speed.py SpeedPerturb) and
    ``wave_aug`` (ops/waveaug.py WaveAugment) run in training only, speed first: the noise is added
    to the perturbed audio under its new lengths. A perturbed utterance keeps at least the samples
    its label needs (``ctc_min_samples``) and at most those of ``max_frames`` (0: no limit), or it
    stays as it is. On a GPU: the augmentations' launches, then the featurizer's two, no host
    synchronisation; on a CPU device all take their reference paths."""

    def __init__(self, kind: str = "mfcc", device=None, wave_aug=None, speed=None, max_frames: int = 0):
        self.featurizer = AudioFeaturizer(kind, device=device, normalize="utterance")
        self.device = self.featurizer.device
        self.kind = kind
        self.wave_aug = wave_aug
        self.speed = speed
        self.max_out = max_samples_for_frames(max_frames, kind) if max_frames > 0 else 0

    @torch.no_grad()
    def _perturb(self, batch, pcm, lens, step: int, first_utt: int, host):
        """Speed perturbation of the batch's audio. ``host`` (the host batch: ``seq_lens`` in rows,
        ``labels`` padded with negative values, ``label_lens``) gives the tight output width;
        without it the width is the policy's worst case."""
        min_out = ctc_min_samples(batch["labels"], batch["label_lens"], self.kind).to(self.device)
        width = None
        if host is not None:
            N, S = pcm.shape
            hmin = ctc_min_samples(torch.as_tensor(host.labels), torch.as_tensor(host.label_lens), self.kind)
            hlens = torch.as_tensor(host.seq_lens).to(torch.int64) * AUDIO_HOP
            width = self.speed.tight_width(hlens, N, S, step, first_utt, hmin, self.max_out)
        return self.speed(pcm, lens, step, first_utt=first_utt, min_out=min_out, max_out=self.max_out, out_width=width)

    @torch.no_grad()
    def __call__(self, batch: Dict[str, torch.Tensor], step: int = 0, first_utt: int = 0,
                 training: bool = False, host=None) -> Dict[str, torch.Tensor]:
        rows = batch["feats"]
        if not is_audio_batch(rows):
            raise ValueError("AudioFrontEnd: feats must be [N, R, %d] audio rows, got %s"
                             % (AUDIO_HOP, tuple(rows.shape)))
        N, R, _ = rows.shape
        pcm = rows.to(self.device).contiguous().view(N, R * AUDIO_HOP)
        lens = (batch["seq_lens"].to(self.device) * AUDIO_HOP).to(torch.int32)
        if training and self.speed is not None:
            pcm, lens = self._perturb(batch, pcm, lens, step, first_utt, host)
        if training and self.wave_aug is not None:
            pcm = self.wave_aug(pcm, lens, step, first_utt=first_utt)
        feats, frames = self.featurizer(pcm, lens)
        return dict(batch, feats=feats, seq_lens=frames)


def front_end_for(feats_width: int, kind: str, device, wave_aug=None, speed=None,
                  max_frames: int = 0) -> Optional[AudioFrontEnd]:
    """The front end of a source whose rows are ``feats_width`` wide: None for feature frames."""
    return AudioFrontEnd(kind, device, wave_aug, speed, max_frames) if feats_width == AUDIO_HOP else None
