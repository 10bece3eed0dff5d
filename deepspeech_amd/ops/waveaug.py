"""Additive noise at a random signal-to-noise ratio on the waveform (csrc/waveaug.hip), the
augmentation of the Deep Speech 2 recipe: it has to act before the featurizer, because its effect
on MFCC / log-spectrogram frames is not linear.

A policy is (p, SNR range); a noise bank is C clips back to back. Per utterance of pcm [B, S] with
n = clamp(lens[b], 0, S) valid samples:

    plan row  (on, clip, off, snr_cdb) int32, one Philox4x32-10 block, key = seed, counter =
              (0, global utterance index u, step) on a stream of its own (bit 30 of the last word)
              on = n > 0 and U(1000000) < p_ppm, clip = U(C), off = U(length[clip]),
              snr_cdb = snr_lo_cdb + U(snr_hi_cdb - snr_lo_cdb + 1), U(m) = (x * m) >> 32
    noise     z_i = the clip read as a loop from off
    k         sqrt(Ex / (En 10^(snr_cdb / 1000))), Ex and En the energies of x and z over i < n:
              torchaudio.functional.add_noise's definition over the whole utterance
    output    fp32: x_i + k z_i for i < n when on (two roundings), x_i when not, +0 for i >= n

The plan is a pure function of (seed, step, u, n, bank shape, policy), whatever the batch size,
the row, the world size or a resume; Ex, En and k depend on the row's content, n, clip and off
alone. ops/reference.py holds the definition in fp64 and exact integers.

The kernels take contiguous fp32 or int16 [B, S] with S % 8 == 0 on the bank's GPU: four launches
(plan, energy partials, coefficient, apply) on the current stream, no host synchronisation.
Anything else on a GPU takes the plan kernel and the torch composite of the same definition, a
CPU tensor the reference: slower, never silently wrong. A gain perturbation is deliberately
absent: the featurizer removes DC and peak-normalises each utterance, so a gain is a no-op.
"""
from __future__ import annotations

import glob
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _ext
from . import reference as R

MAX_B, MAX_S, MIN_CLIP = 65535, (1 << 30) - 8, 160
AUDIO_EXTS = (".wav", ".flac", ".npy")


@dataclass(frozen=True)
class WaveAugPolicy:
    noise: str = "synthetic"     # a directory of noise clips, or "synthetic"
    p_ppm: int = 1000000         # share of utterances that get noise, parts per million
    snr_lo_cdb: int = 1000       # SNR range in integer centi-dB, both ends included
    snr_hi_cdb: int = 3000

    def __post_init__(self):
        for name in ("p_ppm", "snr_lo_cdb", "snr_hi_cdb"):
            v = getattr(self, name)
            if not isinstance(v, int) or isinstance(v, bool) or abs(v) > 1 << 20:
                raise ValueError("wave_aug: %s must be an integer of magnitude <= 2^20, not %r" % (name, v))
        if not 0 <= self.p_ppm <= 1000000:
            raise ValueError("wave_aug: p must lie in [0, 1]")
        if self.snr_lo_cdb > self.snr_hi_cdb:
            raise ValueError("wave_aug: snr=LO:HI needs LO <= HI")
        if not self.noise:
            raise ValueError("wave_aug: noise=PATH|synthetic is empty")

    @classmethod
    def parse(cls, spec: str) -> "WaveAugPolicy":
        """"noise=PATH|synthetic,p=0.4,snr=10:30" (any subset; p is converted once to integer parts
        per million, the SNR bounds in dB to integer centi-dB; snr=20 is the range 20:20)."""
        kw = {}
        for item in filter(None, (s.strip() for s in spec.split(","))):
            key, sep, val = item.partition("=")
            key, val = key.strip(), val.strip()
            if not sep or key in kw:
                raise ValueError("wave_aug: bad or repeated item %r in %r" % (item, spec))
            if key == "noise":
                kw[key] = val
            elif key == "p":
                kw[key] = int(round(float(val) * 1000000))
            elif key == "snr":
                lo, sep2, hi = val.partition(":")
                kw[key] = (int(round(float(lo) * 100)), int(round(float(hi if sep2 else lo) * 100)))
            else:
                raise ValueError("wave_aug: unknown key %r in %r (noise, p, snr)" % (key, spec))
        args = {}
        if "noise" in kw:
            args["noise"] = kw["noise"]
        if "p" in kw:
            args["p_ppm"] = kw["p"]
        if "snr" in kw:
            args["snr_lo_cdb"], args["snr_hi_cdb"] = kw["snr"]
        return cls(**args)

    def __str__(self) -> str:
        return "noise=%s,p=%g,snr=%g:%g" % (self.noise, self.p_ppm / 1e6, self.snr_lo_cdb / 100.0, self.snr_hi_cdb / 100.0)


class NoiseBank:
    """C >= 1 noise clips, each finite and at least 160 samples (one hop): data fp32 [Ntot],
    start / length int32 [C] on the host, with copies per device made on first use."""

    def __init__(self, clips: Sequence):
        clips = [np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c) for c in clips]
        if not clips:
            raise ValueError("NoiseBank: no clips")
        for i, c in enumerate(clips):
            if c.ndim != 1 or c.shape[0] < MIN_CLIP:
                raise ValueError("NoiseBank: clip %d must be 1-D with at least %d samples, got shape %s"
                                 % (i, MIN_CLIP, c.shape))
            if not np.isfinite(c).all():
                raise ValueError("NoiseBank: clip %d holds a non-finite sample" % i)
        length = np.array([c.shape[0] for c in clips], np.int64)
        if int(length.sum()) >= 1 << 31:
            raise ValueError("NoiseBank: %d samples in all; the bank holds fewer than 2^31" % int(length.sum()))
        self.data = torch.from_numpy(np.concatenate([c.astype(np.float32) for c in clips]))
        if not bool(torch.isfinite(self.data).all()):
            raise ValueError("NoiseBank: a clip leaves the fp32 range")
        self.length = torch.from_numpy(length.astype(np.int32))
        self.start = torch.from_numpy((np.cumsum(length) - length).astype(np.int32))
        self._dev = {}

    def __len__(self) -> int:
        return int(self.length.numel())

    def on(self, device):
        """(data, start, length) on ``device``."""
        device = torch.device(device)
        if device.type == "cpu":
            return self.data, self.start, self.length
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.data, self.start, self.length))
        return self._dev[key]

    @classmethod
    def from_dir(cls, path: str, rate: int = 16000) -> "NoiseBank":
        """Every audio file under ``path`` in sorted order, read by data/preprocess.py read_audio;
        a file at another rate is resampled to ``rate`` (ops/resample.py)."""
        from ..data.preprocess import read_audio
        files = sorted(f for f in glob.glob(os.path.join(path, "**", "*"), recursive=True)
                       if os.path.splitext(f)[1].lower() in AUDIO_EXTS)
        if not files:
            raise ValueError("NoiseBank: no audio files (%s) under %s" % (", ".join(AUDIO_EXTS), path))
        clips = []
        for f in files:
            audio, sr = read_audio(f)
            if not np.isfinite(audio).all():
                raise ValueError("NoiseBank: %s holds a non-finite sample" % f)
            if sr != rate:
                from .resample import Resampler
                y, n = Resampler(sr, rate)(audio.astype(np.float32)[None, :])
                audio = y[0, : int(n[0])].cpu().numpy()
            if audio.shape[0] < MIN_CLIP:
                raise ValueError("NoiseBank: %s has %d samples at %d Hz; a clip needs %d" % (f, audio.shape[0], rate, MIN_CLIP))
            clips.append(audio)
        return cls(clips)

    @classmethod
    def synthetic(cls, seed: int = 0) -> "NoiseBank":
        """Four seeded clips of unequal length, white and low-passed (a moving average), made in
        numpy: the bank of --dummy runs, tests and the bench."""
        rng = np.random.default_rng(seed)
        clips = []
        for length, taps in ((16000, 1), (7321, 8), (24000, 32), (4800, 1)):
            w = rng.standard_normal(length + taps - 1)
            clips.append(np.convolve(w, np.ones(taps) / taps, mode="valid").astype(np.float32))
        return cls(clips)

    @classmethod
    def from_policy(cls, policy: WaveAugPolicy, seed: int = 0) -> "NoiseBank":
        return cls.synthetic(seed) if policy.noise == "synthetic" else cls.from_dir(policy.noise)


def kernels_cover(pcm: torch.Tensor) -> bool:
    """True if csrc/waveaug.hip's energy and apply kernels take ``pcm``."""
    return (pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.dim() == 2 and pcm.is_contiguous() and
            1 <= pcm.shape[0] <= MAX_B and 8 <= pcm.shape[1] <= MAX_S and pcm.shape[1] % 8 == 0 and
            pcm.data_ptr() % 16 == 0)


def _lens32(lens, dev) -> Optional[torch.Tensor]:
    if lens is None:
        return None
    lens = torch.as_tensor(lens).to(dev)
    if lens.dtype != torch.int32:
        lens = lens.to(torch.int32)
    return lens.contiguous()


def waveaug_plan(lens, B: int, S: int, bank: NoiseBank, policy: WaveAugPolicy, seed: int, step: int,
                 first_utt: int = 0, device=None) -> torch.Tensor:
    """plan int32 [B, 4] on ``device`` (kernel on a GPU, reference on the CPU)."""
    device = torch.device(device if device is not None else (lens.device if isinstance(lens, torch.Tensor) else "cpu"))
    if device.type != "cuda" or B < 1 or S < 1:
        return R.waveaug_plan_ref(lens, B, S, bank.length, policy, seed, step, first_utt).to(device)
    plan = torch.empty(B, 4, device=device, dtype=torch.int32)
    w = 0xffffffff
    _ext.ext().waveaug.plan(_lens32(lens, device), bank.on(device)[2], plan, S, policy.p_ppm, policy.snr_lo_cdb,
                            policy.snr_hi_cdb, seed & w, (seed >> 32) & w, step & w, (step >> 32) & w, first_utt & w)
    return plan


def waveaug_composite(pcm: torch.Tensor, lens, plan: torch.Tensor, bank: NoiseBank):
    """(y, energy, coef) of the definition in torch ops on pcm's device, from a plan: energies
    summed in fp64, the mix as a rounded product and a rounded sum."""
    dev = pcm.device
    B, S = pcm.shape
    data, start, length = bank.on(dev)
    x = pcm.to(torch.float32)
    n = torch.full((B,), S, device=dev, dtype=torch.int64) if lens is None else lens.to(dev).long().clamp(0, S)
    valid = torch.arange(S, device=dev)[None, :] < n[:, None]
    clip = plan[:, 1].long()
    idx = start.long()[clip][:, None] + (plan[:, 2].long()[:, None] + torch.arange(S, device=dev)[None, :]) % \
        length.long()[clip][:, None]
    z = data[idx]
    zero = torch.zeros((), device=dev, dtype=torch.float64)
    ex = torch.where(valid, x.double() ** 2, zero).sum(1)
    en = torch.where(valid, z.double() ** 2, zero).sum(1)
    energy = torch.stack([ex, en], 1)
    k = torch.sqrt(ex / (en * torch.pow(torch.full_like(ex, 10.0), plan[:, 3].double() / 1000.0))).to(torch.float32)
    on = plan[:, 0] != 0
    coef = torch.where(on & (ex != 0) & (en != 0) & torch.isfinite(k), k, torch.zeros((), device=dev))
    kz = coef[:, None] * z                               # a tensor of its own: never fused into an fma
    y = torch.where(on[:, None], x + kz, x)
    return torch.where(valid, y, torch.zeros((), device=dev)), energy, coef


class WaveAugment:
    """The waveform augmentation of a training run: ``aug(pcm, lens, step, first_utt) -> y``.
    ``plan`` int32 [B, 4], ``energy`` fp64 [B, 2] = (Ex, En) and ``coef`` fp32 [B] of the last call
    are kept."""

    def __init__(self, policy: WaveAugPolicy, bank: NoiseBank, seed: int):
        self.policy, self.bank, self.seed = policy, bank, int(seed)
        self.plan = self.energy = self.coef = None

    @torch.no_grad()
    def __call__(self, pcm: torch.Tensor, lens, step: int, first_utt: int = 0) -> torch.Tensor:
        if pcm.dim() != 2 or (lens is not None and torch.as_tensor(lens).numel() != pcm.shape[0]):
            raise ValueError("WaveAugment: pcm [B, S] and lens [B]")
        if pcm.dtype not in (torch.float32, torch.int16):
            raise ValueError("WaveAugment: pcm must be float32 or int16, not %s" % pcm.dtype)
        B, S = pcm.shape
        dev = pcm.device
        if B == 0 or S == 0:
            self.plan = self.energy = self.coef = None
            return pcm.to(torch.float32)
        step, first_utt = int(step), int(first_utt)
        if not pcm.is_cuda:
            y, self.plan, self.energy, self.coef = R.waveaug_ref(pcm, lens, self.bank, self.policy, self.seed, step,
                                                                 first_utt)
            return y
        lens = _lens32(lens, dev)
        self.plan = waveaug_plan(lens, B, S, self.bank, self.policy, self.seed, step, first_utt, device=dev)
        if not kernels_cover(pcm):
            y, self.energy, self.coef = waveaug_composite(pcm, lens, self.plan, self.bank)
            return y
        C = _ext.ext().waveaug
        data, start, length = self.bank.on(dev)
        part = torch.empty(B, (S + C.segment() - 1) // C.segment(), 2, device=dev, dtype=torch.float32)
        self.energy = torch.empty(B, 2, device=dev, dtype=torch.float64)
        self.coef = torch.empty(B, device=dev, dtype=torch.float32)
        y = torch.empty(B, S, device=dev, dtype=torch.float32)
        C.energy(pcm, lens, self.plan, data, start, length, part)
        C.coef(lens, self.plan, part, self.energy, self.coef, S)
        C.apply(pcm, lens, self.plan, self.coef, data, start, length, y)
        return y
