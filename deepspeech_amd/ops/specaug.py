"""SpecAugment (Park et al., 2019) on stored feature frames (csrc/specaug.hip).

A policy is a time warp, nF frequency masks and nT time masks per utterance, on feats
[B, T, F] with seq_lens [B]; L = clamp(seq_lens[b], 0, T) and frames t >= L are never touched.

Randomness is counter based and stateless (Philox4x32-10, key = seed, counter = (block,
global utterance index u, step)): the plan of an utterance is a pure function of (seed, step,
u, L, T, F, policy), whatever the batch size, the row, the world size or a resume. A uniform
integer in [0, n) is (x * n) >> 32, so the device and ops/reference.py agree bit for bit.

    plan row  (w0, w, f0_0, fw_0, ..., t0_0, tw_0, ...) int32
    warp      n0 = L - 2W - 2; W == 0 or n0 < 1: identity (w0 = w = 0); else
              w0 = W + 1 + U(n0), w = U(2W + 1) - W: frame w0 moves to d0 = w0 + w in [1, L-2],
              the two sides stretch linearly: out[t] = x[i] + (r / den) (x[i+1] - x[i]) with
              (num, den, base) = (t w0, d0, 0) for t <= d0, ((t - d0)(L-1-w0), L-1-d0, w0) beyond,
              i = base + num // den, r = num % den; r == 0 is a bit copy
    freq k    fw = U(min(Fw, F) + 1), f0 = U(F - fw + 1)
    time k    c = min(Tw, L * p_ppm // 1000000), tw = U(c + 1), t0 = U(L - tw + 1)
    output    masks act on warped frame indices; a masked cell holds the fill (0, or the fp32
              mean of the utterance's unwarped bin over t < L) whatever the input holds there

The kernels take fp32 contiguous [B, T, F] with F <= 1024, T <= 32767 on a GPU: at most three
launches (plan, mean for fill = mean, apply) on the current stream, no host synchronisation.
Anything else on a GPU takes the plan kernel and the torch composite of the same definition, a
CPU tensor the reference: slower, never silently wrong.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _ext
from . import reference as R

MAX_NF, MAX_NT, MAX_F, MAX_T, MAX_B = 8, 16, 1024, 32767, 65535
PRESETS = {
    "ld": "W=80,F=27,nF=2,T=100,nT=2,p=1.0",
    "ls": "W=40,F=15,nF=2,T=70,nT=2,p=0.2",
}
_SPEC_KEYS = {"F": "Fw", "nF": "nF", "T": "Tw", "nT": "nT", "W": "W"}


@dataclass(frozen=True)
class SpecAugPolicy:
    nF: int = 0             # frequency masks
    Fw: int = 0             # maximum frequency mask width
    nT: int = 0             # time masks
    Tw: int = 0             # maximum time mask width
    p_ppm: int = 1000000    # cap of one time mask as a share of the utterance, parts per million
    W: int = 0              # time-warp parameter, 0 = no warp
    fill: str = "mean"      # value of masked cells: mean | zero

    def __post_init__(self):
        for name in ("nF", "Fw", "nT", "Tw", "p_ppm", "W"):
            v = getattr(self, name)
            if not isinstance(v, int) or isinstance(v, bool) or v < 0 or v >= 1 << 30:
                raise ValueError("SpecAugment: %s must be an integer in [0, 2^30), not %r" % (name, v))
        if self.nF > MAX_NF or self.nT > MAX_NT:
            raise ValueError("SpecAugment: nF <= %d and nT <= %d" % (MAX_NF, MAX_NT))
        if self.p_ppm > 1000000:
            raise ValueError("SpecAugment: p must lie in [0, 1]")
        if self.fill not in ("mean", "zero"):
            raise ValueError("SpecAugment: fill is mean or zero, not %r" % (self.fill,))

    @property
    def empty(self) -> bool:
        """Nothing to do: no mask can be drawn (a mask of width 0 is still a draw) and no warp."""
        return self.nF == 0 and self.nT == 0 and self.W == 0

    @property
    def plan_width(self) -> int:
        return 2 + 2 * self.nF + 2 * self.nT

    @classmethod
    def parse(cls, spec: str) -> "SpecAugPolicy":
        """A preset name (ld, ls) or "F=27,nF=2,T=100,nT=2,p=0.2,W=0,fill=mean" (any subset; p is
        converted once to integer parts per million)."""
        spec = PRESETS.get(spec.strip(), spec.strip())
        kw = {}
        for item in filter(None, (s.strip() for s in spec.split(","))):
            key, sep, val = item.partition("=")
            key, val = key.strip(), val.strip()
            if not sep or key in kw:
                raise ValueError("SpecAugment: bad or repeated item %r in %r" % (item, spec))
            if key in _SPEC_KEYS:
                kw[key] = int(val)
            elif key == "p":
                kw[key] = int(round(float(val) * 1000000))
            elif key == "fill":
                kw[key] = val
            else:
                raise ValueError("SpecAugment: unknown key %r in %r (F, nF, T, nT, p, W, fill)" % (key, spec))
        args = {_SPEC_KEYS[k]: v for k, v in kw.items() if k in _SPEC_KEYS}
        if "p" in kw:
            args["p_ppm"] = kw["p"]
        if "fill" in kw:
            args["fill"] = kw["fill"]
        return cls(**args)

    def __str__(self) -> str:
        return "F=%d,nF=%d,T=%d,nT=%d,p=%g,W=%d,fill=%s" % (self.Fw, self.nF, self.Tw, self.nT, self.p_ppm / 1e6,
                                                          self.W, self.fill)


def _lens32(lens: torch.Tensor, dev) -> torch.Tensor:
    lens = lens.to(dev)
    if lens.dtype != torch.int32:
        lens = lens.to(torch.int32)
    return lens.contiguous()


def kernels_cover(feats: torch.Tensor) -> bool:
    """True if csrc/specaug.hip's mean and apply kernels take ``feats``."""
    return (feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 3 and feats.is_contiguous() and
            1 <= feats.shape[0] <= MAX_B and 1 <= feats.shape[1] <= MAX_T and 1 <= feats.shape[2] <= MAX_F)


def specaug_plan(lens: torch.Tensor, T: int, F: int, policy: SpecAugPolicy, seed: int, step: int,
                 first_utt: int = 0) -> torch.Tensor:
    """plan int32 [B, 2 + 2 nF + 2 nT] on lens' device (kernel on a GPU, reference on the CPU)."""
    if not lens.is_cuda or lens.numel() == 0 or T < 1 or F < 1:
        return R.specaug_plan_ref(lens, T, F, policy, seed, step, first_utt)
    lens = _lens32(lens, lens.device)
    plan = torch.empty(lens.numel(), policy.plan_width, device=lens.device, dtype=torch.int32)
    w = 0xffffffff
    _ext.ext().specaug_plan(lens, plan, T, F, policy.nF, policy.Fw, policy.nT, policy.Tw, policy.p_ppm, policy.W,
                            seed & w, (seed >> 32) & w, step & w, (step >> 32) & w, first_utt & w)
    return plan


def specaug_mean(feats: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """fp32 mean [B, F] over frames t < L of each utterance (0 for L == 0), on feats' device."""
    if kernels_cover(feats):
        mean = torch.empty(feats.shape[0], feats.shape[2], device=feats.device, dtype=torch.float32)
        _ext.ext().specaug_mean(feats, _lens32(lens, feats.device), mean)
        return mean
    if not feats.is_cuda:
        return R.specaug_mean_ref(feats.float(), lens)
    T = feats.shape[1]
    L = lens.to(feats.device).long().clamp(0, T)
    valid = torch.arange(T, device=feats.device)[None, :] < L[:, None]
    s = torch.where(valid[:, :, None], feats.float(), torch.zeros((), device=feats.device)).sum(1)
    return torch.where(L[:, None] > 0, s / L.clamp(min=1)[:, None].float(), torch.zeros((), device=feats.device))


def specaug_apply(feats: torch.Tensor, lens: torch.Tensor, plan: torch.Tensor, fill: Optional[torch.Tensor],
                  nF: int, inplace: bool = False) -> torch.Tensor:
    """feats under ``plan`` (nF of its masks are frequency masks); fill [B, F] fp32 or None for
    zeros. inplace (plans without a warp only): feats itself is rewritten and returned."""
    if feats.numel() == 0:
        return feats
    if not kernels_cover(feats):
        out = R.specaug_apply_ref(feats, lens, plan, fill, nF)
        return feats.copy_(out) if inplace else out
    nT = (plan.shape[1] - 2 - 2 * nF) // 2
    plan = plan.to(feats.device, torch.int32).contiguous()
    out = feats if inplace else torch.empty_like(feats)
    _ext.ext().specaug_apply(feats, _lens32(lens, feats.device), plan, fill, out, nF, nT, inplace)
    return out


class SpecAugment:
    """The augmentation of a training run: ``aug(feats, seq_lens, step, first_utt)``."""

    def __init__(self, policy: SpecAugPolicy, seed: int):
        self.policy = policy
        self.seed = int(seed)

    @torch.no_grad()
    def __call__(self, feats: torch.Tensor, seq_lens: torch.Tensor, step: int, first_utt: int = 0,
                 inplace: bool = False, return_plan: bool = False):
        p = self.policy
        if inplace and p.W > 0:
            raise ValueError("SpecAugment: a time warp (W > 0) cannot run in place")
        if p.empty:
            return (feats, None) if return_plan else feats
        if feats.dim() != 3 or seq_lens.numel() != feats.shape[0]:
            raise ValueError("SpecAugment: feats [B, T, F] and seq_lens [B]")
        lens = _lens32(seq_lens, feats.device)
        plan = specaug_plan(lens, feats.shape[1], feats.shape[2], p, self.seed, int(step), int(first_utt))
        fill = specaug_mean(feats, lens) if p.fill == "mean" else None
        out = specaug_apply(feats, lens, plan, fill, p.nF, inplace=inplace)
        return (out, plan) if return_plan else out
