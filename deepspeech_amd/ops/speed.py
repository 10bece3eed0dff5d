"""Speed perturbation of training waveforms (csrc/speed.hip): every utterance of a batch is
resampled by its own ratio, the 0.9 / 1.0 / 1.1 recipe of speech recognisers trained from audio.
It changes lengths, so it acts first: speed, then noise (ops/waveaug.py), then the featurizer.

A policy is V distinct integer percents (``--speed_perturb 0.9,1.0,1.1`` is (90, 100, 110)),
1 <= V <= 8, each in 50 .. 200. Per utterance of pcm [B, S] with n = clamp(lens[b], 0, S):

    plan row  (pct, n_out) int32, one Philox4x32-10 block, key = seed, counter = (1, global
              utterance index u, step) on the noise plan's stream with first word 1;
              v = U(x0, V), U(x, m) = (x * m) >> 32, cand = ceil(n L_v / M_v) (n at 100 %);
              (100, n) instead when n == 0, cand < min_out[b] or cand > max_out (0: none)
    output    fp32 [B, S_out]: variant p != 100 is the polyphase Kaiser-sinc of ops/resample.py for
              the rates p -> 100, one fp32 fma chain in ascending k per output, bitwise
              ``Resampler(p, 100)`` on that row alone; 100 % is a bit copy (never the L = M = 1
              filter, which would low-pass); columns at or past n_out are +0, whatever the input
              holds past lens[b]
    S_out     a multiple of 160: ``speed_out_width`` (the worst case over the policy), or a
              smaller ``out_width`` from a caller that holds the lengths on the host
              (``speed_tight_width``); it is never derived by reading device memory

The plan is a pure function of (seed, step, u, n, min_out[b], max_out, policy), whatever the batch
size, the row, the world size or a resume. ops/reference.py holds the definition in integers and
fp64.

The kernels take contiguous, 16-byte aligned fp32 or int16 [B, S] on a GPU: two launches (plan,
apply) on the current stream, no host synchronisation. Anything else on a GPU takes the plan kernel
and the torch composite of the same definition, a CPU tensor the reference: slower, never silently
wrong.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _ext
from . import reference as R
from .resample import TILE_OUT, resample_composite

MAX_B, MAX_S = 65535, (1 << 30) - 1


@functools.lru_cache(maxsize=None)
def _variants(pcts: Tuple[int, ...]):
    """((pct, L, M, K, offset) per variant, the tables back to back as fp32, rounded once): a
    table starts on a 16-byte boundary; the identity has the record (100, 1, 1, 0, 0)."""
    recs, parts, off = [], [], 0
    for p in pcts:
        if p == 100:
            recs.append((100, 1, 1, 0, 0))
            continue
        L, M, K, h = R.resample_table(p, 100)
        h32 = np.ascontiguousarray(h, np.float32).reshape(-1)
        recs.append((p, L, M, K, off))
        pad = -h32.size % 4
        parts.append(np.concatenate([h32, np.zeros(pad, np.float32)]))
        off += h32.size + pad
    h = np.concatenate(parts) if parts else np.zeros(4, np.float32)
    return tuple(recs), torch.from_numpy(h)


@dataclass(frozen=True)
class SpeedPolicy:
    pcts: Tuple[int, ...] = (90, 100, 110)

    def __post_init__(self):
        p = self.pcts
        if not isinstance(p, tuple) or not 1 <= len(p) <= R.SPEED_MAX_V:
            raise ValueError("speed_perturb: 1 to %d factors, got %r" % (R.SPEED_MAX_V, p))
        for v in p:
            if not isinstance(v, int) or isinstance(v, bool) or not R.SPEED_MIN_PCT <= v <= R.SPEED_MAX_PCT:
                raise ValueError("speed_perturb: a factor lies in 0.5 .. 2.0 (an integer percent), got %r" % (v,))
        if len(set(p)) != len(p):
            raise ValueError("speed_perturb: repeated factor in %r" % (p,))

    @classmethod
    def parse(cls, spec: str) -> "SpeedPolicy":
        """"0.9,1.0,1.1": factors, each converted once to an integer percent."""
        pcts = []
        for item in spec.split(","):
            item = item.strip()
            if not item:
                raise ValueError("speed_perturb: empty item in %r" % (spec,))
            try:
                pcts.append(int(round(float(item) * 100)))
            except (ValueError, OverflowError):
                raise ValueError("speed_perturb: %r in %r is not a factor" % (item, spec)) from None
        return cls(tuple(pcts))

    def __str__(self) -> str:
        return ",".join("%g" % (p / 100.0) for p in self.pcts)

    @property
    def records(self):
        return _variants(self.pcts)[0]

    @property
    def vtab(self):
        """The records as the flat integer list the bindings take."""
        return [int(w) for rec in self.records for w in rec]

    @property
    def table(self) -> torch.Tensor:
        return _variants(self.pcts)[1]


def speed_out_width(S: int, policy) -> int:
    return R.speed_out_width(S, policy)


def speed_tight_width(plan) -> int:
    """The smallest multiple of 160 that holds every row's n_out of a plan held on the host."""
    plan = torch.as_tensor(plan)
    if plan.is_cuda:
        raise ValueError("speed_tight_width: the plan must be on the host (speed_plan_ref of a host copy of the lengths)")
    return R.speed_round_width(int(plan[:, 1].max()) if plan.numel() else 0)


def kernels_cover(pcm: torch.Tensor) -> bool:
    """True if csrc/speed.hip's apply kernel takes ``pcm``."""
    return (pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.dim() == 2 and pcm.is_contiguous() and
            1 <= pcm.shape[0] <= MAX_B and 1 <= pcm.shape[1] <= MAX_S and pcm.data_ptr() % 16 == 0)


def _i32(t, dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = torch.as_tensor(t).to(dev)
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t.contiguous()


_dev_tables = {}


def _table_on(policy: SpeedPolicy, dev) -> torch.Tensor:
    key = (policy.pcts, str(dev))
    if key not in _dev_tables:
        _dev_tables[key] = policy.table.to(dev)
    return _dev_tables[key]


def speed_plan(lens, B: int, S: int, policy: SpeedPolicy, seed: int, step: int, first_utt: int = 0, min_out=None,
               max_out: int = 0, device=None) -> torch.Tensor:
    """plan int32 [B, 2] on ``device`` (kernel on a GPU, reference on the CPU)."""
    device = torch.device(device if device is not None else (lens.device if isinstance(lens, torch.Tensor) else "cpu"))
    if device.type != "cuda" or B < 1 or S < 1:
        return R.speed_plan_ref(lens, B, S, policy, seed, step, first_utt, min_out, max_out).to(device)
    plan = torch.empty(B, 2, device=device, dtype=torch.int32)
    w = 0xffffffff
    _ext.ext().speed.plan(_i32(lens, device), _i32(min_out, device), plan, S, int(max_out), policy.vtab, seed & w,
                          (seed >> 32) & w, step & w, (step >> 32) & w, first_utt & w)
    return plan


def speed_composite(pcm: torch.Tensor, lens, plan: torch.Tensor, policy: SpeedPolicy, out_width: int):
    """(y fp32 [B, out_width], out_lens int32 [B]) of the definition in torch ops on pcm's device,
    from a plan: ``resample_composite`` once per variant over the whole batch, each row selected
    from its own variant (a rounded product and a rounded sum per tap where the kernel's fma has
    one rounding)."""
    dev = pcm.device
    B, S = pcm.shape
    W = int(out_width)
    n = torch.full((B,), S, device=dev, dtype=torch.int64) if lens is None else lens.to(dev).long().clamp(0, S)
    pct, cnt = plan[:, 0].long(), plan[:, 1].long().clamp(0, W)
    cnt = torch.where(pct == 100, torch.minimum(cnt, n), cnt)
    zero = torch.zeros((), device=dev, dtype=torch.float32)
    y = torch.zeros(B, W, device=dev, dtype=torch.float32)
    w0 = min(S, W)
    y[:, :w0] = pcm[:, :w0].to(torch.float32)                       # the identity; columns >= cnt go below
    table = _table_on(policy, dev)
    for p, L, M, K, off in policy.records:
        if p == 100:
            continue
        wp = min(W, R.resample_out_len(S, L, M))
        yp, _ = resample_composite(pcm, n, table[off:off + L * K].view(L, K), L, M, -(K // 2 - 1), 0, wp, True)
        if wp < W:
            yp = torch.cat([yp, torch.zeros(B, W - wp, device=dev, dtype=torch.float32)], 1)
        y = torch.where((pct == p)[:, None], yp, y)
    keep = torch.arange(W, device=dev)[None, :] < cnt[:, None]
    return torch.where(keep, y, zero), cnt.to(torch.int32)


class SpeedPerturb:
    """The speed perturbation of a training run:
    ``sp(pcm, lens, step, first_utt, min_out, max_out, out_width) -> (y, out_lens)``. ``plan`` int32
    [B, 2] of the last call is kept."""

    def __init__(self, policy: SpeedPolicy, seed: int):
        self.policy, self.seed = policy, int(seed)
        self.plan = None

    def out_width(self, S: int) -> int:
        return speed_out_width(S, self.policy)

    def tight_width(self, lens, B: int, S: int, step: int, first_utt: int = 0, min_out=None, max_out: int = 0) -> int:
        """The tight output width of a call, from host copies of ``lens`` and ``min_out``."""
        return speed_tight_width(R.speed_plan_ref(lens, B, S, self.policy, self.seed, int(step), int(first_utt), min_out,
                                                  max_out))

    @torch.no_grad()
    def __call__(self, pcm: torch.Tensor, lens, step: int, first_utt: int = 0, min_out=None, max_out: int = 0,
                 out_width: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if pcm.dim() != 2 or any(t is not None and torch.as_tensor(t).numel() != pcm.shape[0] for t in (lens, min_out)):
            raise ValueError("SpeedPerturb: pcm [B, S], lens [B] and min_out [B]")
        if not (pcm.dtype == torch.int16 or pcm.dtype.is_floating_point):
            raise ValueError("SpeedPerturb: pcm must be floating point or int16, not %s" % pcm.dtype)
        B, S = pcm.shape
        dev = pcm.device
        if B == 0 or S == 0:
            raise ValueError("SpeedPerturb: an empty batch, got %s" % (tuple(pcm.shape),))
        worst = self.out_width(S)
        if out_width is None:
            W, tight = worst, False
        else:
            W, tight = int(out_width), True
            if W < R.SPEED_HOP or W % R.SPEED_HOP != 0:
                raise ValueError("SpeedPerturb: out_width must be a positive multiple of %d, got %d" % (R.SPEED_HOP, W))
        step, first_utt, max_out = int(step), int(first_utt), int(max_out)
        if not pcm.is_cuda:
            self.plan = R.speed_plan_ref(lens, B, S, self.policy, self.seed, step, first_utt, min_out, max_out)
            return R.speed_ref(pcm, lens, self.plan, W)
        lens = _i32(lens, dev)
        self.plan = speed_plan(lens, B, S, self.policy, self.seed, step, first_utt, _i32(min_out, dev), max_out, device=dev)
        if not kernels_cover(pcm):
            return speed_composite(pcm, lens, self.plan, self.policy, W)
        C = _ext.ext().speed
        if C.tile() != TILE_OUT:
            raise RuntimeError("csrc/speed.hip and ops/resample.py disagree on the tile")
        y = torch.empty(B, W, device=dev, dtype=torch.float32)
        out_lens = torch.empty(B, device=dev, dtype=torch.int32)
        C.apply(pcm, lens, self.plan, _table_on(self.policy, dev), self.policy.vtab, y, out_lens, tight)
        return y, out_lens
