"""Dropout between stacked recurrent layers (csrc/dropout.hip).

x [T, N, H], time-major, is the tensor one recurrent layer hands to the next. The mask is never
stored: forward and backward regenerate it from (seed, step, utterance, frame, unit, site) with
the counter-based Philox4x32-10 that SpecAugment uses, so it does not depend on the batch size,
the row, the world size or a resume, and ops/reference.py seq_dropout_mask_ref gives the same
bits in integer arithmetic.

    thr     clamp(round(p * 65536), 0, 65535); the drop probability is exactly thr / 65536 and
            thr == 0 is no op at all (the input object comes back, no launch, no autograd node)
    scale   fp32(65536) / fp32(65536 - thr)
    block   key = seed, counter = (t or 0 when locked, first_utt + b, step,
            0x80000000 | locked << 30 | site << 16 | i >> 3) serves units 8 g .. 8 g + 7
    keep    r = (x[e >> 1] >> (16 * (e & 1))) & 0xffff >= thr, e = i & 7
    output  kept: bf16(float(x) * scale); dropped: +0 by selection (an inf or NaN does not survive)
    mode    element: one draw per (frame, utterance, unit); locked: one per (utterance, unit),
            shared by all frames

step and first_utt live in a device int32[2] tensor (DropoutState.ctr) that the kernel reads,
so a captured training step replays with the current step's mask. The kernel takes bf16
contiguous [T, N, H] with H % 8 == 0 on a GPU; anything else (fp32, H % 8 != 0, a
non-contiguous view, a CPU tensor) takes the torch composite of the same definition, which
reads ctr on the host: slower, never silently different.
"""
from __future__ import annotations

import torch

from . import _ext
from . import reference as R

MODES = ("element", "locked")
MAX_SITE = 16384

threshold = R.seq_dropout_threshold
scale_of = R.seq_dropout_scale


class DropoutState:
    """Owner of ``ctr`` = (step, first_utt) mod 2^32, int32 [2] on ``device``."""

    def __init__(self, device):
        self.ctr = torch.zeros(2, dtype=torch.int32, device=device)

    def set(self, step: int, first_utt: int = 0) -> None:
        """Write ctr on the current stream, without a host synchronisation; never called inside a
        graph capture. On a GPU it is one csrc/fill.hip multi_fill launch whose two patterns are
        kernel arguments (a pinned staging buffer would have to outlive a host that runs ahead)."""
        s, u = int(step) & 0xffffffff, int(first_utt) & 0xffffffff
        if self.ctr.is_cuda:
            _ext.ext().multi_fill([self.ctr[0:1], self.ctr[1:2]], [s, u])
        else:
            self.ctr[0] = s - (1 << 32) if s >= 1 << 31 else s
            self.ctr[1] = u - (1 << 32) if u >= 1 << 31 else u

    def get(self):
        """(step, first_utt) as unsigned 32-bit values: a host read (synchronises a GPU)."""
        s, u = self.ctr.tolist()
        return s & 0xffffffff, u & 0xffffffff


def kernel_covers(x: torch.Tensor, ctr: torch.Tensor) -> bool:
    """True if csrc/dropout.hip takes ``x`` with ``ctr``."""
    return (x.is_cuda and ctr.is_cuda and ctr.device == x.device and x.dtype == torch.bfloat16 and x.dim() == 3 and
            x.is_contiguous() and x.numel() > 0 and x.shape[2] % 8 == 0 and x.shape[2] <= 8 * 65536 and
            x.numel() // 8 < 1 << 31 and x.data_ptr() % 16 == 0)


def _apply(x: torch.Tensor, ctr: torch.Tensor, seed: int, site: int, thr: int, locked: bool,
           inplace: bool) -> torch.Tensor:
    if x.numel() == 0:
        return x
    if kernel_covers(x, ctr):
        out = x if inplace else torch.empty_like(x)
        _ext.ext().seq_dropout(x, out, ctr, seed & 0xffffffff, (seed >> 32) & 0xffffffff, site, thr, scale_of(thr),
                               locked)
        return out
    s, u = ctr.tolist()
    return R.seq_dropout_ref(x, seed, s & 0xffffffff, u & 0xffffffff, site, thr, locked)


class SeqDropout(torch.autograd.Function):
    """y = dropout(x); backward regenerates the mask from ctr and the launch constants (nothing
    else is kept). grad_inplace: the incoming gradient is a fresh tensor nobody else reads (the dx
    a recurrent layer's projection GEMM produced) and is rewritten in place."""

    @staticmethod
    def forward(ctx, x, ctr, seed: int, site: int, thr: int, locked: bool, grad_inplace: bool = False):
        ctx.ctr = ctr
        ctx.consts = (seed, site, thr, locked, grad_inplace)
        return _apply(x, ctr, seed, site, thr, locked, False)

    @staticmethod
    def backward(ctx, dy):
        seed, site, thr, locked, grad_inplace = ctx.consts
        return _apply(dy, ctx.ctr, seed, site, thr, locked, grad_inplace), None, None, None, None, None, None


def seq_dropout(x: torch.Tensor, state: DropoutState, seed: int, site: int, thr: int, mode: str = "element",
                grad_inplace: bool = False) -> torch.Tensor:
    """x [T, N, H] under the dropout mask of (seed, state.ctr, site, thr, mode); thr == 0: x itself."""
    thr, site, seed = int(thr), int(site), int(seed)
    if mode not in MODES:
        raise ValueError("dropout mode is element or locked, not %r" % (mode,))
    if not 0 <= thr <= 65535 or not 0 <= site < MAX_SITE or not 0 <= seed < 1 << 64:
        raise ValueError("seq_dropout: thr in [0, 65535], site in [0, 16384), seed in [0, 2^64)")
    if thr == 0:
        return x
    if x.dim() != 3:
        raise ValueError("seq_dropout: x [T, N, H]")
    return SeqDropout.apply(x, state.ctr, seed, site, thr, mode == "locked", grad_inplace)
