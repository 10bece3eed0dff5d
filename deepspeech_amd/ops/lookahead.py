"""Lookahead (row) convolution on the HIP engine (csrc/lookahead.hip).

Deep Speech 2 (section 3.7) gives a unidirectional model a little future context with a
per-feature convolution over the next tau outputs of the top recurrent layer. With time-major
h [T, B, H], w [H, tau+1], 1 <= tau <= 31, and valid(t, b) = t < min(lens[b], T):

    forward   r[t,b,i]  = valid(t,b) ? sum_{j=0..tau, valid(t+j,b)} w[i,j] h[t+j,b,i] : 0
    backward  dh[t,b,i] = valid(t,b) ? sum_{j=0..min(tau,t)} w[i,j] dr[t-j,b,i]       : 0
              dw[i,j]   = sum_b sum_{t : valid(t+j,b)} dr[t,b,i] h[t+j,b,i]

dr at invalid positions is ignored. Linear: no activation, no bias. Every kernel sums in ascending
j with fp32 FMAs, so the streaming kernel agrees bitwise with the whole-sequence one.

The kernels take bf16 [T, B, H] contiguous tensors with H % 8 == 0 and 16-byte aligned bases and
read w from the parameter's bf16 shadow. Anything else (another dtype or device, a
non-contiguous tensor, tau > 31, H % 8 != 0) takes the torch composite of the same definition
on the tensor's own device: slower, never silent garbage.
"""
from __future__ import annotations

import torch

from . import _ext
from . import reference as R
from .optim import arena_of

MAX_TAU = 31
_LDS_BYTES = 160 * 1024


def _lens32(lens: torch.Tensor, dev) -> torch.Tensor:
    lens = lens.to(dev)
    if lens.dtype != torch.int32:
        lens = lens.to(torch.int32)
    return lens.contiguous()


def _plain(t: torch.Tensor) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 3 and t.is_contiguous() and
            t.data_ptr() % 16 == 0 and t.shape[0] >= 1 and t.shape[1] >= 1)


def kernels_cover(x: torch.Tensor, w16: torch.Tensor) -> bool:
    """True if csrc/lookahead.hip takes activations ``x`` [T, B, H] with weights ``w16`` [H, tau+1]."""
    if not _plain(x) or w16.dim() != 2 or w16.shape[0] != x.shape[2]:
        return False
    H, tau = x.shape[2], w16.shape[1] - 1
    return (H % 8 == 0 and 1 <= tau <= MAX_TAU and (tau + 15) * H * 2 <= _LDS_BYTES and w16.is_cuda and
            w16.dtype == torch.bfloat16 and w16.is_contiguous() and w16.data_ptr() % 16 == 0)


def shadow_of(weight: torch.Tensor) -> torch.Tensor:
    """The bf16 weights the kernels read: the arena's shadow, or a cast of a free parameter."""
    if arena_of(weight) is not None:
        return weight.bf16
    return weight.detach().to(torch.bfloat16).contiguous()


# ---- torch composite (any dtype / device / layout): fp32 arithmetic of the same definition
def _composite_fwd(h, w16, lens):
    return R.lookahead_ref(h.float(), w16.float(), lens).to(h.dtype)


def _masked(x, lens):
    m = R.time_mask(lens.to(x.device), x.shape[0]).unsqueeze(-1)
    return torch.where(m, x.float(), torch.zeros((), device=x.device)), m


def _composite_bwd_data(dr, w16, lens):
    d, m = _masked(dr, lens)
    T = d.shape[0]
    w = w16.float()
    dh = torch.zeros_like(d)
    for j in range(min(w.shape[1], T)):
        term = w[:, j] * d[:T - j]
        dh = dh + (term if j == 0 else torch.nn.functional.pad(term, (0, 0, 0, 0, j, 0)))
    return torch.where(m, dh, torch.zeros((), device=d.device)).to(dr.dtype)


def _composite_bwd_weight(dr, h, lens, taps):
    d, _ = _masked(dr, lens)
    x, _ = _masked(h, lens)
    T = d.shape[0]
    cols = [(d[:T - j] * x[j:]).sum((0, 1)) if j < T else torch.zeros(d.shape[2], device=d.device)
            for j in range(taps)]
    return torch.stack(cols, 1)


def lookahead_fwd(h: torch.Tensor, w16: torch.Tensor, lens: torch.Tensor, out=None) -> torch.Tensor:
    """r [T, B, H] of the definition above (kernel where it covers the operands)."""
    if not kernels_cover(h, w16):
        r = _composite_fwd(h, w16, lens)
        return r if out is None else out.copy_(r)
    out = torch.empty_like(h) if out is None else out
    _ext.ext().lookahead(h, w16, _lens32(lens, h.device), out, False)
    return out


def lookahead_bwd_data(dr: torch.Tensor, w16: torch.Tensor, lens: torch.Tensor, out=None) -> torch.Tensor:
    if not kernels_cover(dr, w16):
        g = _composite_bwd_data(dr, w16, lens)
        return g if out is None else out.copy_(g)
    out = torch.empty_like(dr) if out is None else out
    _ext.ext().lookahead(dr, w16, _lens32(lens, dr.device), out, True)
    return out


def lookahead_bwd_weight(dr: torch.Tensor, h: torch.Tensor, lens: torch.Tensor, tau: int, out: torch.Tensor,
                         accumulate: bool = False) -> torch.Tensor:
    """dw into ``out`` (fp32 [H, tau+1], contiguous), written or accumulated. Two steps: one fp32
    partial [H, tau+1] per workgroup (batch rows summed in a fixed order through LDS), then
    col_sum over the partials in a fixed order: bitwise reproducible, no atomics."""
    if not (_plain(dr) and _plain(h) and dr.shape == h.shape and h.shape[2] % 8 == 0 and 1 <= tau <= MAX_TAU and
            out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
        g = _composite_bwd_weight(dr, h, lens, tau + 1)
        return out.add_(g) if accumulate else out.copy_(g)
    C = _ext.ext()
    T, B, H = h.shape
    P = int(C.lookahead_wgrad_parts(T, B, H))
    part = torch.empty(P, H * (tau + 1), device=h.device, dtype=torch.float32)
    C.lookahead_wgrad(dr, h, _lens32(lens, h.device), part, tau)
    C.col_sum([part.view(1, P, H * (tau + 1))], [out], [bool(accumulate)])
    return out


def lookahead_stream(hist: torch.Tensor, x: torch.Tensor, w16: torch.Tensor) -> torch.Tensor:
    """One streaming step: with s = [hist (tau frames); x (n frames)], out[k] = sum_j w[:,j] s[k+j]
    and ``hist`` is rewritten with the last tau frames of s. One launch, no host synchronisation,
    capturable. out[k] is the layer's output for the frame tau steps before x[k]."""
    if not (kernels_cover(x, w16) and _plain(hist) and hist.shape[0] == w16.shape[1] - 1 and
            hist.shape[1:] == x.shape[1:]):
        return _stream_composite(hist, x, w16)
    out = torch.empty_like(x)
    _ext.ext().lookahead_stream(hist, x, w16, out)
    return out


def _stream_composite(hist, x, w16):
    h32 = hist.to(torch.float32, copy=True)
    out = R.lookahead_stream_ref(h32, x.float(), w16.float())
    hist.copy_(h32)
    return out.to(x.dtype)


class LookaheadConv(torch.autograd.Function):
    """r = lookahead(h, w, lens); the weight gradient goes straight to the arena."""

    @staticmethod
    def forward(ctx, h, weight, lens):
        if arena_of(weight) is not None:
            arena_of(weight).await_params(weight)          # a carried optimizer update (Trainer)
        w16 = shadow_of(weight)
        h = h.contiguous()
        r = lookahead_fwd(h, w16, lens)
        ctx.save_for_backward(h, w16, lens)
        ctx.weight = weight
        return r

    @staticmethod
    def backward(ctx, dr):
        h, w16, lens = ctx.saved_tensors
        weight = ctx.weight
        dr = dr.to(h.dtype).contiguous()
        tau = w16.shape[1] - 1
        dh = lookahead_bwd_data(dr, w16, lens) if ctx.needs_input_grad[0] else None
        a = arena_of(weight)
        if a is not None:
            lookahead_bwd_weight(dr, h, lens, tau, weight.main_grad, accumulate=not a.first_write(weight))
            a.grad_done(weight)
            return dh, None, None
        if not ctx.needs_input_grad[1]:
            return dh, None, None
        gw = torch.empty(w16.shape, device=h.device, dtype=torch.float32)
        lookahead_bwd_weight(dr, h, lens, tau, gw)
        return dh, gw.to(weight.dtype), None
