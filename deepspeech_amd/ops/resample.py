"""Sample-rate conversion of raw PCM in front of the featurizer.

``Resampler(in_rate, out_rate)`` converts [B, S] PCM (float32 or int16) to ``out_rate`` with the
polyphase Kaiser-windowed sinc of ``ops/reference.py`` (``resample_table``, ``resample_ref``):
with L = out / gcd and M = in / gcd, output n is one chain of K fp32 fma in ascending k over
``h[n M % L, k] * x[n M // L - (K/2 - 1) + k]``, samples outside a row read as +0. On a GPU inside
the kernel's contract (``L * K <= 24576`` table words, ``K <= 320``) that is one launch of
``csrc/resample.hip``; anything else, and every CPU device, takes a torch composite of the same
definition (gather, then multiply and add in ascending k; two roundings per tap where the kernel's
fma has one, so the two agree to the rounding bound, not bitwise).

``Resampler.stream(B)`` converts audio as it arrives. An output is emitted once its last tap has
arrived (``K/2`` input samples of latency), computed from exactly the values the whole call
reads, so the concatenated stream is bitwise the whole-call result for any chunking. The
counters are Python ints; the device sees a buffer-relative offset and a start phase.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .reference import resample_emitted, resample_out_len, resample_table

TILE_OUT = 1024                # outputs per workgroup tile of csrc/resample.hip (checked at load)

PcmLike = Union[torch.Tensor, np.ndarray, Sequence]


def pack_pcm(pcm: PcmLike, lens, float_dtype: torch.dtype, pin: bool):
    """-> (tensor [B, S] where it already lives, or on the host for a list; lens or None). int16
    stays int16; anything else becomes ``float_dtype``. A list of 1-D utterances is zero-padded
    and implies ``lens``."""
    if isinstance(pcm, torch.Tensor) or (isinstance(pcm, np.ndarray) and pcm.ndim == 2):
        t = pcm if isinstance(pcm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pcm))
        if t.dim() != 2:
            raise ValueError("pcm must be [B, S] or a list of 1-D arrays")
        if t.dtype != torch.int16:
            t = t.to(float_dtype)
        if lens is not None:
            lens = torch.as_tensor(lens, dtype=torch.int32)
        return t, lens
    if lens is not None:
        raise ValueError("lens is implied by a list of utterances")
    arrs = [u.detach().cpu().numpy() if isinstance(u, torch.Tensor) else np.asarray(u) for u in pcm]
    if not arrs or any(a.ndim != 1 or a.size == 0 for a in arrs):
        raise ValueError("pcm must be a non-empty list of non-empty 1-D arrays")
    i16 = all(a.dtype == np.int16 for a in arrs)
    B, S = len(arrs), max(a.size for a in arrs)
    buf = torch.zeros(B, S, dtype=torch.int16 if i16 else float_dtype, pin_memory=pin)
    view = buf.numpy()
    for b, a in enumerate(arrs):
        view[b, :a.size] = a
    return buf, torch.tensor([a.size for a in arrs], dtype=torch.int32)


def resample_composite(x: torch.Tensor, lens: Optional[torch.Tensor], h: torch.Tensor, L: int, M: int,
                       in_off: int, ph0: int, n_out: int, to_end: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernel's launch in torch ops on x's device: x [B, S] fp32 / int16, h fp32 [L, K]; output
    j reads x[in_off + (ph0 + j M) // L + k] against h[(ph0 + j M) % L, k], out-of-row samples
    selected to +0, accumulated from +0 in ascending k (a rounded product, then a rounded sum)."""
    B, S = x.shape
    K = h.shape[1]
    dev = x.device
    n_out = int(n_out)
    if lens is None:
        ln = torch.full((B,), S, dtype=torch.int64, device=dev)
    else:
        ln = lens.to(dev, torch.int64).clamp(0, S)
    if to_end:
        num = (ln - (in_off + K // 2 - 1)) * L - ph0
        cnt = torch.where(num <= 0, torch.zeros_like(num), (num + (M - 1)) // M).clamp(max=n_out)
    else:
        cnt = torch.full((B,), n_out, dtype=torch.int64, device=dev)
    t = ph0 + torch.arange(n_out, dtype=torch.int64, device=dev) * M
    q, ph = t // L, t % L
    xf = x.to(torch.float32)
    hT = h.t().contiguous()                                        # [K, L]
    acc = torch.zeros(B, n_out, dtype=torch.float32, device=dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    if S > 0 and n_out > 0:
        for k in range(K):
            idx = q + (in_off + k)
            ok = (idx >= 0)[None, :] & (idx[None, :] < ln[:, None])
            v = torch.where(ok, xf[:, idx.clamp(0, S - 1)], zero)
            acc = torch.add(acc, torch.mul(v, hT[k][ph][None, :]))
    keep = torch.arange(n_out, device=dev)[None, :] < cnt[:, None]
    return torch.where(keep, acc, zero), cnt.to(torch.int32)


_tables: Dict[tuple, tuple] = {}


def _table(in_rate: int, out_rate: int, device: torch.device):
    key = (in_rate, out_rate, str(device))
    t = _tables.get(key)
    if t is None:
        L, M, K, h = resample_table(in_rate, out_rate)
        t = (L, M, K, torch.from_numpy(np.ascontiguousarray(h, np.float32)).to(device))   # rounded once
        _tables[key] = t
    return t


class Resampler:
    """PCM [B, S] at ``in_rate`` -> (y [B, N(S)] fp32, out_lens [B] int32) at ``out_rate`` on
    ``device``, N(S) = ceil(S L / M). Columns at or past a row's count are exact zeros; nothing at
    or past ``lens[b]`` (garbage, NaN) reaches an output. Output is in the input's units (int16
    input is not rescaled and not rounded back)."""

    def __init__(self, in_rate: int, out_rate: int = 16000, device=None):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.identity = self.in_rate == self.out_rate
        self.L, self.M, self.K, self.h = _table(self.in_rate, self.out_rate, self.device)
        self.use_kernel = False
        if self.device.type == "cuda" and not self.identity:
            from . import _ext
            self._C = _ext.ext()                     # raises if the extension is not built
            if self._C.resample_tile() != TILE_OUT:
                raise RuntimeError("csrc/resample.hip and ops/resample.py disagree on the tile")
            self.use_kernel = bool(self._C.resample_supported(self.L, self.M, self.K))   # the contract

    def out_len(self, n_samples: int) -> int:
        return int(n_samples) if self.identity else resample_out_len(n_samples, self.L, self.M)

    def _pack(self, pcm: PcmLike, lens):
        return pack_pcm(pcm, lens, torch.float32, self.device.type == "cuda")

    def _run(self, x: torch.Tensor, lens, in_off: int, ph0: int, n_out: int, to_end: bool):
        """One launch (or the composite) on device tensors."""
        if self.use_kernel:
            B = x.shape[0]
            out = torch.empty(B, n_out, dtype=torch.float32, device=self.device)
            out_lens = torch.empty(B, dtype=torch.int32, device=self.device)
            self._C.resample(x.contiguous(), lens, self.h, self.L, self.M, in_off, ph0, to_end, out, out_lens)
            return out, out_lens
        return resample_composite(x, lens, self.h, self.L, self.M, in_off, ph0, n_out, to_end)

    @torch.no_grad()
    def __call__(self, pcm: PcmLike, lens=None) -> Tuple[torch.Tensor, torch.Tensor]:
        x, lens = self._pack(pcm, lens)
        x = x.to(self.device, non_blocking=True)
        if lens is not None:
            lens = lens.to(self.device, non_blocking=True)
        B, S = x.shape
        if self.identity:                            # no launch
            if lens is None:
                lens = torch.full((B,), S, dtype=torch.int32, device=self.device)
            return x.to(torch.float32), lens
        return self._run(x, lens, -(self.K // 2 - 1), 0, self.out_len(S), True)

    def stream(self, batch: int) -> "ResampleStream":
        """State of ``batch`` concurrent streams that share one chunk schedule."""
        return ResampleStream(self, batch)


class ResampleStream:
    """Incremental resampling. ``push(chunk)`` returns the outputs that became complete,
    [B, E_new]: after P input samples exactly ``resample_emitted(P)`` outputs exist, those whose
    last tap has arrived. ``push(chunk, final=True)`` emits the rest, the missing samples read as
    zero, so a row's total is N(its length); ``last_lens`` then holds each row's valid count of
    that push. The state is the unconsumed input tail plus absolute counters (Python ints)."""

    def __init__(self, rs: Resampler, batch: int):
        self.rs, self.B = rs, int(batch)
        self.buf: Optional[torch.Tensor] = None      # [B, tail] raw samples from absolute index `base`
        self.base = 0                                # absolute input index of buf[:, 0]
        self.received = 0                            # input samples so far
        self.emitted = 0                             # outputs so far
        self.finished = False
        self.last_lens: Optional[torch.Tensor] = None

    @torch.no_grad()
    def push(self, chunk, final: bool = False, lens=None) -> torch.Tensor:
        """Feed [B, S_c] samples. ``lens`` ([B] valid samples of this chunk) is accepted only with
        ``final=True``, where streams may end at different samples."""
        rs = self.rs
        if self.finished:
            raise RuntimeError("stream already finished")
        if lens is not None and not final:
            raise ValueError("lens is only meaningful with final=True")
        chunk, lens = rs._pack(chunk, lens)
        if chunk.shape[0] != self.B:
            raise ValueError("chunk must be [%d, S_c]" % self.B)
        chunk = chunk.to(rs.device)
        if self.buf is None:
            self.buf = chunk
        else:
            if chunk.dtype != self.buf.dtype:
                raise ValueError("a stream's chunks must share one dtype")
            self.buf = torch.cat([self.buf, chunk], 1)
        self.received += chunk.shape[1]
        if lens is not None:                         # valid samples of the buffer
            lens = (lens.to(rs.device) + (self.buf.shape[1] - chunk.shape[1])).to(torch.int32)
        if final:
            self.finished = True
        if rs.identity:
            out, self.buf = self.buf.to(torch.float32), None
            self.base = self.received
            self.emitted += out.shape[1]
            if final:
                self.last_lens = lens if lens is not None else torch.full(
                    (self.B,), out.shape[1], dtype=torch.int32, device=rs.device)
            return out
        L, M, K = rs.L, rs.M, rs.K
        total = rs.out_len(self.received) if final else resample_emitted(self.received, L, M, K)
        e_new = total - self.emitted
        if e_new <= 0 and not final:
            return torch.zeros(self.B, 0, dtype=torch.float32, device=rs.device)
        t0 = self.emitted * M                        # exact: Python ints
        i0, ph0 = t0 // L, t0 % L
        in_off = i0 - (K // 2 - 1) - self.base
        out, out_lens = rs._run(self.buf, lens, in_off, ph0, max(e_new, 0), final)
        self.emitted = total
        if final:
            self.last_lens = out_lens
            self.buf = None
        else:                                        # keep from tap 0 of the next output
            nxt = (self.emitted * M) // L - (K // 2 - 1)
            drop = max(0, nxt - self.base)
            self.buf = self.buf[:, drop:]
            self.base += drop
        return out
