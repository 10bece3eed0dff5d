"""Audio in: batched and streaming featurization of raw PCM.

``AudioFeaturizer`` turns PCM (float32 or int16) into the [B, T, 161] feature frames the
model consumes, for both feature kinds of ``data/featurizer.py`` (``mfcc``, ``spectrogram``).
On a GPU at 16 kHz it runs the HIP kernels of ``csrc/featurize.hip`` (a missing extension is
an error, never a silent fallback); on a CPU device, or at another sample rate, it computes
with ``data/featurizer.py`` itself, so the interface works everywhere. That numpy module stays
the fp64 oracle: every table the kernels consume is derived here from its formulas in fp64 and
rounded to fp32 once. Audio recorded at another rate reaches the kernels through
``input_rate``: it is resampled to ``sample_rate`` first (``ops/resample.py``), on the device.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ..data import featurizer as F
from .resample import Resampler, pack_pcm

HOP = 160                      # 10 ms at 16 kHz
FRAME_LEN = {"mfcc": 400, "spectrogram": 320}
NUM_FEATURES = 161
NFILT, NFFT, MEL_TAPS, DCT_LD, LIFTER = 322, 512, 8, 192, 22
KERNEL_RATE = 16000
_KIND_ID = {"mfcc": 0, "spectrogram": 1}


def num_frames(n_samples: int, kind: str = "mfcc") -> int:
    """Frames of an ``n_samples`` signal (the last one zero-padded), as ``featurizer._frames``."""
    L = FRAME_LEN[kind]
    n = int(n_samples)
    return 1 if n <= L else 1 + int(math.ceil((n - L) / float(HOP)))


def _stream_frames(n: int, kind: str, mode: int) -> int:
    """Frame count of the kernels' three modes (csrc/featurize.hip frame_count)."""
    L = FRAME_LEN[kind]
    if mode == 1:                                   # stream in flight: complete frames only
        return 0 if n < L else 1 + (n - L) // HOP
    if mode == 2 and n <= L - HOP:                  # stream end: nothing new to cover
        return 0
    return num_frames(n, kind)


# ---- tables (fp64; the device gets them rounded to fp32 once) ---------------------------------
def dft_basis(kind: str) -> np.ndarray:
    """Packed real-DFT basis [L, 2 * NH] of the zero-padded frame: columns [0, NH) are cos of
    bins 0 .. NH-1, column NH is cos of the Nyquist bin NH (whose sin, like bin 0's, is 0) and
    column NH + c is sin of bin c. The spectrogram's Hamming window is folded into the rows."""
    L = FRAME_LEN[kind]
    nfft = NFFT if kind == "mfcc" else L
    nh = nfft // 2
    n = np.arange(L, dtype=np.int64)[:, None]
    c = np.arange(nh, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * c) % nfft).astype(np.float64) / nfft       # exact phase reduction
    basis = np.empty((L, 2 * nh), np.float64)
    basis[:, :nh] = np.cos(ang)
    basis[:, nh:] = np.sin(ang)
    basis[:, nh] = np.where(n[:, 0] % 2 == 0, 1.0, -1.0)
    if kind == "spectrogram":
        basis *= np.hamming(L)[:, None]
    return basis


def power_from_dft(y: np.ndarray, kind: str) -> np.ndarray:
    """[T, 2 * NH] packed DFT output -> [T, NH + 1] power spectrum (mfcc: / nfft)."""
    nh = y.shape[-1] // 2
    p = np.empty(y.shape[:-1] + (nh + 1,), y.dtype)
    p[..., 1:nh] = y[..., 1:nh] ** 2 + y[..., nh + 1:] ** 2
    p[..., 0] = y[..., 0] ** 2
    p[..., nh] = y[..., nh] ** 2
    return p / NFFT if kind == "mfcc" else p


def mel_table(sample_rate: int = KERNEL_RATE) -> Tuple[np.ndarray, np.ndarray]:
    """Banded form of ``mel_filterbank(322, 512, sr)``: idx [322, 2] = (first bin, taps) and
    w [322, 8]. Empty filters (117 of them at 16 kHz) have 0 taps."""
    fb = F.mel_filterbank(NFILT, NFFT, sample_rate)
    idx = np.zeros((NFILT, 2), np.int32)
    w = np.zeros((NFILT, MEL_TAPS), np.float64)
    for j in range(NFILT):
        nz = np.nonzero(fb[j])[0]
        if nz.size == 0:
            continue
        # the kernel always reads MEL_TAPS bins from `first` (weights past the taps are zero), so
        # the window must end inside the 257 bins
        first = min(int(nz[0]), NFFT // 2 + 1 - MEL_TAPS)
        taps = int(nz[-1]) - first + 1
        if taps > MEL_TAPS:
            raise ValueError("mel filter %d spans %d bins (table holds %d)" % (j, taps, MEL_TAPS))
        idx[j] = (first, taps)
        w[j, :taps] = fb[j, first:first + taps]
    return idx, w


def expand_mel(idx: np.ndarray, w: np.ndarray) -> np.ndarray:
    fb = np.zeros((NFILT, NFFT // 2 + 1), w.dtype)
    for j in range(NFILT):
        first, taps = int(idx[j, 0]), int(idx[j, 1])
        fb[j, first:first + taps] = w[j, :taps]
    return fb


def dct_table() -> np.ndarray:
    """Orthonormal DCT-II of 322 inputs, first 161 outputs, as [322, 192] (columns >= 161 zero):
    ``_dct2_ortho`` with its scale folded in."""
    k = np.arange(NFILT, dtype=np.float64)
    c = np.arange(NUM_FEATURES, dtype=np.float64)
    t = np.cos(np.pi * (2 * k[:, None] + 1) * c[None, :] / (2.0 * NFILT))
    t[:, 0] *= math.sqrt(1.0 / (4 * NFILT)) * 2
    t[:, 1:] *= math.sqrt(1.0 / (2 * NFILT)) * 2
    out = np.zeros((NFILT, DCT_LD), np.float64)
    out[:, :NUM_FEATURES] = t
    return out


def lifter_table() -> np.ndarray:
    n = np.arange(NUM_FEATURES)
    return 1 + (LIFTER / 2.0) * np.sin(np.pi * n / LIFTER)


def frame_signal(sig: np.ndarray, kind: str) -> np.ndarray:
    """[T, L] frames of a (normalised) signal, pre-emphasised for mfcc: the A operand of the DFT."""
    sig = np.asarray(sig)
    if kind == "mfcc":
        sig = np.append(sig[0], sig[1:] - sig.dtype.type(0.97) * sig[:-1])
    return F._frames(sig, FRAME_LEN[kind], HOP).astype(sig.dtype)


def features_from_tables(sig: np.ndarray, kind: str, dtype=np.float64) -> np.ndarray:
    """The kernels' formulation in numpy at ``dtype``: frames @ basis, banded mel, log, DCT table,
    lifter, c0 = log energy. In fp64 it equals ``featurizer.mfcc`` / ``spectrogram`` to rounding; in
    fp32 it shows what single precision costs against that oracle."""
    dt = np.dtype(dtype).type
    fr = frame_signal(np.asarray(sig, dtype), kind)
    p = power_from_dft(fr @ dft_basis(kind).astype(dtype), kind)
    if kind == "spectrogram":
        return np.log(p + dt(1e-14))
    eps = dt(np.finfo(float).eps)
    energy = p.sum(1)
    energy = np.where(energy == 0, eps, energy)
    idx, w = mel_table()
    w = w.astype(dtype)
    feat = np.zeros((p.shape[0], NFILT), dtype)
    for t in range(MEL_TAPS):
        on = idx[:, 1] > t
        feat[:, on] += p[:, idx[on, 0] + t] * w[on, t]
    feat = np.where(feat == 0, eps, feat)
    cep = (np.log(feat) @ dct_table().astype(dtype))[:, :NUM_FEATURES] * lifter_table().astype(dtype)
    cep[:, 0] = np.log(energy)
    return cep


_device_tables: Dict[tuple, dict] = {}


def _tables(kind: str, sample_rate: int, device: torch.device) -> dict:
    key = (kind, sample_rate, str(device))
    t = _device_tables.get(key)
    if t is None:
        def f32(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
        t = {"basis": f32(dft_basis(kind)), "mel_idx": None, "mel_w": None, "dct": None, "lifter": None}
        if kind == "mfcc":
            idx, w = mel_table(sample_rate)
            t.update(mel_idx=torch.from_numpy(idx).to(device), mel_w=f32(w), dct=f32(dct_table()),
                     lifter=f32(lifter_table()))
        _device_tables[key] = t
    return t


PcmLike = Union[torch.Tensor, np.ndarray, Sequence]


class AudioFeaturizer:
    """PCM -> (feats [B, T_max, 161], frames [B] int32). Rows at or past an utterance's frame
    count are exact zeros (the conv front-end relies on zero padding).

    ``normalize="utterance"`` reproduces ``compute_features`` (DC removal and peak
    normalisation per utterance, statistics computed on the device); ``normalize="fixed"``
    applies ``(x - offset) * gain`` with the given scalars (default gain 1/32768 for int16
    input, 1 for float).

    ``input_rate`` (when given and different from ``sample_rate``) is the rate of the PCM handed
    in: it is resampled ``input_rate -> sample_rate`` by ``ops/resample.py`` and then featurized,
    on a GPU at 16 kHz as resample kernel, (statistics kernel,) featurize kernel with no
    synchronisation between them. Utterance statistics are those of the resampled signal; the
    default fixed gain still follows the dtype of the PCM handed in. Without it, a
    ``sample_rate`` other than 16 kHz featurizes at that rate on the host.
    """

    def __init__(self, kind: str = "mfcc", sample_rate: int = 16000, device=None,
                 out_dtype: torch.dtype = torch.float32, normalize: str = "utterance",
                 gain: Optional[float] = None, offset: float = 0.0, input_rate: Optional[int] = None):
        if kind not in FRAME_LEN:
            raise ValueError("kind must be 'mfcc' or 'spectrogram', not %r" % (kind,))
        if normalize not in ("utterance", "fixed"):
            raise ValueError("normalize must be 'utterance' or 'fixed'")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be float32 or bfloat16")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.kind, self.sample_rate = kind, int(sample_rate)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.out_dtype, self.normalize = out_dtype, normalize
        self.gain, self.offset = gain, float(offset)
        self.use_kernels = self.device.type == "cuda" and self.sample_rate == KERNEL_RATE
        self._fixed: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}
        if self.use_kernels:
            from . import _ext
            self._C = _ext.ext()                     # raises if the extension is not built
            self._t = _tables(kind, self.sample_rate, self.device)
        self.input_rate = None if input_rate is None else int(input_rate)
        self._rs: Optional[Resampler] = None
        if self.input_rate is not None and self.input_rate != self.sample_rate:
            self._rs = Resampler(self.input_rate, self.sample_rate, self.device)

    # ---- helpers -------------------------------------------------------------------------
    def _gain_for(self, is_int16: bool) -> float:
        if self.gain is not None:
            return float(self.gain)
        return 1.0 / 32768.0 if is_int16 else 1.0

    def _pack(self, pcm: PcmLike, lens):
        """-> (tensor [B, S] on the host or the device, lens or None). int16 stays int16; anything
        else becomes float32 for the kernels and float64 (exact) for the numpy path."""
        ft = torch.float32 if self.use_kernels else torch.float64
        return pack_pcm(pcm, lens, ft, self.use_kernels)

    def _fixed_stats(self, B: int, is_int16: bool):
        key = (B, is_int16)
        if key not in self._fixed:
            self._fixed[key] = (torch.full((B,), self.offset, dtype=torch.float32, device=self.device),
                                torch.full((B,), self._gain_for(is_int16), dtype=torch.float32, device=self.device))
        return self._fixed[key]

    def _launch(self, pcm: torch.Tensor, lens, offset, gain, lead: int, mode: int, t_max: int):
        B = pcm.shape[0]
        out = torch.empty(B, t_max, NUM_FEATURES, dtype=self.out_dtype, device=self.device)
        frames = torch.empty(B, dtype=torch.int32, device=self.device)
        t = self._t
        self._C.featurize(pcm, lens, offset, gain, t["basis"], t["mel_idx"], t["mel_w"], t["dct"], t["lifter"],
                          _KIND_ID[self.kind], lead, mode, out, frames)
        return out, frames

    def _normalise_cpu(self, x: np.ndarray, is_int16: bool) -> np.ndarray:
        return (x.astype(np.float64) - self.offset) * self._gain_for(is_int16)

    def _features_cpu(self, sig: np.ndarray) -> np.ndarray:
        if self.kind == "mfcc":
            return F.mfcc(sig, self.sample_rate)
        return F.spectrogram(sig, self.sample_rate)

    # ---- whole utterances --------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, pcm: PcmLike, lens=None) -> Tuple[torch.Tensor, torch.Tensor]:
        pcm, lens = self._pack(pcm, lens)
        is_i16 = pcm.dtype == torch.int16                # of the PCM handed in: the default gain's
        if self._rs is not None:
            pcm, lens = self._pack(*self._rs(pcm, lens))
        B, S = pcm.shape
        if self.use_kernels:
            pcm = pcm.to(self.device, non_blocking=True).contiguous()
            if lens is not None:
                lens = lens.to(self.device, non_blocking=True)
            if self.normalize == "utterance":
                offset = torch.empty(B, dtype=torch.float32, device=self.device)
                gain = torch.empty(B, dtype=torch.float32, device=self.device)
                self._C.audio_stats(pcm, lens, offset, gain)
            else:
                offset, gain = self._fixed_stats(B, is_i16)
            return self._launch(pcm, lens, offset, gain, 0, 0, num_frames(S, self.kind))
        # CPU path (also every sample rate the kernels do not cover): data/featurizer.py
        x = pcm.cpu().numpy()
        ns = [S] * B if lens is None else [int(v) for v in lens.cpu().tolist()]
        feats = []
        for b in range(B):
            a = x[b, :ns[b]]
            if self.normalize == "utterance":
                feats.append(F.compute_features(a, self.sample_rate, self.kind))
            else:
                feats.append(self._features_cpu(self._normalise_cpu(a, is_i16)))
        t_max = max(f.shape[0] for f in feats)
        out = np.zeros((B, t_max, NUM_FEATURES), np.float32)
        for b, f in enumerate(feats):
            out[b, :f.shape[0]] = f
        frames = torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)
        return torch.from_numpy(out).to(self.device, self.out_dtype), frames.to(self.device)

    # ---- streaming ---------------------------------------------------------------------------
    def stream(self, batch: int) -> "FeatureStream":
        """State of ``batch`` concurrent audio streams (see :class:`FeatureStream`)."""
        if self.normalize != "fixed":
            raise ValueError("streaming needs normalize='fixed': a whole-utterance mean and peak do "
                             "not exist yet while audio is still arriving")
        return FeatureStream(self, batch)


class FeatureStream:
    """Incremental featurization of ``B`` streams that share one chunk schedule.

    ``push(chunk)`` returns the frames that became complete; the state carries the
    unconsumed tail of the signal plus the one sample before it (the pre-emphasis needs it).
    ``push(chunk, final=True)`` also emits the zero-padded last frame, so the total over a
    stream equals ``num_frames`` of the whole signal, and the frames equal those of one whole
    call. Streams use ``normalize="fixed"``: the per-utterance mean and peak of
    ``normalize="utterance"`` are not known before the audio has ended.
    """

    def __init__(self, fz: AudioFeaturizer, batch: int):
        self.fz, self.B = fz, int(batch)
        self.buf: Optional[torch.Tensor] = None      # [B, lead + tail] raw samples
        self.lead = 0                                # 1: buf[:, 0] is the sample before the tail
        self.emitted = 0                             # frames emitted so far
        self.finished = False
        self.last_frames: Optional[torch.Tensor] = None
        self.rs = fz._rs.stream(batch) if fz._rs is not None else None   # input_rate: resample first
        self.src_i16: Optional[bool] = None          # dtype of the PCM handed in (default gain)

    @torch.no_grad()
    def push(self, chunk, final: bool = False, lens=None) -> torch.Tensor:
        """Feed [B, S_c] samples. ``lens`` ([B] valid samples of this chunk) is accepted only
        with ``final=True``, where streams may end at different samples."""
        fz = self.fz
        if self.finished:
            raise RuntimeError("stream already finished")
        if lens is not None and not final:
            raise ValueError("lens is only meaningful with final=True")
        chunk, lens = fz._pack(chunk, lens)
        if chunk.shape[0] != self.B:
            raise ValueError("chunk must be [%d, S_c]" % self.B)
        if self.src_i16 is None:
            self.src_i16 = chunk.dtype == torch.int16
        if self.rs is not None:                      # the resampler's new outputs are this push's chunk
            chunk = self.rs.push(chunk, final, lens)
            chunk, lens = fz._pack(chunk, self.rs.last_lens if final else None)
        dev = fz.device if fz.use_kernels else torch.device("cpu")
        chunk = chunk.to(dev)
        if self.buf is None:
            self.buf = chunk
        else:
            if chunk.dtype != self.buf.dtype:
                raise ValueError("a stream's chunks must share one dtype")
            self.buf = torch.cat([self.buf, chunk], 1)
        n = self.buf.shape[1] - self.lead            # logical samples not yet consumed
        mode = 1 if not final else (0 if self.emitted == 0 else 2)
        t_new = _stream_frames(n, fz.kind, mode)
        if lens is not None:
            lens = (lens.to(dev) + (n - chunk.shape[1])).to(torch.int32)
        if final:
            self.finished = True
        if t_new == 0:
            self.last_frames = torch.zeros(self.B, dtype=torch.int32, device=fz.device)
            return torch.zeros(self.B, 0, NUM_FEATURES, dtype=fz.out_dtype, device=fz.device)
        is_i16 = self.src_i16
        if fz.use_kernels:
            offset, gain = fz._fixed_stats(self.B, is_i16)
            out, self.last_frames = fz._launch(self.buf.contiguous(), lens, offset, gain, self.lead, mode, t_new)
        else:
            out, self.last_frames = self._push_cpu(n, lens, mode, t_new, is_i16)
        self.emitted += t_new
        if not final:
            used = t_new * HOP                       # the next frame starts here
            self.buf = self.buf[:, self.lead + used - 1:]
            self.lead = 1
        return out

    def _push_cpu(self, n, lens, mode, t_new, is_i16):
        fz = self.fz
        x = fz._normalise_cpu(self.buf.numpy(), is_i16)
        out = np.zeros((self.B, t_new, NUM_FEATURES), np.float32)
        frames = []
        for b in range(self.B):
            nb = n if lens is None else int(lens[b])
            sig = x[b, self.lead:self.lead + nb]
            if fz.kind == "mfcc":
                prev = x[b, :self.lead]              # the sample before the tail, if any
                full = np.concatenate([prev, sig])
                pre = full[1:] - 0.97 * full[:-1]
                sig = pre if self.lead else np.append(sig[:1], pre)
            tb = _stream_frames(nb, fz.kind, mode)
            if tb:
                if mode == 1:                        # complete frames only: no padded frame
                    sig = sig[:(tb - 1) * HOP + FRAME_LEN[fz.kind]]
                f = F.mfcc(sig, fz.sample_rate, preemph=0.0) if fz.kind == "mfcc" else \
                    F.spectrogram(sig, fz.sample_rate)
                out[b, :tb] = f[:tb]
            frames.append(tb)
        return (torch.from_numpy(out).to(fz.device, fz.out_dtype),
                torch.tensor(frames, dtype=torch.int32, device=fz.device))
