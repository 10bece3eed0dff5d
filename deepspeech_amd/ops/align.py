"""CTC forced alignment: the best (Viterbi) path of a label sequence through frame-wise
emissions, with per-label frame spans and scores.

GPU tensors run csrc/align.hip (one wave per utterance, forward pass and backtrack in one
launch, nothing synchronised); CPU tensors run the oracle ``ops/reference.py ctc_viterbi_ref``.
The recurrence, its fixed tie rule (stay, then s-1, then s-2; final state 2L before 2L-1) and the
output conventions are documented there.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import BLANK
from . import reference as R

MAX_CLASSES = 32          # csrc/align.hip: one 32-wide log-prob row per frame
MAX_STATES = 2048         # lattice states 2*Lmax+1 the widest register tile holds


class Alignment(NamedTuple):
    path: torch.Tensor        # [N, T] int32: class on the best path per frame, -1 for t >= len
    tok_start: torch.Tensor   # [N, Lmax] int32: first frame in each label's state, -1 past label_lens
    tok_end: torch.Tensor     # [N, Lmax] int32: last frame (inclusive)
    tok_score: torch.Tensor   # [N, Lmax] fp32: sum of lp over those frames
    score: torch.Tensor       # [N] fp32: the path's total log-probability (-inf: no path)


def _check_limits(K: int, Lmax: int, blank: int) -> None:
    if K > MAX_CLASSES:
        raise ValueError("ctc_forced_align: K = %d classes exceeds the limit of %d" % (K, MAX_CLASSES))
    if 2 * Lmax + 1 > MAX_STATES:
        raise ValueError("ctc_forced_align: 2*Lmax+1 = %d lattice states exceeds the limit of %d "
                         "(at most %d labels per utterance)" % (2 * Lmax + 1, MAX_STATES, (MAX_STATES - 1) // 2))
    if not 0 <= blank < K:
        raise ValueError("ctc_forced_align: blank = %d outside the %d classes" % (blank, K))


def ctc_forced_align(emissions: torch.Tensor, lens: torch.Tensor, labels: torch.Tensor, label_lens: torch.Tensor,
                     blank: int = BLANK, log_probs: bool = False) -> Alignment:
    """emissions [T, N, K] time-major (fp32 or bf16): log-probabilities when ``log_probs``, else
    logits (log-softmaxed per valid frame first). lens [N], labels [N, Lmax], label_lens [N].
    The result stays on the emissions' device; nothing is synchronised."""
    if emissions.dim() != 3:
        raise ValueError("ctc_forced_align: emissions must be [T, N, K]")
    T, N, K = emissions.shape
    if labels.dim() == 1:
        labels = labels.view(N, -1)
    _check_limits(K, labels.shape[1], blank)
    if not emissions.is_cuda:
        lp = emissions.float() if log_probs else torch.log_softmax(emissions.float(), -1)
        return Alignment(*R.ctc_viterbi_ref(lp, lens, labels, label_lens, blank))
    from . import _ext
    C = _ext.ext()
    dev = emissions.device
    em = emissions if emissions.dtype in (torch.float32, torch.bfloat16) else emissions.float()
    em = em.contiguous()
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    if labels.shape[1] == 0:
        labels = torch.zeros(N, 1, device=dev, dtype=torch.int32)
    Lmax = labels.shape[1]
    lens = lens.to(device=dev, dtype=torch.int32).contiguous()
    label_lens = label_lens.to(device=dev, dtype=torch.int32).contiguous()
    i32 = dict(device=dev, dtype=torch.int32)
    f32 = dict(device=dev, dtype=torch.float32)
    out = Alignment(torch.empty(N, T, **i32), torch.empty(N, Lmax, **i32), torch.empty(N, Lmax, **i32),
                    torch.empty(N, Lmax, **f32), torch.empty(N, **f32))
    ws = torch.empty(max(16, int(C.ctc_align_ws_bytes(T, N, Lmax))), device=dev, dtype=torch.uint8)
    C.ctc_align(em, lens, labels, label_lens, out.path, out.tok_start, out.tok_end, out.tok_score, out.score, ws,
                blank, bool(log_probs))
    return out
