"""Pure-PyTorch reference implementations ("engine=ref").

These are the golden model for every HIP kernel test and the CPU plumbing path
(BASELINE config 1). They follow the reference's semantics op by op:

* clipped ReLU            — src/custom_ops.py:99-104
* get_rnn_seqlen          — src/deepSpeech.py:38-48
* ReLU-RNN cell (+SBN)    — src/custom_ops.py:36-72 (CustomRNNCell2)
* bidirectional dynamic RNN with per-utterance reversal and zero outputs past the
  length, directions summed — src/custom_ops.py:75-96, TF bidirectional_dynamic_rnn
* CTC loss (blank = last class, mean over batch) — src/deepSpeech_NCHW.py:204-228
* greedy CTC decoder      — src/deepSpeech_test.py:212-215

The GRU cell is the cuDNN/"reset-after" form so the recurrent product of all three
gates is one GEMM:  r,z = sigma(gx_rz + U_rz h + b_rz); n = tanh(gx_n + r*(U_n h + b_hn));
h' = (1-z) n + z h.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import BLANK

RELU_CLIP = 20.0
SBN_EPS = 1e-5


def clipped_relu(x: torch.Tensor, cap: float = RELU_CLIP) -> torch.Tensor:
    return torch.clamp(x, min=0.0, max=cap)


def get_rnn_seqlen(seq_lens: torch.Tensor) -> torch.Tensor:
    """T2 = ceil((ceil((T-19)/2) - 9)/2) of the reference (src/deepSpeech.py:38-48).

    For integer T this is floor((floor((T-18)/2) - 8)/2) = floor((T-34)/4): two integer
    kernels instead of a float64 round trip (exact for every integer, negative included)."""
    s = seq_lens.to(torch.int32) if seq_lens.dtype != torch.int32 else seq_lens
    return torch.div(s - 34, 4, rounding_mode="floor").to(torch.int32)


def reverse_index(lens: torch.Tensor, T: int) -> torch.Tensor:
    """idx[t, b] = lens[b]-1-t for t < lens[b] else t  (TF ReverseSequence semantics)."""
    t = torch.arange(T, device=lens.device).unsqueeze(1)          # [T,1]
    L = lens.to(torch.long).unsqueeze(0)                          # [1,N]
    return torch.where(t < L, L - 1 - t, t.expand(T, L.shape[1]))


def reverse_sequence(x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """Reverse x[T, N, ...] within each utterance's length (time-major)."""
    T = x.shape[0]
    idx = reverse_index(lens, T)
    idx = idx.view(T, idx.shape[1], *([1] * (x.dim() - 2))).expand_as(x)
    return torch.gather(x, 0, idx)


def time_mask(lens: torch.Tensor, T: int, dtype=torch.bool) -> torch.Tensor:
    """[T, N] mask, True where t < lens[b]."""
    t = torch.arange(T, device=lens.device).unsqueeze(1)
    return (t < lens.to(torch.long).unsqueeze(0)).to(dtype)


def lookahead_ref(h: torch.Tensor, w: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """Lookahead (row) convolution (Deep Speech 2, section 3.7) over time-major h [T, B, H] with
    w [H, tau+1] and valid(t, b) = t < min(lens[b], T):

        r[t,b,i] = valid(t,b) ? sum_{j=0..tau, valid(t+j,b)} w[i,j] h[t+j,b,i] : 0

    Linear, no bias; summed in ascending j in h's dtype (fp64 in: the oracle of the kernels)."""
    T = h.shape[0]
    m = time_mask(lens.to(h.device), T).unsqueeze(-1)                 # [T, B, 1]
    hm = torch.where(m, h, torch.zeros((), dtype=h.dtype, device=h.device))
    w = w.to(h.dtype)
    r = torch.zeros_like(hm)
    for j in range(min(w.shape[1], T)):
        term = w[:, j] * hm[j:]
        r = r + (term if j == 0 else F.pad(term, (0, 0, 0, 0, 0, j)))
    return torch.where(m, r, torch.zeros((), dtype=h.dtype, device=h.device))


def lookahead_stream_ref(hist: torch.Tensor, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """One streaming step of the lookahead convolution: with s = [hist (tau frames); x (n frames)],
    out[k] = sum_j w[:,j] s[k+j] for k < n, and hist is rewritten in place with the last tau
    frames of s. Output k is the layer's output for the frame tau steps before input k."""
    tau, n = hist.shape[0], x.shape[0]
    s = torch.cat([hist, x.to(hist.dtype)], 0)
    w = w.to(s.dtype)
    out = torch.zeros_like(s[:n])
    for j in range(tau + 1):
        out = out + w[:, j] * s[j:j + n]
    hist.copy_(s[n:])
    return out


def seq_batch_norm(y: torch.Tensor, lens: torch.Tensor, mode: str,
                   moving_mean: Optional[torch.Tensor] = None,
                   moving_var: Optional[torch.Tensor] = None,
                   training: bool = True, momentum: float = 0.5) -> torch.Tensor:
    """Sequence-wise BN of the input projection y[T, N, D].

    mode 'frozen': normalise with the (never-updated) moving stats — reference parity
    (src/custom_ops.py:184-199, quirk Q3): y * 1/sqrt(var+eps) with mean 0 / var 1.
    mode 'batch' : DS2-paper sequence-wise BN — statistics over every valid (t, n)
    row during training (running stats updated), moving stats in eval.
    mode 'none'  : identity.
    """
    if mode == "none":
        return y
    if mode == "frozen" or not training:
        mean = moving_mean if moving_mean is not None else torch.zeros(y.shape[-1], device=y.device)
        var = moving_var if moving_var is not None else torch.ones(y.shape[-1], device=y.device)
        return (y - mean.to(y.dtype)) * torch.rsqrt(var.to(y.dtype) + SBN_EPS)
    T, N, D = y.shape
    m = time_mask(lens, T, y.dtype).unsqueeze(-1)               # [T,N,1]
    cnt = m.sum().clamp(min=1.0)
    mean = (y * m).sum(dim=(0, 1)) / cnt
    var = (((y - mean) * m) ** 2).sum(dim=(0, 1)) / cnt
    if moving_mean is not None:
        with torch.no_grad():
            moving_mean.mul_(momentum).add_((1 - momentum) * mean.detach().float())
            moving_var.mul_(momentum).add_((1 - momentum) * var.detach().float())
    return (y - mean) * torch.rsqrt(var + SBN_EPS)


# ---------------------------------------------------------------------------------
# single-direction recurrences over a precomputed input projection gx[T, N, G*H]
# ---------------------------------------------------------------------------------
def _mm_in(h: torch.Tensor, mm_dtype) -> torch.Tensor:
    """Operand rounding of the recurrent product (the HIP kernels feed h to MFMA in bf16
    while keeping the state itself in fp32); identity when mm_dtype is None."""
    return h if mm_dtype is None else h.to(mm_dtype).to(h.dtype)


def rnn_relu_scan(gx: torch.Tensor, U: torch.Tensor, lens: torch.Tensor,
                  h0: Optional[torch.Tensor] = None, cap: float = RELU_CLIP, mm_dtype=None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """h_t = min(relu(gx_t + U h_{t-1}), cap); gx already holds SBN(Wx) + B.

    Returns (outputs[T,N,H] with zeros past each length, final state[N,H])."""
    T, N, H = gx.shape
    h = gx.new_zeros(N, H) if h0 is None else h0
    mask = time_mask(lens, T).unsqueeze(-1)
    outs = []
    Ut = U.t()
    for t in range(T):
        hn = torch.clamp(gx[t] + _mm_in(h, mm_dtype) @ Ut, 0.0, cap)
        m = mask[t]
        outs.append(torch.where(m, hn, torch.zeros_like(hn)))
        h = torch.where(m, hn, h)
    return torch.stack(outs, 0), h


def gru_scan(gx: torch.Tensor, U: torch.Tensor, b_h: torch.Tensor, lens: torch.Tensor,
             h0: Optional[torch.Tensor] = None, mm_dtype=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reset-after GRU over gx[T,N,3H] (gate order r, z, n)."""
    T, N, G3 = gx.shape
    H = G3 // 3
    h = gx.new_zeros(N, H) if h0 is None else h0
    mask = time_mask(lens, T).unsqueeze(-1)
    outs = []
    Ut = U.t()
    for t in range(T):
        gh = _mm_in(h, mm_dtype) @ Ut + b_h
        r = torch.sigmoid(gx[t, :, :H] + gh[:, :H])
        z = torch.sigmoid(gx[t, :, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gx[t, :, 2 * H:] + r * gh[:, 2 * H:])
        hn = (1.0 - z) * n + z * h
        m = mask[t]
        outs.append(torch.where(m, hn, torch.zeros_like(hn)))
        h = torch.where(m, hn, h)
    return torch.stack(outs, 0), h


def recurrent_scan(cell: str, gx, U, b_h, lens, h0=None, mm_dtype=None):
    if cell == "rnn_relu":
        return rnn_relu_scan(gx, U, lens, h0, mm_dtype=mm_dtype)
    if cell == "gru":
        return gru_scan(gx, U, b_h, lens, h0, mm_dtype=mm_dtype)
    raise ValueError(cell)


def birnn_ref(cell: str, gx_f: torch.Tensor, gx_b: Optional[torch.Tensor],
              U_f, U_b, bh_f, bh_b, lens: torch.Tensor, mm_dtype=None) -> torch.Tensor:
    """Bidirectional layer over precomputed projections; returns fw + bw (Q2)."""
    y_f, _ = recurrent_scan(cell, gx_f, U_f, bh_f, lens, mm_dtype=mm_dtype)
    if gx_b is None:
        return y_f
    y_b_rev, _ = recurrent_scan(cell, reverse_sequence(gx_b, lens), U_b, bh_b, lens, mm_dtype=mm_dtype)
    return y_f + reverse_sequence(y_b_rev, lens)


# ---------------------------------------------------------------------------------
# CTC
# ---------------------------------------------------------------------------------
def collapse_repeated(labels: Sequence[int]) -> List[int]:
    out: List[int] = []
    for c in labels:
        if not out or out[-1] != c:
            out.append(c)
    return out


def ctc_loss_ref(logits: torch.Tensor, targets: torch.Tensor, logit_lens: torch.Tensor,
                 target_lens: torch.Tensor, blank: int = BLANK,
                 zero_infinity: bool = True) -> torch.Tensor:
    """Per-utterance CTC negative log-likelihood over time-major logits [T, N, K].

    Returns the vector of losses [N] (fp32); the model reduces it with mean like
    tf.reduce_mean(ctc_loss) (src/deepSpeech_NCHW.py:225-226)."""
    lp = F.log_softmax(logits.float(), dim=-1)
    return F.ctc_loss(lp, targets, logit_lens.long(), target_lens.long(), blank=blank,
                      reduction="none", zero_infinity=zero_infinity)


def greedy_decode(logits: torch.Tensor, lens: torch.Tensor, blank: int = BLANK) -> List[List[int]]:
    """tf.nn.ctc_greedy_decoder(merge_repeated=True): argmax, merge repeats, drop blank."""
    best = logits.argmax(-1).cpu()            # [T, N]
    lens = lens.cpu()
    out = []
    for b in range(best.shape[1]):
        seq = best[: int(lens[b]), b].tolist()
        res, prev = [], None
        for c in seq:
            if c != prev and c != blank:
                res.append(c)
            prev = c
        out.append(res)
    return out


# ---------------------------------------------------------------------------------
# CTC forced alignment (the oracle of csrc/align.hip)
# ---------------------------------------------------------------------------------
def ctc_viterbi_ref(log_probs: torch.Tensor, lens, labels, label_lens, blank: int = BLANK):
    """Best CTC path of each utterance's labels through ``log_probs`` [T, N, K] (natural-log
    probabilities, used as they are after widening to fp32).

    Lattice states s = 0 .. 2L (even = blank, odd = label s >> 1), start in state 0 or 1, end in
    state 2L or 2L-1:

        v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), [v_{t-1}(s-2) if s odd and label != label of s-2])
                 + lp_t(class(s))

    in fp32, ``max`` first and then ONE add per state and frame: the operations of the kernel in
    the kernel's order, so ``score`` is bitwise the kernel's on the same log-probs.
    Tie rule: on equal values stay (s), then s-1, then s-2 (strict ``>`` in that order); at the
    end state 2L wins over 2L-1 unless 2L-1 is strictly better.

    Returns (path [N, T] int32, tok_start [N, Lmax] int32, tok_end [N, Lmax] int32,
    tok_score [N, Lmax] fp32, score [N] fp32) as CPU tensors, Lmax = max(1, labels.shape[1]):
    ``path`` is the class on the best path per frame (-1 for t >= len), ``tok_start`` /
    ``tok_end`` the first / last frame (inclusive) spent in each label's state and
    ``tok_score`` the sum of lp over those frames (-1 / -1 / 0 at and past ``label_lens``),
    ``score`` the path's total log-probability. An utterance without a finite path (len <= 0,
    fewer frames than labels + adjacent equal labels, -inf on every path) has score -inf,
    path -1 and spans -1; a NaN in a valid frame gives score NaN (as it makes the CTC loss
    NaN), path -1 and spans -1."""
    import numpy as np
    lp_all = log_probs.detach().to(torch.float32).cpu().numpy()
    T, N, K = lp_all.shape
    lens = np.asarray(torch.as_tensor(lens).cpu().numpy(), dtype=np.int64).reshape(N)
    label_lens = np.asarray(torch.as_tensor(label_lens).cpu().numpy(), dtype=np.int64).reshape(N)
    labels = np.asarray(torch.as_tensor(labels).cpu().numpy(), dtype=np.int64).reshape(N, -1)
    Lw = labels.shape[1]
    Lmax = max(1, Lw)
    path = np.full((N, T), -1, np.int32)
    tok_start = np.full((N, Lmax), -1, np.int32)
    tok_end = np.full((N, Lmax), -1, np.int32)
    tok_score = np.zeros((N, Lmax), np.float32)
    score = np.full((N,), -np.inf, np.float32)
    ninf = np.float32(-np.inf)
    for b in range(N):
        n = int(min(lens[b], T))
        L = int(max(0, min(label_lens[b], Lw)))
        if n <= 0 or L > n:
            continue
        lab = labels[b, :L]
        if L and (lab.min() < 0 or lab.max() >= K):
            continue                                  # no finite path through a class that is not there
        S = 2 * L + 1
        cls = np.full(S, blank, np.int64)
        cls[1::2] = lab
        skip = np.zeros(S, bool)
        skip[3::2] = lab[1:] != lab[:-1]
        lp = lp_all[:n, b]                            # [n, K] fp32
        if np.isnan(lp).any():
            score[b] = np.float32(np.nan)
            continue
        em = lp[:, cls]                               # [n, S]
        v = np.full(S, ninf, np.float32)
        v[:2] = em[0, :2]
        bp = np.zeros((n, S), np.int8)
        with np.errstate(invalid="ignore"):
            for t in range(1, n):
                a1 = np.full(S, ninf, np.float32)
                a1[1:] = v[:-1]
                a2 = np.full(S, ninf, np.float32)
                a2[2:] = v[:-2]
                a2 = np.where(skip, a2, ninf)
                best, k = v, np.zeros(S, np.int8)
                m = a1 > best
                best, k = np.where(m, a1, best), np.where(m, np.int8(1), k)
                m = a2 > best
                best, k = np.where(m, a2, best), np.where(m, np.int8(2), k)
                v = (best + em[t]).astype(np.float32)
                bp[t] = k
        s = S - 1
        if S >= 2 and v[S - 2] > v[S - 1]:
            s = S - 2
        score[b] = v[s]
        if not np.isfinite(v[s]):
            if v[s] != ninf:                          # +inf / NaN out of infinities: report, no path
                score[b] = v[s]
            continue
        for t in range(n - 1, -1, -1):
            path[b, t] = cls[s]
            if s & 1:
                l = s >> 1
                if tok_end[b, l] < 0:
                    tok_end[b, l] = t
                tok_start[b, l] = t
            if t > 0:
                s -= int(bp[t, s])
        for l in range(L):
            acc = np.float32(0.0)
            for t in range(tok_start[b, l], tok_end[b, l] + 1):
                acc = np.float32(acc + lp[t, lab[l]])
            tok_score[b, l] = acc
    return (torch.from_numpy(path), torch.from_numpy(tok_start), torch.from_numpy(tok_end),
            torch.from_numpy(tok_score), torch.from_numpy(score))


# ---- SpecAugment (ops/specaug.py, csrc/specaug.hip) ---------------------------------------
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
SPECAUG_MEAN_SLICES = 32


def philox4x32(ctr, key):
    """Philox4x32-10: ``ctr`` four and ``key`` two 32-bit words (ints, or numpy arrays that
    broadcast against each other); returns the four output words as uint64 arrays (ints for
    int inputs)."""
    scalar = all(isinstance(v, (int, np.integer)) for v in tuple(ctr) + tuple(key))
    m32 = np.uint64(0xffffffff)
    c = [np.asarray(v, np.uint64) & m32 for v in ctr]
    k = [np.asarray(v, np.uint64) & m32 for v in key]
    for _ in range(10):
        p0 = np.uint64(PHILOX_M[0]) * c[0]
        p1 = np.uint64(PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(PHILOX_W[0])) & m32, (k[1] + np.uint64(PHILOX_W[1])) & m32]
    return tuple(int(v) for v in c) if scalar else tuple(c)


def specaug_plan_ref(lens, T: int, F: int, policy, seed: int, step: int, first_utt: int = 0) -> torch.Tensor:
    """The SpecAugment plan [B, 2 + 2 nF + 2 nT] int32 = (w0, w, f0, fw, ..., t0, tw, ...) of
    utterances first_utt .. first_utt + B - 1 at ``step``, in exact integer arithmetic.
    ``policy`` has nF, Fw, nT, Tw, p_ppm, W. Block j of the generator has counter (j, u, step)
    and key seed; word i of the stream is x[i]; a uniform integer in [0, n) is (x * n) >> 32."""
    L = np.clip(np.asarray(torch.as_tensor(lens).cpu()).astype(np.int64).reshape(-1), 0, T)
    B = L.shape[0]
    nF, nT, W = int(policy.nF), int(policy.nT), int(policy.W)
    ndraw = 2 + 2 * nF + 2 * nT
    u = (int(first_utt) + np.arange(B, dtype=np.uint64)) & np.uint64(0xffffffff)
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    words = []
    for j in range((ndraw + 3) // 4):
        words.extend(philox4x32((np.uint64(j), u, np.uint64(step & 0xffffffff), np.uint64((step >> 32) & 0xffffffff)),
                                (np.uint64(key[0]), np.uint64(key[1]))))
    x = [np.broadcast_to(w, (B,)).astype(np.uint64) for w in words]

    def mulhi(xw, n):                      # n int64 array or int, 0 <= n <= 2^32
        return ((xw * np.asarray(n, np.int64).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)

    plan = np.zeros((B, ndraw), np.int64)
    n0 = L - 2 * W - 2
    warp = (n0 >= 1) & (W > 0)
    plan[:, 0] = np.where(warp, W + 1 + mulhi(x[0], np.maximum(n0, 0)), 0)
    plan[:, 1] = np.where(warp, mulhi(x[1], 2 * W + 1) - W, 0)
    d = 2
    for k in range(nF):
        fw = mulhi(x[d], min(int(policy.Fw), F) + 1)
        plan[:, 2 + 2 * k] = mulhi(x[d + 1], F - fw + 1)
        plan[:, 3 + 2 * k] = fw
        d += 2
    c = np.minimum(int(policy.Tw), (L * int(policy.p_ppm)) // 1000000)
    for k in range(nT):
        tw = mulhi(x[d], c + 1)
        plan[:, 2 + 2 * nF + 2 * k] = mulhi(x[d + 1], L - tw + 1)
        plan[:, 3 + 2 * nF + 2 * k] = tw
        d += 2
    return torch.from_numpy(plan.astype(np.int32))


def specaug_warp_index(lens: torch.Tensor, plan: torch.Tensor, T: int):
    """Source of every output frame under the plan's warp: (i, r, den, valid), each [B, T] int64
    (valid bool): out[t] = x[i] + (r / den) (x[i+1] - x[i]) for valid = t < L; i = t, r = 0 and
    den = 1 in the padding and under the identity warp (w0 = 0)."""
    dev = plan.device
    L = lens.to(dev).long().clamp(0, T)[:, None]
    t = torch.arange(T, device=dev)[None, :]
    w0 = plan[:, 0:1].long()
    d0 = w0 + plan[:, 1:2].long()
    valid = t < L
    plain = (w0 == 0) | ~valid
    left = t <= d0
    num = torch.where(left, t * w0, (t - d0) * (L - 1 - w0))
    den = torch.where(left, d0, L - 1 - d0)
    base = torch.where(left, torch.zeros_like(w0), w0)
    den = torch.where(plain, torch.ones_like(den), den).clamp(min=1)
    num = torch.where(plain, torch.zeros_like(num), num)
    q = torch.div(num, den, rounding_mode="floor")
    i = torch.where(plain, t.expand_as(num), base + q)
    return i, num - q * den, den, valid


def specaug_masks(lens: torch.Tensor, plan: torch.Tensor, T: int, F: int, nF: int):
    """(time mask [B, T], frequency mask [B, F]) of a plan, both bool; the padding is in neither."""
    dev = plan.device
    t = torch.arange(T, device=dev)[None, :]
    f = torch.arange(F, device=dev)[None, :]
    tm = torch.zeros(plan.shape[0], T, dtype=torch.bool, device=dev)
    fm = torch.zeros(plan.shape[0], F, dtype=torch.bool, device=dev)
    for k in range(nF):
        f0, fw = plan[:, 2 + 2 * k, None].long(), plan[:, 3 + 2 * k, None].long()
        fm |= (f >= f0) & (f < f0 + fw)
    for k in range((plan.shape[1] - 2 - 2 * nF) // 2):
        t0, tw = plan[:, 2 + 2 * nF + 2 * k, None].long(), plan[:, 3 + 2 * nF + 2 * k, None].long()
        tm |= (t >= t0) & (t < t0 + tw)
    return tm & (t < lens.to(dev).long().clamp(0, T)[:, None]), fm


def specaug_apply_ref(x: torch.Tensor, lens: torch.Tensor, plan: torch.Tensor, fill_values: Optional[torch.Tensor],
                      nF: int) -> torch.Tensor:
    """SpecAugment by ``plan`` on x [B, T, F], on x's device: fp64 arithmetic for an fp64 x (the
    oracle), fp32 otherwise (the CPU path and the composite). Warp first, masks on warped frame
    indices, frames >= L bit copies; masked cells take fill_values [B, F] (None: zeros) by
    selection, whatever the input holds there."""
    B, T, F = x.shape
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    xc = x.to(ct)
    plan = plan.to(x.device)
    i, r, den, valid = specaug_warp_index(lens, plan, T)
    a = torch.gather(xc, 1, i[:, :, None].expand(B, T, F))
    if x.device.type != "cpu" or bool((plan[:, 0] != 0).any()):      # no host round trip on a GPU
        b = torch.gather(xc, 1, (i + 1).clamp(max=T - 1)[:, :, None].expand(B, T, F))
        q = (r.to(ct) / den.to(ct))[:, :, None]
        a = torch.where((r == 0)[:, :, None], a, a + q * (b - a))
    tm, fm = specaug_masks(lens, plan, T, F, nF)
    fill = (torch.zeros(B, F, dtype=ct, device=x.device) if fill_values is None else fill_values.to(x.device, ct))
    masked = (tm[:, :, None] | fm[:, None, :]) & valid[:, :, None]
    out = torch.where(masked, fill[:, None, :].expand(B, T, F), a)
    return torch.where(valid[:, :, None], out.to(x.dtype), x)


def specaug_mean_ref(x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """mean [B, F] of x [B, T, F] over frames t < L (0 for L == 0). fp64 x: the plain fp64 mean
    (the oracle). Otherwise fp32 in the kernel's order: 32 partial sums over frames s, s + 32, ...
    in ascending order, added pairwise, divided by float(L)."""
    B, T, F = x.shape
    Ls = np.clip(np.asarray(torch.as_tensor(lens).cpu()).astype(np.int64).reshape(-1), 0, T)
    if x.dtype == torch.float64:
        out = torch.zeros(B, F, dtype=torch.float64)
        for b, L in enumerate(Ls):
            if L:
                out[b] = x[b, :L].sum(0) / float(L)
        return out
    xs = x.detach().to("cpu", torch.float32).numpy()
    S = SPECAUG_MEAN_SLICES
    out = np.zeros((B, F), np.float32)
    for b, L in enumerate(Ls):
        if L == 0:
            continue
        acc = np.zeros((S, F), np.float32)
        full = L // S
        for k in range(full):
            acc += xs[b, k * S:(k + 1) * S]
        acc[:L - full * S] += xs[b, full * S:L]
        while acc.shape[0] > 1:
            acc = acc[0::2] + acc[1::2]
        out[b] = acc[0] / np.float32(L)
    return torch.from_numpy(out)


# ---- dropout between recurrent layers (ops/dropout.py, csrc/dropout.hip) ------------------
def seq_dropout_threshold(p: float) -> int:
    """thr = clamp(round(p * 65536), 0, 65535) of a drop probability p in [0, 1): the effective
    probability is exactly thr / 65536, and thr == 0 is no dropout at all."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout probability must lie in [0, 1), not %r" % (p,))
    return min(max(int(round(p * 65536)), 0), 65535)


def seq_dropout_scale(thr: int) -> float:
    """65536 / (65536 - thr) as one correctly rounded fp32 division."""
    return float(np.float32(65536) / np.float32(65536 - int(thr)))


def seq_dropout_mask_ref(T: int, N: int, H: int, seed: int, step: int, first_utt: int, site: int, thr: int,
                         locked: bool) -> torch.Tensor:
    """The keep mask, bool [T, N, H] (True: kept), of the dropout between recurrent layers, in
    exact integer arithmetic. Element (t, b, i) has group g = i >> 3 and slot e = i & 7; the
    Philox4x32-10 block of key seed and counter (locked ? 0 : t, first_utt + b, step,
    0x80000000 | locked << 30 | site << 16 | g) gives words x0..x3, r = (x[e >> 1] >> (16 * (e & 1)))
    & 0xffff, and the element is kept iff r >= thr. Any H: a last partial group uses its first
    slots."""
    site, thr, locked = int(site), int(thr), bool(locked)
    G = (H + 7) // 8
    if not (0 <= site < 16384 and G <= 65536 and 0 <= thr <= 65535):
        raise ValueError("seq_dropout: site < 16384, H <= 8 * 65536, thr in [0, 65535]")
    Tm = 1 if locked else T
    t = np.arange(Tm, dtype=np.uint64)[:, None, None]
    u = ((int(first_utt) + np.arange(N, dtype=np.uint64)) & np.uint64(0xffffffff))[None, :, None]
    c3 = np.uint64(0x80000000 | (int(locked) << 30) | (site << 16)) | np.arange(G, dtype=np.uint64)[None, None, :]
    key = (np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff))
    words = philox4x32((t, u, np.uint64(step & 0xffffffff), c3), key)
    r = np.empty((Tm, N, G, 8), np.uint64)
    for j, w in enumerate(words):
        w = np.broadcast_to(w, (Tm, N, G))
        r[..., 2 * j] = w & np.uint64(0xffff)
        r[..., 2 * j + 1] = (w >> np.uint64(16)) & np.uint64(0xffff)
    keep = (r >= np.uint64(thr)).reshape(Tm, N, G * 8)[:, :, :H]
    return torch.from_numpy(np.array(np.broadcast_to(keep, (T, N, H))))


def seq_dropout_ref(x: torch.Tensor, seed: int, step: int, first_utt: int, site: int, thr: int,
                    locked: bool) -> torch.Tensor:
    """Dropout of x [T, N, H] under seq_dropout_mask_ref, on x's device: a kept element gives
    bf16(float(x) * scale) for a bf16 x (x * scale in x's precision otherwise) with scale =
    fp32(65536) / fp32(65536 - thr), a dropped one +0 by selection, whatever the input holds
    there. thr == 0: x itself. Differentiable: the gradient is the same map of the incoming one."""
    if int(thr) == 0:
        return x
    T, N, H = x.shape
    keep = seq_dropout_mask_ref(T, N, H, seed, step, first_utt, site, thr, locked).to(x.device)
    scale = seq_dropout_scale(thr)
    y = (x.float() * scale).to(x.dtype) if x.dtype in (torch.bfloat16, torch.float16) else x * scale
    return torch.where(keep, y, torch.zeros((), dtype=x.dtype, device=x.device))


# ---- audio resampling (ops/resample.py, csrc/resample.hip) --------------------------------
RESAMPLE_ZEROS = 24          # Z: sinc zero crossings on each side at the lower of the two rates
RESAMPLE_ROLLOFF = 0.90
RESAMPLE_BETA = 8.0          # Kaiser window


def resample_table(in_rate: int, out_rate: int) -> Tuple[int, int, int, np.ndarray]:
    """(L, M, K, h) of the polyphase windowed-sinc resampler in_rate -> out_rate: L = out / gcd,
    M = in / gcd, K = 2 ceil(Z max(1, M / L)) taps per output and h [L, K] fp64 with
    d = k - (K/2 - 1) - ph / L, h = scale sinc(scale d) I0(beta sqrt(1 - (d / (K/2))^2)) / I0(beta),
    scale = min(1, L / M) rolloff, 0 where |d| > K/2. Not renormalised."""
    in_rate, out_rate = int(in_rate), int(out_rate)
    if in_rate <= 0 or out_rate <= 0:
        raise ValueError("sample rates must be positive")
    g = int(np.gcd(in_rate, out_rate))
    L, M = out_rate // g, in_rate // g
    K = 2 * (-((-RESAMPLE_ZEROS * max(L, M)) // L))
    scale = min(1.0, L / M) * RESAMPLE_ROLLOFF
    half = K // 2
    d = (np.arange(K, dtype=np.float64)[None, :] - (half - 1)) - np.arange(L, dtype=np.float64)[:, None] / L
    r = 1.0 - (d / half) ** 2
    win = np.where(r >= 0, np.i0(RESAMPLE_BETA * np.sqrt(np.maximum(r, 0.0))) / np.i0(RESAMPLE_BETA), 0.0)
    return L, M, K, scale * np.sinc(scale * d) * win


def resample_out_len(S: int, L: int, M: int) -> int:
    """N(S) = ceil(S L / M): outputs of a row of S samples."""
    return -((-int(S) * int(L)) // int(M))


def resample_emitted(P: int, L: int, M: int, K: int) -> int:
    """E(P) = max(0, ceil((P - K/2) L / M)): outputs whose last tap lies inside the first P input
    samples, i.e. what a stream has emitted once P samples have arrived."""
    return max(0, -((-(int(P) - int(K) // 2) * int(L)) // int(M)))


def resample_ref(x, in_rate: int, out_rate: int, lens=None, return_abs: bool = False):
    """fp64 oracle: x [B, S] (or [S]) -> y [B, N(S)] with y[n] = sum_k h[ph, k] x[i - (K/2 - 1) + k],
    i = n M // L, ph = n M % L, x outside [0, lens[b]) read as +0 by selection; columns at or past
    N(lens[b]) are zeros. ``return_abs`` adds sum_k |h x| per output (the scale of the rounding
    bound of a fp32 evaluation)."""
    x = np.asarray(x)
    one = x.ndim == 1
    x = np.atleast_2d(x).astype(np.float64)
    B, S = x.shape
    L, M, K, h = resample_table(in_rate, out_rate)
    ns = [S] * B if lens is None else [int(v) for v in np.asarray(lens).reshape(-1)]
    N = resample_out_len(S, L, M)
    y = np.zeros((B, N), np.float64)
    a = np.zeros((B, N), np.float64)
    half = K // 2
    for b in range(B):
        sb = min(max(ns[b], 0), S)
        xp = np.zeros(S + K, np.float64)
        xp[half - 1:half - 1 + sb] = x[b, :sb]            # selection: nothing past sb is read
        nb = resample_out_len(sb, L, M)
        for n0 in range(0, nb, 8192):
            n = np.arange(n0, min(nb, n0 + 8192), dtype=np.int64)
            t = n * M
            taps = xp[(t // L)[:, None] + np.arange(K)[None, :]] * h[t % L]
            y[b, n] = taps.sum(1)
            a[b, n] = np.abs(taps).sum(1)
    if one:
        y, a = y[0], a[0]
    return (y, a) if return_abs else y


# ---------------------------------------------------------------------------- gradient-norm clipping
# Definition shared by csrc/optim.hip (grad_sumsq + clip_finalize + the CLIP Adam kernels), the CPU
# branch of FusedAdamEMA and the tests. With threshold C > 0 (inf: measure only) and
# x_i = fl32(g_i gscale), the first product of adam1 (csrc/common.h):
#   S = sum_i x_i^2 over the whole arena      norm = fl32(sqrt(S))
#   bad  = norm is not finite (a NaN / inf gradient, or S past the fp32 range)
#   coef = 0 if bad, else 1.0 exactly (selected, never computed) if norm <= C, else fl32(C / norm)
# A bad step updates nothing. Otherwise every element takes adam1 with g' = fl32(x_i coef) in place
# of x_i; x * 1.0f is exact, so a step with coef == 1 is bitwise the unclipped step.
def clip_from_sumsq(S: float, max_norm: float) -> Tuple[float, float, bool]:
    """(norm, coef, bad) of the definition from an fp32 sum of squares S, in fp32 arithmetic (sqrt and
    the quotient correctly rounded, as __fsqrt_rn / __fdiv_rn are): exactly what clip_finalize
    derives from its own S."""
    if not max_norm > 0:
        raise ValueError("max_norm must be > 0 (inf: measure only)")
    s = torch.tensor(float(S), dtype=torch.float32)
    norm = torch.sqrt(s)
    if not bool(torch.isfinite(norm)):
        return float(norm), 0.0, True
    c = torch.tensor(float(max_norm), dtype=torch.float32)
    coef = 1.0 if bool(norm <= c) else float(c / norm)
    return float(norm), coef, False


def clip_coef_ref(g: torch.Tensor, gscale: float, max_norm: float, oracle: bool = False):
    """(S, norm, coef, bad) of gradient ``g`` (any shape, fp32). fp32 composite: S summed by
    torch in fp32; ``oracle``: S in fp64 from the fp32-rounded x_i (then norm and coef from
    fl32(S) as the definition says)."""
    x = g.detach().reshape(-1).to(torch.float32) * torch.tensor(float(gscale), dtype=torch.float32, device=g.device)
    if oracle:
        x = x.to(torch.float64)
    S = float((x * x).sum().to(torch.float32)) if x.numel() else 0.0
    norm, coef, bad = clip_from_sumsq(S, max_norm)
    return S, norm, coef, bad


def clipped_adam_ref(p, g, m, v, ema, p16, lr_t: float, b1: float, b2: float, eps: float, gscale: float,
                     coef: Optional[float], keep: float, oracle: bool = False):
    """One Adam (TF epsilon-hat) + EMA update of flat arrays with the gradient scaled by ``coef``
    (None: unclipped; the caller skips a bad step).

    fp32 composite (default): in place on p, m, v (and ema, p16 when given), the op sequence of the
    unclipped CPU update with g' = (g gscale) coef in front. ``oracle``: nothing is modified; returns
    fp64 {p, m, v, ema} computed from the fp32-rounded g' (the kernel's operand)."""
    gj = g * gscale
    if coef is not None:
        gj = gj * coef
    if oracle:
        gj, p0, m0, v0 = gj.to(torch.float64), p.to(torch.float64), m.to(torch.float64), v.to(torch.float64)
        m1 = b1 * m0 + (1 - b1) * gj
        v1 = b2 * v0 + (1 - b2) * gj * gj
        p1 = p0 - lr_t * m1 / (v1.sqrt() + eps)
        out = dict(p=p1, m=m1, v=v1)
        if ema is not None:
            out["ema"] = p1 + keep * (ema.to(torch.float64) - p1)
        return out
    m.mul_(b1).add_(gj, alpha=1 - b1)
    v.mul_(b2).addcmul_(gj, gj, value=1 - b2)
    p.sub_(lr_t * m / (v.sqrt() + eps))
    if ema is not None:
        ema.copy_(p + keep * (ema - p))
    if p16 is not None:
        p16.copy_(p)
    return None


# ---------------------------------------------------------------------------- additive noise (ops/waveaug.py, csrc/waveaug.hip)
# Definition shared by the kernels, the torch composite and the tests. x [B, S] fp32 or int16
# (converted exactly, no 1/32768), n = clamp(lens[b], 0, S) (lens None: S), a bank of C clips
# (data fp32 [Ntot], start / length int32 [C]), a policy (p_ppm, snr_lo_cdb, snr_hi_cdb):
#   plan   (on, clip, off, snr_cdb) from one Philox4x32-10 block per utterance, key seed, counter
#          (0, u, step & 0xffffffff, 0x40000000 | (step >> 32) & 0x3fffffff), u = first_utt + b;
#          with U(w, m) = (w * m) >> 32: on = n > 0 and U(x0, 1000000) < p_ppm, clip = U(x1, C),
#          off = U(x2, length[clip]), snr_cdb = snr_lo_cdb + U(x3, snr_hi_cdb - snr_lo_cdb + 1)
#   z_i    data[start[clip] + (off + i) mod length[clip]]
#   Ex, En sum over i < n of x_i^2 and z_i^2 (fp64 here)
#   k      fl32(sqrt(Ex / (En 10^(snr_cdb / 1000)))), 0 when not on, Ex == 0, En == 0 or not finite
#   y_i    fl32(x_i + fl32(k z_i)) for i < n when on, x_i (a bit copy) when not, +0 for i >= n
WAVEAUG_STREAM = 0x40000000


def waveaug_lens(lens, B: int, S: int) -> np.ndarray:
    if lens is None:
        return np.full(B, S, np.int64)
    return np.clip(np.asarray(torch.as_tensor(lens).cpu()).astype(np.int64).reshape(-1), 0, S)


def waveaug_plan_ref(lens, B: int, S: int, length, policy, seed: int, step: int, first_utt: int = 0) -> torch.Tensor:
    """The plan [B, 4] int32 = (on, clip, off, snr_cdb) of utterances first_utt .. first_utt + B - 1
    at ``step``, in exact integer arithmetic. ``length`` [C] are the bank's clip lengths, ``policy``
    has p_ppm, snr_lo_cdb, snr_hi_cdb."""
    n = waveaug_lens(lens, B, S)
    length = np.asarray(torch.as_tensor(length).cpu()).astype(np.int64).reshape(-1)
    u = (int(first_utt) + np.arange(B, dtype=np.uint64)) & np.uint64(0xffffffff)
    x = philox4x32((np.uint64(0), u, np.uint64(step & 0xffffffff),
                    np.uint64(WAVEAUG_STREAM | ((step >> 32) & 0x3fffffff))),
                   (np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)))
    x = [np.broadcast_to(w, (B,)).astype(np.uint64) for w in x]

    def U(xw, m):
        return ((xw * np.asarray(m, np.int64).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)

    plan = np.zeros((B, 4), np.int64)
    plan[:, 0] = (n > 0) & (U(x[0], 1000000) < int(policy.p_ppm))
    plan[:, 1] = U(x[1], length.shape[0])
    plan[:, 2] = U(x[2], length[plan[:, 1]])
    plan[:, 3] = int(policy.snr_lo_cdb) + U(x[3], int(policy.snr_hi_cdb) - int(policy.snr_lo_cdb) + 1)
    return torch.from_numpy(plan.astype(np.int32))


def waveaug_noise_ref(plan, data, start, length, S: int) -> torch.Tensor:
    """z [B, S] fp32: each row's clip read as a loop from its offset."""
    plan = np.asarray(torch.as_tensor(plan).cpu()).astype(np.int64)
    data = np.asarray(torch.as_tensor(data).cpu())
    start = np.asarray(torch.as_tensor(start).cpu()).astype(np.int64)
    length = np.asarray(torch.as_tensor(length).cpu()).astype(np.int64)
    clip = plan[:, 1]
    idx = start[clip][:, None] + (plan[:, 2][:, None] + np.arange(S, dtype=np.int64)[None, :]) % length[clip][:, None]
    return torch.from_numpy(np.ascontiguousarray(data[idx], np.float32))


def waveaug_energy_ref(x, lens, z) -> torch.Tensor:
    """fp64 [B, 2] = (Ex, En) over i < n."""
    xv = np.asarray(torch.as_tensor(x).cpu()).astype(np.float64)
    zv = np.asarray(torch.as_tensor(z).cpu()).astype(np.float64)
    B, S = xv.shape
    valid = np.arange(S)[None, :] < waveaug_lens(lens, B, S)[:, None]
    e = np.stack([np.where(valid, xv * xv, 0.0).sum(1), np.where(valid, zv * zv, 0.0).sum(1)], 1)
    return torch.from_numpy(e)


def waveaug_coef_ref(plan, energy) -> torch.Tensor:
    """fp32 [B]: k evaluated in fp64 and rounded once, 0 by selection."""
    plan = np.asarray(torch.as_tensor(plan).cpu()).astype(np.int64)
    e = np.asarray(torch.as_tensor(energy).cpu()).astype(np.float64)
    with np.errstate(all="ignore"):
        k = np.sqrt(e[:, 0] / (e[:, 1] * np.power(10.0, plan[:, 3] / 1000.0))).astype(np.float32)
    ok = (plan[:, 0] != 0) & (e[:, 0] != 0) & (e[:, 1] != 0) & np.isfinite(k)
    return torch.from_numpy(np.where(ok, k, np.float32(0)).astype(np.float32))


def waveaug_mix_ref(x, lens, plan, z, coef) -> torch.Tensor:
    """y fp32 [B, S] from a plan, its noise rows and coefficients: two roundings per sample."""
    xv = np.asarray(torch.as_tensor(x).cpu())
    if xv.dtype != np.float32:
        xv = xv.astype(np.float32)                       # int16: exact
    zv = np.asarray(torch.as_tensor(z).cpu()).astype(np.float32)
    k = np.asarray(torch.as_tensor(coef).cpu()).astype(np.float32)
    on = np.asarray(torch.as_tensor(plan).cpu())[:, 0] != 0
    B, S = xv.shape
    valid = np.arange(S)[None, :] < waveaug_lens(lens, B, S)[:, None]
    with np.errstate(all="ignore"):
        mixed = (xv + (k[:, None] * zv).astype(np.float32)).astype(np.float32)
    y = np.where(on[:, None], mixed, xv)
    return torch.from_numpy(np.where(valid, y, np.float32(0)).astype(np.float32))


def waveaug_ref(x, lens, bank, policy, seed: int, step: int, first_utt: int = 0):
    """(y, plan, energy, coef) of the definition; ``bank`` has data, start, length."""
    x = torch.as_tensor(x)
    B, S = x.shape
    plan = waveaug_plan_ref(lens, B, S, bank.length, policy, seed, step, first_utt)
    z = waveaug_noise_ref(plan, bank.data, bank.start, bank.length, S)
    energy = waveaug_energy_ref(x, lens, z)
    coef = waveaug_coef_ref(plan, energy)
    return waveaug_mix_ref(x, lens, plan, z, coef), plan, energy, coef


# ---------------------------------------------------------------------------- speed perturbation (ops/speed.py, csrc/speed.hip)
# Definition shared by the kernels, the torch composite and the tests. A policy is V distinct
# integer percents p_0 .. p_{V-1}, 1 <= V <= 8, 50 <= p <= 200. Variant p != 100 resamples with
# (L, M, K, h) = resample_table(in_rate=p, out_rate=100), h rounded to fp32 once; p == 100 is the
# identity, a bit copy (never the L = M = 1 filter, which would low-pass the signal). Per
# utterance of x [B, S] with n = clamp(lens[b], 0, S):
#   plan   (pct, n_out) from one Philox4x32-10 block, key seed, counter (1, u, step & 0xffffffff,
#          WAVEAUG_STREAM | (step >> 32) & 0x3fffffff), u = first_utt + b: the noise plan's stream
#          with first word 1. v = U(x0, V), cand = ceil(n L_v / M_v) (n for the identity); the row
#          is (p_v, cand), or (100, n) by selection when n == 0, cand < min_out[b] or
#          (max_out > 0 and) cand > max_out
#   y      fp32 [B, S_out]: a perturbed row is resample_ref of that row alone (one fp32 fma chain
#          in ascending k on the device; fp64 rounded once here), an identity row fp32(x[j]);
#          every column at or past n_out is +0 whatever x holds past n
#   S_out  a multiple of 160: speed_out_width (the worst case over the policy), or the tight
#          width of a plan computed from a host copy of the lengths
SPEED_MAX_V = 8
SPEED_MIN_PCT, SPEED_MAX_PCT = 50, 200
SPEED_HOP = 160


def speed_pcts(policy) -> Tuple[int, ...]:
    return tuple(int(p) for p in getattr(policy, "pcts", policy))


def speed_out_len(n: int, pct: int) -> int:
    """Samples of an n-sample row played at pct percent of its speed."""
    if int(pct) == 100:
        return int(n)
    g = int(np.gcd(int(pct), 100))
    return resample_out_len(n, 100 // g, int(pct) // g)


def speed_round_width(n: int) -> int:
    """The smallest multiple of one hop (and at least one) that holds n samples."""
    return max(1, -(-int(n) // SPEED_HOP)) * SPEED_HOP


def speed_out_width(S: int, policy) -> int:
    """The output width that holds any row of S samples under any variant of the policy (a row
    may always fall back to the identity)."""
    return speed_round_width(max([int(S)] + [speed_out_len(S, p) for p in speed_pcts(policy)]))


def speed_plan_ref(lens, B: int, S: int, policy, seed: int, step: int, first_utt: int = 0, min_out=None,
                   max_out: int = 0) -> torch.Tensor:
    """The plan [B, 2] int32 = (pct, n_out) of utterances first_utt .. first_utt + B - 1 at ``step``,
    in exact integer arithmetic."""
    pcts = speed_pcts(policy)
    n = waveaug_lens(lens, B, S)
    u = (int(first_utt) + np.arange(B, dtype=np.uint64)) & np.uint64(0xffffffff)
    x = philox4x32((np.uint64(1), u, np.uint64(step & 0xffffffff),
                    np.uint64(WAVEAUG_STREAM | ((step >> 32) & 0x3fffffff))),
                   (np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)))
    x0 = np.broadcast_to(x[0], (B,)).astype(np.uint64)
    v = ((x0 * np.uint64(len(pcts))) >> np.uint64(32)).astype(np.int64)
    pct = np.asarray(pcts, np.int64)[v]
    cand = np.array([speed_out_len(int(n[b]), int(pct[b])) for b in range(B)], np.int64)
    lo = np.zeros(B, np.int64) if min_out is None else \
        np.asarray(torch.as_tensor(min_out).cpu()).astype(np.int64).reshape(-1)
    back = (n == 0) | (cand < lo) | ((int(max_out) > 0) & (cand > int(max_out)))
    plan = np.stack([np.where(back, 100, pct), np.where(back, n, cand)], 1)
    return torch.from_numpy(plan.astype(np.int32))


def speed_ref(x, lens, plan, out_width: int, return_abs: bool = False):
    """(y fp32 [B, out_width], out_lens int32 [B]) of the definition from a plan; ``return_abs``:
    (y64, a64, out_lens), the fp64 values and sum_k |h x| per output (|x| on identity rows)."""
    xv = np.asarray(torch.as_tensor(x).cpu())
    B, S = xv.shape
    n = waveaug_lens(lens, B, S)
    plan = np.asarray(torch.as_tensor(plan).cpu()).astype(np.int64)
    W = int(out_width)
    y = np.zeros((B, W), np.float64)
    a = np.zeros((B, W), np.float64)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        pct, c = int(plan[b, 0]), int(min(max(plan[b, 1], 0), W))
        row = xv[b, :n[b]].astype(np.float64)
        if pct == 100:
            c = min(c, int(n[b]))
            y[b, :c], a[b, :c] = row[:c], np.abs(row[:c])
        elif c > 0:
            r, ra = resample_ref(row, pct, 100, return_abs=True)
            y[b, :c], a[b, :c] = r[:c], ra[:c]
        cnt[b] = c
    if return_abs:
        return y, a, torch.from_numpy(cnt)
    return torch.from_numpy(y.astype(np.float32)), torch.from_numpy(cnt)
