"""csrc/ctc.hip (ds2_ctc_fused, ds2_head_ctc, ds2_fc_logits) against the fp64 oracle of
tests/ctc_cases.py, per utterance and per element.

Bounds. Every error is measured against the fp64 oracle, and so is e_ref, the error of the plain
fp32 computation (ops/reference.py ctc_loss_ref on the CPU with autograd gradients; the fp32 addmm
for the FC head) under the same metric. The kernel must stay within max(8 * e_ref, floor):
  loss            |l - o| / |o| per utterance, floor 1e-4 (1e-3 for the long-label cases)
  gradient norm   |g_b - o_b| / |o_b| over the utterance's valid frames, floor 1e-4 for fp32
                  output, 2^-8 for bf16 output (bf16 keeps 8 significant bits: one rounding moves
                  an element by at most 2^-8 of itself, so the vector by at most 2^-8 of its norm)
  element         |g - o| per element; floor 1e-4 * max|o_b| for fp32 output (the norm floor at
                  element granularity), 2^-8 |o| + 2^-8 max|o_b| for bf16 output
  fc_logits       floor H 2^-24 (sum_i |h_i w_i| + |bias|) per element, the a-priori bound of an
                  fp32 dot product of H terms in any order; plus the bf16 element floor for bf16 out
  dh (bf16)       per-utterance norm floor 2^-7: two bf16 roundings (G, then dh) of 2^-8 each;
                  dW, db (fp32 sums of the bf16 G) 2^-8
Frames past the length, infeasible rows and G's padding columns are exactly zero. The oracle is
given the bf16-rounded inputs of a bf16 case, so input rounding is no kernel error.

Measured on an MI355X, worst utterance of each family, kernel / e_ref (each test prints its own):
  family                          loss             gradient norm     element
  (a) tiles, bf16 logits          1.1e-6 / 8.4e-7  2.2e-3 / 2.3e-3   4.8e-3 / 4.1e-3
  (a) tiles 127 and 1023, fp32    6.7e-7 / 1.4e-6  3.5e-3 / 5.4e-3   7.4e-3 / 8.2e-3
  (b) edge batch, fp32            3.9e-7 / 3.8e-7  1.1e-4 / 1.8e-4   2.7e-4 / 3.0e-4
  (b) edge batch, bf16            2.0e-7 / 1.1e-7  1.7e-3 / 7.3e-5   2.1e-3 / 1.3e-4
  (b) all targets empty, fp32     3.6e-7 / 3.3e-7  1.8e-4 / 2.0e-4   3.1e-4 / 3.4e-4
  (b) all targets empty, bf16     1.3e-7 / 1.1e-7  1.3e-3 / 7.9e-5   2.1e-3 / 1.7e-4
  (c) single path, fp32           9.9e-8 / 9.2e-8  4.0e-5 / 4.4e-5   9.2e-5 / 9.9e-5
  (d) blank and K, fp32           2.4e-7 / 2.3e-7  8.3e-5 / 4.8e-5   1.2e-4 / 1.0e-4
  (e) dynamic range, fp32         3.8e-7 / 1.1e-7  2.9e-3 / 2.0e-3   5.9e-3 / 6.3e-3
  (h) head_ctc, G in bf16         3.7e-6 / 3.2e-7  2.9e-3 / 2.2e-4   2.1e-3 / 3.3e-4
  (g) fc_logits fp32 out          element 3.4e-6 / 1.4e-6, at most 0.03 of its bound
  (g) fc_logits bf16 out          element 1.6e-2 / 1.4e-6, at most 0.49 of its bound (bf16 rounding)
  (h) FusedHeadCTC                dh 2.4e-3 / 2.2e-4 per utterance, dW 1.3e-3 / 1.2e-4, db 2.4e-4 / 1.4e-4
With fp32 output the kernel sits at the error of the plain fp32 computation, which itself misses
1e-4 per utterance on long lattices (the subtraction alpha + beta - logP cancels ~1e3 nats); with
bf16 output the output rounding dominates. (f) holds bitwise.

Which test executes what: ctc_recur_kernel<4, 5, 6, 8, 12, 16, 32> test_every_register_tile_width
[127 .. 1023] in this order (<4> also every other CTC test here); fc_lsm_kernel<float> with logits
out test_fc_logits[*-float32], with lp out test_head_ctc; fc_lsm_kernel<bf16> test_fc_logits[*-bfloat16];
the > 64 KB LDS opt-in test_fc_logits[1024-*] and test_head_ctc[wide]; ctc_grad_lp_kernel's
in-launch mean over more than 64 utterances test_head_ctc[many].
"""
import functools
import math

import numpy as np
import pytest
import torch

import ctc_cases as CC
from align_cases import pad_labels

from deepspeech_amd.ops import reference as R

pytestmark = pytest.mark.gpu

LOSS_FLOOR, LONG_LOSS_FLOOR, NORM_FLOOR, BF16 = 1e-4, 1e-3, 1e-4, 2.0 ** -8
NAN = float("nan")


def _ext():
    from deepspeech_amd.ops import _ext as E
    return E.ext()


def _i32(v, dev):
    return torch.as_tensor(v, dtype=torch.int32).to(dev).contiguous()


def _run_fused(cuda, x, lens, lab, ll, blank, zero_inf=True):
    """Raw ds2_ctc_fused on NaN-filled outputs and a NaN-filled workspace: anything the kernels
    leave unwritten, or read without having written it, shows up in the comparison."""
    C = _ext()
    T, N, K = x.shape
    xd = x.to(cuda).contiguous()
    loss = torch.full((N,), NAN, device=cuda)
    grad = torch.full_like(xd, NAN)
    ws = torch.full((int(C.ctc_ws_floats(T, N, lab.shape[1])),), NAN, device=cuda)
    C.ctc_fused(xd, _i32(lens, cuda), _i32(lab, cuda), _i32(ll, cuda), loss, grad, ws, blank, zero_inf)
    torch.cuda.synchronize()
    return loss.cpu(), grad.cpu()


def _clamped(lens, lab, ll, T):
    return [min(int(v), T) for v in lens], [min(int(v), lab.shape[1]) for v in ll]


def _ref32(x, lens, lab, ll, blank, o_loss):
    """e_ref's computation: fp32 log-softmax + F.ctc_loss on the CPU, autograd gradient. Rows the
    oracle calls infeasible are handed over as empty one-frame rows: nothing of them is used."""
    T = x.shape[0]
    lens, ll = _clamped(lens, lab, ll, T)
    for b in range(len(lens)):
        if math.isinf(o_loss[b]):
            lens[b], ll[b] = 1, 0
    xr = x.float().clone().requires_grad_(True)
    if lab.shape[1] == 0:
        lab = torch.zeros(lab.shape[0], 1, dtype=torch.int32)
    lr = R.ctc_loss_ref(xr, lab.long(), torch.tensor(lens), torch.tensor(ll), blank=blank)
    lr.sum().backward()
    return lr.detach().double().numpy(), xr.grad.double().numpy()


def _oracle_and_ref(x, lens, lab, ll, blank):
    want = CC.ctc_oracle(x.double(), lens, lab, ll, blank)
    return want, _ref32(x, lens, lab, ll, blank, want[0])


def _check(tag, loss, grad, want, ref, lens, zero_inf=True, bf16_out=False, loss_floor=LOSS_FLOOR):
    """Every utterance and every element of loss [N] / grad [T, N, K] against the oracle."""
    o_loss, o_grad = want
    r_loss, r_grad = ref
    loss = loss.double().numpy()
    grad = grad.double().numpy()
    T, N, _ = grad.shape
    worst = dict(loss=0.0, loss_ref=0.0, norm=0.0, norm_ref=0.0, elem=0.0, elem_ref=0.0)
    for b in range(N):
        n = max(0, min(int(lens[b]), T))
        g = grad[:, b]
        if math.isinf(o_loss[b]):
            assert loss[b] == (0.0 if zero_inf else math.inf), (tag, b, loss[b])
            assert not g.any(), (tag, b, "gradient of an infeasible row")
            continue
        assert not g[n:].any(), (tag, b, "gradient past the length")
        o, r = o_grad[:n, b], r_grad[:n, b]
        # (a -inf logit makes torch's backward NaN over that frame: e_ref is taken over the
        # reference's finite elements, the kernel is compared on every element)
        fin = np.isfinite(r)
        e_l, e_l_ref = abs(loss[b] - o_loss[b]) / abs(o_loss[b]), abs(r_loss[b] - o_loss[b]) / abs(o_loss[b])
        on = np.linalg.norm(o)
        e_n, e_n_ref = np.linalg.norm(g[:n] - o) / on, np.linalg.norm(np.where(fin, r - o, 0.0)) / on
        d, d_ref = np.abs(g[:n] - o), float(np.abs(np.where(fin, r - o, 0.0)).max())
        omax = np.abs(o).max()
        floor_e = BF16 * np.abs(o) + BF16 * omax if bf16_out else np.full_like(o, NORM_FLOOR * omax)
        bound_e = np.maximum(8 * d_ref, floor_e)
        print("ctc-err %s b=%d len=%d loss %.3e (ref %.3e) norm %.3e (ref %.3e) elem %.3e (ref %.3e, bound use %.2f)"
              % (tag, b, n, e_l, e_l_ref, e_n, e_n_ref, d.max(), d_ref, float((d / bound_e).max())))
        for k, v in (("loss", e_l), ("loss_ref", e_l_ref), ("norm", e_n), ("norm_ref", e_n_ref), ("elem", d.max()),
                     ("elem_ref", d_ref)):
            worst[k] = max(worst[k], float(v))
        assert e_l <= max(8 * e_l_ref, loss_floor), (tag, b, "loss", loss[b], o_loss[b], e_l, e_l_ref)
        assert e_n <= max(8 * e_n_ref, BF16 if bf16_out else NORM_FLOOR), (tag, b, "gradient norm", e_n, e_n_ref)
        bad = np.argwhere(~(d <= bound_e))
        assert bad.size == 0, (tag, b, "element", bad[:4].tolist(), float(d.max()), d_ref)
    print("ctc-worst %s %s" % (tag, " ".join("%s=%.2e" % kv for kv in worst.items())))
    return worst


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


# --------------------------------------------------------------------------- (a) register tiles
@pytest.mark.parametrize("Lmax,dtype", [(L, torch.bfloat16) for L in CC.LONG_LMAX]
                         + [(127, torch.float32), (1023, torch.float32)])
def test_every_register_tile_width(cuda, Lmax, dtype):
    """2 Lmax + 1 = 64 SPL - 1 lattice states: one case per ctc_recur_kernel instantiation with
    lane 63's registers in use; row 0 is feasible by 20 frames (Lmax + 20 repeats in Lmax + 40)."""
    spl = CC.expected_spl(Lmax)
    assert 2 * Lmax + 1 == 64 * spl - 1
    T, N, K = Lmax + 40, 3, 29
    assert _ext().ctc_ws_floats(T, N, Lmax) == N * T * (32 + 2 * 64 * spl) + N
    rows, lens = CC.long_rows(Lmax), CC.long_lens(Lmax)
    lab, ll = pad_labels(rows)
    assert lab.shape[1] == Lmax
    x = CC.ctc_logits(T, N, K, seed=Lmax, sharp=1.5).to(dtype)
    want, ref = _oracle_and_ref(x.float(), lens, lab, ll, 28)
    assert np.isfinite(want[0]).all()
    loss, grad = _run_fused(cuda, x, lens, lab, ll, 28)
    _check("tile%d-%s" % (Lmax, str(dtype)[6:]), loss, grad, want, ref, lens, bf16_out=dtype == torch.bfloat16,
           loss_floor=LONG_LOSS_FLOOR)


def test_1024_labels_are_rejected(cuda):
    T, N, K = 8, 2, 29
    lab = torch.zeros(N, 1024, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"code -21"):
        _run_fused(cuda, CC.ctc_logits(T, N, K, seed=0), [T, T], lab, [1, 1], 28)


# --------------------------------------------------------------------------- (b) edge batch
@functools.lru_cache(maxsize=None)
def _edge(dtype):
    x = CC.ctc_logits(CC.EDGE_T, 8, 29, seed=40).to(dtype)
    lab, ll = pad_labels(CC.edge_rows(0))
    want, ref = _oracle_and_ref(x.float(), CC.EDGE_LENS, lab, ll, 28)
    for a in want + ref:
        a.setflags(write=False)
    return x, lab, ll, want, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_edge_batch(cuda, dtype):
    """lens at the 64-frame staging edges, L = 0, L == len, one label in two frames; then the
    same batch with a len past T and a label length past the padded width: bitwise the same."""
    x, lab, ll, want, ref = _edge(dtype)
    assert np.isfinite(want[0]).all()
    loss, grad = _run_fused(cuda, x, CC.EDGE_LENS, lab, ll, 28)
    _check("edge-%s" % str(dtype)[6:], loss, grad, want, ref, CC.EDGE_LENS, bf16_out=dtype == torch.bfloat16)
    lens2, ll2 = list(CC.EDGE_LENS), ll.clone()
    lens2[7] += 3
    ll2[6] = lab.shape[1] + 5
    loss2, grad2 = _run_fused(cuda, x, lens2, lab, ll2, 28)
    assert _bits(loss2) == _bits(loss) and _bits(grad2) == _bits(grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_edge_batch_all_targets_empty(cuda, dtype):
    """A [N, 0] label tensor through ops/ctc.py (which substitutes one zero column)."""
    from deepspeech_amd.ops import ctc as CTC
    x = _edge(dtype)[0]
    lab = torch.zeros(8, 0, dtype=torch.int32)
    ll = torch.zeros(8, dtype=torch.int32)
    want, ref = _oracle_and_ref(x.float(), CC.EDGE_LENS, lab, ll, 28)
    xd = x.to(cuda).requires_grad_(True)
    loss = CTC.ctc_loss_hip(xd, _i32(CC.EDGE_LENS, cuda), lab.to(cuda), ll.to(cuda), 28)
    loss.sum().backward()
    _check("empty-%s" % str(dtype)[6:], loss.detach().cpu(), xd.grad.cpu(), want, ref, CC.EDGE_LENS,
           bf16_out=dtype == torch.bfloat16)


# --------------------------------------------------------------------------- (c) single path
def test_single_path_and_repeat_infeasible_rows(cuda):
    """[c]*L in 2L-1 frames has one path; in 2L-2 frames none, though L <= len: the recursion
    runs and ends on its log 0. zero_inf picks 0 or +inf for the loss; the gradient of such a
    row is exactly zero either way and the feasible neighbours do not notice."""
    rows, lens = CC.single_path_rows(1)
    lab, ll = pad_labels(rows)
    x = CC.ctc_logits(CC.SINGLE_T, len(rows), 29, seed=41)
    want, ref = _oracle_and_ref(x, lens, lab, ll, 28)
    assert [math.isinf(v) for v in want[0]] == [CC.infeasible(r, n) for r, n in zip(rows, lens)]
    assert sum(math.isinf(v) for v in want[0]) == 3 and lens.count(0) == 1
    lp = CC.log_softmax64(x.double().numpy())
    for b in range(3):                                   # the oracle on these rows is the one path
        path = [rows[b][0] if t % 2 == 0 else 28 for t in range(lens[b])]
        assert abs(want[0][b] + sum(lp[t, b, c] for t, c in enumerate(path))) <= 1e-12 * want[0][b]
    out = {}
    for zero_inf in (True, False):
        out[zero_inf] = _run_fused(cuda, x, lens, lab, ll, 28, zero_inf)
        _check("single-zi%d" % zero_inf, *out[zero_inf], want, ref, lens, zero_inf=zero_inf)
    for b in range(len(rows)):
        if not math.isinf(want[0][b]):
            assert _bits(out[True][0][b]) == _bits(out[False][0][b])
            assert _bits(out[True][1][:, b]) == _bits(out[False][1][:, b])


# --------------------------------------------------------------------------- (d) blank and K
@pytest.mark.parametrize("K,blank", CC.KB_CASES)
def test_blank_position_and_class_count(cuda, K, blank):
    """T N = 350 frames: the last block of ctc_lsm / ctc_grad holds two waves."""
    rows = CC.kb_rows(2, K, blank)
    lab, ll = pad_labels(rows)
    x = CC.ctc_logits(CC.KB_T, 5, K, seed=42 + K + blank)
    want, ref = _oracle_and_ref(x, CC.KB_LENS, lab, ll, blank)
    assert np.isfinite(want[0]).all()
    loss, grad = _run_fused(cuda, x, CC.KB_LENS, lab, ll, blank)
    _check("kb%d-%d" % (K, blank), loss, grad, want, ref, CC.KB_LENS)


# --------------------------------------------------------------------------- (e) dynamic range
def test_dynamic_range(cuda):
    """Logits x 40: log-probs to ~-300 nats a frame, logP ~ -1e4 over 200 frames, and one -inf
    logit on a class outside the label. Finite, feasible, and on the oracle."""
    T, N, K = 200, 4, 29
    rng = np.random.default_rng(3)
    rows = [CC.random_labels(rng, L, K, 28) for L in (40, 1, 80, 0)]
    lens = [200, 150, 199, 64]
    x = CC.ctc_logits(T, N, K, seed=30, sharp=40.0)
    x[17, 0, next(c for c in range(28) if c not in rows[0])] = -math.inf
    lab, ll = pad_labels(rows)
    want, ref = _oracle_and_ref(x, lens, lab, ll, 28)
    assert np.isfinite(want[0]).all() and want[0].min() > 5e3
    loss, grad = _run_fused(cuda, x, lens, lab, ll, 28, zero_inf=False)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    _check("range", loss, grad, want, ref, lens, zero_inf=False)


# --------------------------------------------------------------------------- (f) invariance
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_composition_invariance(cuda, dtype):
    """An utterance's loss and gradient do not depend on its neighbours or its slot: the edge
    batch, its reverse, and every utterance alone (same padded label width), bitwise."""
    x, lab, ll, _, _ = _edge(dtype)
    lens = CC.EDGE_LENS
    loss, grad = _run_fused(cuda, x, lens, lab, ll, 28)
    rev = list(range(7, -1, -1))
    loss_r, grad_r = _run_fused(cuda, x[:, rev], [lens[b] for b in rev], lab[rev], ll[rev], 28)
    for i, b in enumerate(rev):
        assert _bits(loss_r[i]) == _bits(loss[b]), ("reversed", b)
        assert _bits(grad_r[:, i]) == _bits(grad[:, b]), ("reversed", b)
    for b in range(8):
        l1, g1 = _run_fused(cuda, x[:, b:b + 1], lens[b:b + 1], lab[b:b + 1], ll[b:b + 1], 28)
        assert _bits(l1[0]) == _bits(loss[b]), ("alone", b)
        assert _bits(g1[:, 0]) == _bits(grad[:, b]), ("alone", b)


# --------------------------------------------------------------------------- (g) fc_logits
def _head_operands(M, H, K, seed):
    g = torch.Generator().manual_seed(seed)
    h = (0.5 * torch.randn(M, H, generator=g)).bfloat16()
    W = (torch.randn(K, H, generator=g) * (3.0 / math.sqrt(H))).bfloat16()     # logits of std ~1.5
    bias = (0.5 * torch.randn(K, generator=g)).bfloat16()
    return h, W, bias


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [32, 160, 192, 1024])
def test_fc_logits(cuda, H, out_dtype):
    """H = 32 one K-step, 160 one full chunk of 5 fragments, 192 the clamped tail, 1024 the
    > 64 KB LDS opt-in; M below a wave tile, one short of it, a tail inside a block, two blocks
    and a 2-row tail; K = 5, 29, 32. Against the fp64 product of the bf16 operands."""
    C = _ext()
    bf = out_dtype == torch.bfloat16
    worst = [0.0, 0.0, 0.0]
    for K in (5, 29, 32):
        for M in (1, 15, 111, 130):
            h, W, bias = _head_operands(M, H, K, seed=H + K + M)
            o = (h.double() @ W.double().t() + bias.double()).numpy()
            mass = (h.double().abs() @ W.double().abs().t() + bias.double().abs()).numpy()
            r = torch.addmm(bias.float(), h.float(), W.float().t()).double().numpy()
            out = torch.full((M + 2, K), NAN, device=cuda, dtype=out_dtype)       # a canary row either side
            C.fc_logits(h.to(cuda), W.to(cuda), bias.to(cuda), out[1:M + 1])
            torch.cuda.synchronize()
            assert torch.isnan(out[0]).all() and torch.isnan(out[M + 1]).all(), (K, M)
            got = out[1:M + 1].cpu().double().numpy()
            d, e_ref = np.abs(got - o), float(np.abs(r - o).max())
            floor = H * 2.0 ** -24 * mass
            if bf:
                floor = floor + BF16 * np.abs(o) + BF16 * np.abs(o).max(axis=1, keepdims=True)
            bound = np.maximum(8 * e_ref, floor)
            worst = [max(worst[0], float(d.max())), max(worst[1], e_ref), max(worst[2], float((d / bound).max()))]
            bad = np.argwhere(~(d <= bound))
            assert bad.size == 0, (K, M, bad[:4].tolist(), float(d.max()), e_ref)
    print("ctc-worst fc H=%d %s elem=%.2e elem_ref=%.2e bound use %.2f" % (H, str(out_dtype)[6:], *worst))


# --------------------------------------------------------------------------- (h) head_ctc
def _head_case(name):
    """(T, N, H, K, blank, lens, rows)"""
    if name == "edge":
        return 129, 8, 192, 29, 28, CC.EDGE_LENS, CC.edge_rows(0)
    if name == "kb":
        return 70, 5, 32, 5, 4, CC.KB_LENS, CC.kb_rows(2, 5, 4)
    rng = np.random.default_rng(7)
    if name == "many":       # N > 64: the in-launch mean takes two passes over the batch
        return 3, 70, 32, 5, 4, [1 + b % 3 for b in range(70)], [[b % 4] * (b % 2) for b in range(70)]
    if name == "short":
        return 37, 3, 160, 29, 28, [37, 20, 1], [CC.random_labels(rng, 10, 29, 28),
                                                 CC.labels_no_repeat(rng, 20, 29, 28), []]
    assert name == "wide"
    return 20, 5, 1024, 32, 31, [20, 7, 13, 1, 20], [CC.random_labels(rng, 5, 32, 31), [30] * 4, [], [0],
                                                     CC.labels_with_repeats(rng, 8, 32, 31, 2)]


def _run_head(cuda, h, W, bias, lens, lab, ll, blank, zero_inf=True, counter0=7):
    C = _ext()
    T, N, H = h.shape
    loss = torch.full((N,), NAN, device=cuda)
    G = torch.full((T * N, 32), NAN, device=cuda, dtype=torch.bfloat16)
    ws = torch.full((int(C.ctc_ws_floats(T, N, lab.shape[1])),), NAN, device=cuda)
    mean = torch.full((1,), NAN, device=cuda)
    counter = torch.tensor([counter0], dtype=torch.int32, device=cuda)
    first_bad = torch.tensor([-1], dtype=torch.int32, device=cuda)
    C.head_ctc(h.to(cuda), W.to(cuda), bias.to(cuda), _i32(lens, cuda), _i32(lab, cuda), _i32(ll, cuda), loss, G, ws,
               blank, zero_inf, mean=mean, counter=counter, first_bad=first_bad)
    torch.cuda.synchronize()
    return loss.cpu(), G.cpu(), float(mean.item()), int(counter.item()), int(first_bad.item())


def _head_oracle(h, W, bias, lens, lab, ll, blank):
    """The oracle on the fp64 logits of the bf16 operands; e_ref from the fp32 addmm's logits."""
    T, N, H = h.shape
    logits = (h.double().view(T * N, H) @ W.double().t() + bias.double()).view(T, N, -1)
    want = CC.ctc_oracle(logits, lens, lab, ll, blank)
    l32 = torch.addmm(bias.float(), h.float().view(T * N, H), W.float().t()).view(T, N, -1)
    return want, _ref32(l32, lens, lab, ll, blank, want[0])


@pytest.mark.parametrize("name", ["short", "edge", "wide", "kb", "many"])
def test_head_ctc(cuda, name):
    """Raw ds2_head_ctc: per-utterance loss, G per utterance and per element, zero padding
    columns and zero rows past the length, the in-launch batch mean and the divergence watch."""
    T, N, H, K, blank, lens, rows = _head_case(name)
    lab, ll = pad_labels(rows)
    h, W, bias = _head_operands(T * N, H, K, seed=50 + H)
    h = h.view(T, N, H)
    want, ref = _head_oracle(h, W, bias, lens, lab, ll, blank)
    assert np.isfinite(want[0]).all()
    loss, G, mean, counter, first_bad = _run_head(cuda, h, W, bias, lens, lab, ll, blank)
    assert not G[:, K:].double().numpy().any(), "padding columns of G"
    _check("head-" + name, loss, G[:, :K].reshape(T, N, K), want, ref, lens, bf16_out=True)
    total = loss.double().sum().item()
    assert abs(mean - total / N) <= 2.0 ** -24 * (N + 1) * loss.double().abs().sum().item() / N, (mean, total / N)
    assert counter == 8 and first_bad == -1
    if name == "edge":       # a len past T, a label length past the padded width: bitwise the clamped call
        lens2, ll2 = list(lens), ll.clone()
        lens2[7] += 3
        ll2[6] = lab.shape[1] + 5
        loss2, G2, mean2, _, _ = _run_head(cuda, h, W, bias, lens2, lab, ll2, blank)
        assert _bits(loss2) == _bits(loss) and _bits(G2) == _bits(G) and mean2 == mean


def test_head_ctc_infeasible_row_and_watch(cuda):
    """One row infeasible through a repeat alone, one without frames. zero_inf: they count 0 in
    the mean and the watch stays clear; without it the mean is +inf and the watch records the
    step. G of those rows is exactly zero both times, the neighbour is bitwise the same."""
    T, N, H, K, blank, lens, rows = _head_case("short")
    rows = [rows[0], rows[1][:10] + rows[1][9:19], [5]]              # 20 labels, one repeat, 20 frames
    lens = [lens[0], lens[1], 0]
    assert CC.infeasible(rows[1], lens[1]) and len(rows[1]) <= lens[1]
    lab, ll = pad_labels(rows)
    h, W, bias = _head_operands(T * N, H, K, seed=50 + H)
    h = h.view(T, N, H)
    want, ref = _head_oracle(h, W, bias, lens, lab, ll, blank)
    assert [math.isinf(v) for v in want[0]] == [False, True, True]
    out = {}
    for zero_inf in (True, False):
        loss, G, mean, counter, first_bad = out[zero_inf] = _run_head(cuda, h, W, bias, lens, lab, ll, blank, zero_inf,
                                                                       counter0=11)
        assert not G[:, K:].double().numpy().any()
        _check("head-inf-zi%d" % zero_inf, loss, G[:, :K].reshape(T, N, K), want, ref, lens, zero_inf=zero_inf,
               bf16_out=True)
        assert counter == 12
        if zero_inf:
            fin = loss.double().sum().item() / N
            assert abs(mean - fin) <= 2.0 ** -24 * (N + 1) * abs(fin) and first_bad == -1
        else:
            assert mean == math.inf and first_bad == 11
    assert _bits(out[True][0][0]) == _bits(out[False][0][0])
    assert _bits(out[True][1].view(T, N, 32)[:, 0]) == _bits(out[False][1].view(T, N, 32)[:, 0])


def test_fused_head_ctc_gradients(cuda):
    """ops/ctc.py FusedHeadCTC on the edge batch: dh per utterance, dW and db, against the fp64
    chain rule through the oracle's gradient (mean loss: dlogits = oracle gradient / N)."""
    from deepspeech_amd.ops import ctc as CTC
    T, N, H, K, blank, lens, rows = _head_case("edge")
    lab, ll = pad_labels(rows)
    h, W, bias = _head_operands(T * N, H, K, seed=50 + H)
    h = h.view(T, N, H)
    (o_loss, o_grad), _ = _head_oracle(h, W, bias, lens, lab, ll, blank)
    dl = torch.from_numpy(o_grad) / N
    dh_o = (dl.view(T * N, K) @ W.double()).view(T, N, H)
    dW_o = dl.view(T * N, K).t() @ h.double().view(T * N, H)
    db_o = dl.view(T * N, K).sum(0)
    # e_ref: the same chain in fp32 on the CPU
    hr, Wr, br = (t.float().clone().requires_grad_(True) for t in (h, W, bias))
    lr = R.ctc_loss_ref(hr @ Wr.t() + br, lab.long(), torch.tensor(lens), ll.long(), blank=blank).mean()
    lr.backward()
    hx = h.to(cuda).requires_grad_(True)
    Wx, bx = W.float().to(cuda).requires_grad_(True), bias.float().to(cuda).requires_grad_(True)
    loss = CTC.head_ctc_mean_loss_hip(hx, Wx, bx, _i32(lens, cuda), lab.to(cuda), ll.to(cuda), blank)
    loss.backward()
    torch.cuda.synchronize()
    e_l, e_l_ref = abs(loss.item() - o_loss.mean()) / o_loss.mean(), abs(lr.item() - o_loss.mean()) / o_loss.mean()
    assert e_l <= max(8 * e_l_ref, LOSS_FLOOR), (loss.item(), o_loss.mean(), e_l_ref)

    def rel(a, o):
        return float(torch.linalg.norm(a.double() - o) / torch.linalg.norm(o))

    dh = hx.grad.cpu()
    for b in range(N):
        n = lens[b]
        assert not dh[n:, b].double().numpy().any(), (b, "dh past the length")
        e, e_ref = rel(dh[:n, b], dh_o[:n, b]), rel(hr.grad[:n, b], dh_o[:n, b])
        print("ctc-err fused-head dh b=%d %.3e (ref %.3e)" % (b, e, e_ref))
        assert e <= max(8 * e_ref, 2 * BF16), (b, e, e_ref)
    for nm, a, r, o in (("dW", Wx.grad.cpu(), Wr.grad, dW_o), ("db", bx.grad.cpu(), br.grad, db_o)):
        e, e_ref = rel(a, o), rel(r, o)
        print("ctc-err fused-head %s %.3e (ref %.3e)" % (nm, e, e_ref))
        assert e <= max(8 * e_ref, BF16), (nm, e, e_ref)


def test_fused_head_ctc_all_targets_empty(cuda):
    """A [N, 0] label tensor through FusedHeadCTC (ops/ctc.py substitutes one zero column): the
    mean loss and dh per utterance."""
    from deepspeech_amd.ops import ctc as CTC
    T, N, H, K, blank, lens, _ = _head_case("short")
    lab, ll = torch.zeros(N, 0, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    h, W, bias = _head_operands(T * N, H, K, seed=50 + H)
    h = h.view(T, N, H)
    (o_loss, o_grad), (r_loss, r_grad) = _head_oracle(h, W, bias, lens, lab, ll, blank)
    dh_o = ((torch.from_numpy(o_grad) / N).view(T * N, K) @ W.double()).view(T, N, H)
    dh_r = ((torch.from_numpy(r_grad) / N).view(T * N, K) @ W.double()).view(T, N, H)
    hx = h.to(cuda).requires_grad_(True)
    loss = CTC.head_ctc_mean_loss_hip(hx, W.float().to(cuda), bias.float().to(cuda), _i32(lens, cuda), lab.to(cuda),
                                      ll.to(cuda), blank)
    loss.backward()
    e_l, e_l_ref = abs(loss.item() - o_loss.mean()) / o_loss.mean(), abs(r_loss.mean() - o_loss.mean()) / o_loss.mean()
    assert e_l <= max(8 * e_l_ref, LOSS_FLOOR), (loss.item(), o_loss.mean(), e_l_ref)
    dh = hx.grad.cpu().double()
    for b in range(N):
        n = lens[b]
        assert not dh[n:, b].numpy().any(), (b, "dh past the length")
        e = float(torch.linalg.norm(dh[:n, b] - dh_o[:n, b]) / torch.linalg.norm(dh_o[:n, b]))
        e_ref = float(torch.linalg.norm(dh_r[:n, b] - dh_o[:n, b]) / torch.linalg.norm(dh_o[:n, b]))
        print("ctc-err fused-head-empty dh b=%d %.3e (ref %.3e)" % (b, e, e_ref))
        assert e <= max(8 * e_ref, 2 * BF16), (b, e, e_ref)
