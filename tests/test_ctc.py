"""The fp64 CTC oracle of tests/ctc_cases.py against brute-force path enumeration and against
torch's float64 CTC on the CPU: the oracle is what tests/test_ctc_gpu.py holds csrc/ctc.hip to."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_cases as CC
from align_cases import collapse, pad_labels


def _brute_logp(lp, label, blank):
    """log sum over all K^T frame paths that collapse to ``label`` (torch double, differentiable)."""
    T, K = lp.shape
    terms = [sum(lp[t, c] for t, c in enumerate(path))
             for path in itertools.product(range(K), repeat=T) if collapse(path, blank) == list(label)]
    return torch.logsumexp(torch.stack(terms), 0) if terms else None


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_oracle_against_path_enumeration(T):
    """K = 3, every label sequence of length 0..3 (repeats included), all of them in one batch."""
    K, blank = 3, 2
    seqs = [list(s) for L in range(4) for s in itertools.product(range(K - 1), repeat=L)]
    N = len(seqs)
    x = CC.ctc_logits(T, N, K, seed=T, sharp=1.5).double().requires_grad_(True)
    lab, ll = pad_labels(seqs)
    loss, grad = CC.ctc_oracle(x.detach(), [T] * N, lab, ll, blank)
    lp = torch.log_softmax(x, -1)
    total, feasible = 0.0, []
    for b, s in enumerate(seqs):
        logp = _brute_logp(lp[:, b], s, blank)
        assert (logp is None) == CC.infeasible(s, T) == math.isinf(loss[b]), (b, s)
        if logp is not None:
            assert abs(loss[b] + logp.item()) <= 1e-12 * max(1.0, abs(loss[b])), (b, s)
            total = total - logp
            feasible.append(b)
    total.backward()
    g = x.grad.numpy()
    assert len(feasible) > 0
    for b in range(N):
        if b in feasible:
            assert np.abs(grad[:, b] - g[:, b]).max() <= 1e-12, (b, seqs[b])
        else:
            assert not grad[:, b].any()


def test_oracle_short_frames_and_other_blank():
    """len < T (frames past it carry no gradient) and blank = 0, by enumeration."""
    K, blank, T = 3, 0, 6
    seqs, lens = [[1, 2], [2, 2], [1], []], [4, 5, 2, 3]
    x = CC.ctc_logits(T, 4, K, seed=9).double().requires_grad_(True)
    lab, ll = pad_labels(seqs)
    loss, grad = CC.ctc_oracle(x.detach(), lens, lab, ll, blank)
    lp = torch.log_softmax(x, -1)
    total = 0.0
    for b, s in enumerate(seqs):
        logp = _brute_logp(lp[: lens[b], b], s, blank)
        assert abs(loss[b] + logp.item()) <= 1e-12
        total = total - logp
    total.backward()
    assert np.abs(grad - x.grad.numpy()).max() <= 1e-12
    for b in range(4):
        assert not grad[lens[b]:, b].any()


def _torch64(x, lens, rows, blank):
    lab, ll = pad_labels(rows)
    xr = x.double().clone().requires_grad_(True)
    loss = F.ctc_loss(torch.log_softmax(xr, -1), lab.long(), torch.tensor(lens), ll.long(), blank=blank,
                      reduction="none", zero_infinity=True)
    loss.sum().backward()
    return loss.detach().numpy(), xr.grad.numpy()


def _against_torch64(x, lens, rows, blank):
    lab, ll = pad_labels(rows)
    loss, grad = CC.ctc_oracle(x.double(), lens, lab, ll, blank)
    tl, tg = _torch64(x, lens, rows, blank)
    seen = 0
    for b, r in enumerate(rows):
        assert math.isinf(loss[b]) == CC.infeasible(r, lens[b])
        if math.isinf(loss[b]):
            # torch reports 0 with zero_infinity; the gradient of such a row is compared for the
            # feasible rows only (torch's convention for it is its own), the oracle's is zero
            assert tl[b] == 0.0 and not grad[:, b].any()
            continue
        seen += 1
        assert abs(loss[b] - tl[b]) <= 1e-9 * max(1.0, abs(tl[b])), (b, loss[b], tl[b])
        assert np.abs(grad[:, b] - tg[:, b]).max() <= 1e-9, b
        assert not grad[lens[b]:, b].any()
    assert seen > 0


def test_oracle_against_torch_float64_edge_batch():
    _against_torch64(CC.ctc_logits(CC.EDGE_T, 8, 29, seed=20), CC.EDGE_LENS, CC.edge_rows(0), 28)


def test_oracle_against_torch_float64_single_path_batch():
    rows, lens = CC.single_path_rows(1)
    _against_torch64(CC.ctc_logits(CC.SINGLE_T, len(rows), 29, seed=21), lens, rows, 28)


@pytest.mark.parametrize("K,blank", CC.KB_CASES)
def test_oracle_against_torch_float64_blank_positions(K, blank):
    _against_torch64(CC.ctc_logits(CC.KB_T, 5, K, seed=22), CC.KB_LENS, CC.kb_rows(2, K, blank), blank)


def test_single_path_rows_have_one_path():
    """[c]*L in 2L-1 frames: loss = -sum of lp along c, blank, c, ..., gradient = softmax - one-hot."""
    rows, lens = CC.single_path_rows(1)
    x = CC.ctc_logits(CC.SINGLE_T, len(rows), 29, seed=23).double()
    lab, ll = pad_labels(rows)
    loss, grad = CC.ctc_oracle(x, lens, lab, ll, 28)
    lp = CC.log_softmax64(x.numpy())
    for b in range(3):
        path = [rows[b][0] if t % 2 == 0 else 28 for t in range(lens[b])]
        assert abs(loss[b] + sum(lp[t, b, c] for t, c in enumerate(path))) <= 1e-12 * loss[b]
        want = np.exp(lp[: lens[b], b])
        want[np.arange(lens[b]), path] -= 1.0
        assert np.abs(grad[: lens[b], b] - want).max() <= 1e-12


def test_infeasibility_predicate_on_every_table():
    """L + adjacent repeats > len is exactly where the oracle reports +inf."""
    n_inf = 0
    for name, rows, lens, K, blank in CC.all_tables():
        x = CC.ctc_logits(max(lens), len(rows), K, seed=5, sharp=1.0).double()
        lab, ll = pad_labels(rows)
        loss, _ = CC.ctc_oracle(x, lens, lab, ll, blank)
        for b, r in enumerate(rows):
            assert math.isinf(loss[b]) == CC.infeasible(r, lens[b]), (name, b)
            n_inf += math.isinf(loss[b])
    assert n_inf >= 3


def test_oracle_clamps_lengths():
    rows = CC.edge_rows(0)
    x = CC.ctc_logits(CC.EDGE_T, 8, 29, seed=24).double()
    lab, ll = pad_labels(rows)
    want = CC.ctc_oracle(x, CC.EDGE_LENS, lab, ll, 28)
    lens2, ll2 = list(CC.EDGE_LENS), ll.clone()
    lens2[7] += 3
    ll2[6] = lab.shape[1] + 5
    got = CC.ctc_oracle(x, lens2, lab, ll2, 28)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    empty = CC.ctc_oracle(x, CC.EDGE_LENS, torch.zeros(8, 0, dtype=torch.int32), ll, 28)
    lp = CC.log_softmax64(x.numpy())
    for b in range(8):
        assert abs(empty[0][b] + lp[: CC.EDGE_LENS[b], b, 28].sum()) <= 1e-12 * empty[0][b]
