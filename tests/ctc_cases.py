"""fp64 CTC oracle and input builders shared by tests/test_ctc.py (CPU) and tests/test_ctc_gpu.py.

The oracle is the textbook alpha/beta recursion over the 2L+1 lattice in float64 log space,
written without F.ctc_loss. It follows the conventions of csrc/ctc.hip: ``len`` is clamped to T
and the label length to the padded label width, an utterance without frames or without a path
is infeasible (loss +inf, gradient 0), and the gradient is softmax - occupancy on the valid
frames and 0 past them."""
import numpy as np
import torch

from align_cases import labels_no_repeat, pad_labels  # noqa: F401  (re-exported to the tests)


def _lse(stack):
    """log-sum-exp over axis 0 that keeps an all--inf column at -inf."""
    m = np.max(stack, axis=0)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return ms + np.log(np.sum(np.exp(stack - ms), axis=0))


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x, axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True))


def ctc_oracle(logits_f64, lens, labels, label_lens, blank):
    """loss [N] (+inf when infeasible) and grad [T, N, K] = d loss_b / d logits, float64 numpy."""
    x = logits_f64.detach().cpu().numpy() if torch.is_tensor(logits_f64) else np.asarray(logits_f64)
    assert x.dtype == np.float64
    T, N, K = x.shape
    lens = np.asarray(lens, dtype=np.int64).reshape(N)
    label_lens = np.asarray(label_lens, dtype=np.int64).reshape(N)
    labels = np.asarray(labels, dtype=np.int64).reshape(N, -1)
    lp = log_softmax64(x)
    loss = np.full(N, np.inf)
    grad = np.zeros((T, N, K))
    for b in range(N):
        n = int(min(lens[b], T))
        L = int(min(label_lens[b], labels.shape[1]))
        if n <= 0 or L > n:
            continue
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)
        ext[1::2] = labels[b, :L]
        skip = np.zeros(S, dtype=bool)                  # the s-2 -> s transition exists
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        e = lp[:n, b][:, ext]                           # [n, S]
        ninf = -np.inf
        alpha = np.full((n, S), ninf)
        alpha[0, :2] = e[0, :2]
        for t in range(1, n):
            a = alpha[t - 1]
            a1, a2 = np.full(S, ninf), np.full(S, ninf)
            a1[1:] = a[:-1]
            a2[2:] = np.where(skip[2:], a[:-2], ninf)
            alpha[t] = _lse(np.stack((a, a1, a2))) + e[t]
        beta = np.full((n, S), ninf)
        beta[n - 1, max(S - 2, 0):] = e[n - 1, max(S - 2, 0):]
        for t in range(n - 2, -1, -1):
            v = beta[t + 1]
            b1, b2 = np.full(S, ninf), np.full(S, ninf)
            b1[:-1] = v[1:]
            b2[:-2] = np.where(skip[2:], v[2:], ninf)           # the s -> s+2 transition exists
            beta[t] = _lse(np.stack((v, b1, b2))) + e[t]
        logp = _lse(alpha[n - 1, max(S - 2, 0):].reshape(-1, 1))[0]
        if logp == ninf:
            continue
        loss[b] = -logp
        with np.errstate(invalid="ignore"):
            gamma = np.where(np.isfinite(e), np.exp(alpha + beta - e - logp), 0.0)
        occ = np.zeros((K, n))
        np.add.at(occ, ext, gamma.T)
        grad[:n, b] = np.exp(lp[:n, b]) - occ.T
    return loss, grad


# --------------------------------------------------------------------------- builders
def ctc_logits(T, N, K, seed, sharp=2.0):
    """Seeded fp32 logits [T, N, K]: a standard normal times ``sharp``."""
    g = torch.Generator().manual_seed(seed)
    return sharp * torch.randn(T, N, K, generator=g)


def classes(K, blank):
    return [c for c in range(K) if c != blank]


def labels_with_repeats(rng, L, K, blank, repeats):
    """L label ids without the blank and with exactly ``repeats`` adjacent equal pairs."""
    assert 0 <= repeats < max(L, 1)
    base = labels_no_repeat(rng, L - repeats, K, blank)
    extra = np.bincount(rng.integers(0, len(base), size=repeats), minlength=len(base)) if repeats else [0] * len(base)
    out = []
    for c, n in zip(base, extra):
        out += [c] * (1 + int(n))
    assert len(out) == L and adjacent_repeats(out) == repeats
    return out


def random_labels(rng, L, K, blank):
    """L label ids drawn freely from the non-blank classes (adjacent repeats as they fall)."""
    cl = classes(K, blank)
    return [cl[int(i)] for i in rng.integers(0, len(cl), size=L)]


def adjacent_repeats(row):
    return sum(1 for a, b in zip(row[:-1], row[1:]) if a == b)


def infeasible(row, n):
    """No frame path of length n collapses to ``row`` (an utterance without frames has none)."""
    return n <= 0 or len(row) + adjacent_repeats(row) > n


# --------------------------------------------------------------------------- case tables
# (b) the mixed edge batch: lens at the 64-frame staging edges, L = 0 twice, L == len without
# repeats (row 2: one path, no blank fits), a single label in two frames (row 1).
EDGE_T = 129
EDGE_LENS = [1, 2, 63, 64, 65, 127, 128, 129]
EDGE_LABEL_LENS = [0, 1, 63, 20, 0, 63, 64, 5]


def edge_rows(seed, K=29, blank=28):
    rng = np.random.default_rng(seed)
    rows = [[], random_labels(rng, 1, K, blank), labels_no_repeat(rng, 63, K, blank), random_labels(rng, 20, K, blank),
            [], random_labels(rng, 63, K, blank), labels_with_repeats(rng, 64, K, blank, 5)]
    c = classes(K, blank)
    rows.append([c[0], c[0], c[1], c[1], c[1]])
    assert [len(r) for r in rows] == EDGE_LABEL_LENS
    return rows


# (c) single-path rows [c]*L in 2L-1 frames, the same rows one frame short (infeasible through
# the repeats alone: L <= len), a row without frames, feasible neighbours in between.
SINGLE_T = 70


def single_path_rows(seed, K=29, blank=28):
    rng = np.random.default_rng(seed)
    c = classes(K, blank)
    rows, lens = [], []
    for i, L in enumerate((1, 4, 33)):
        rows.append([c[(3 * i + 1) % len(c)]] * L); lens.append(2 * L - 1)
    rows.append(random_labels(rng, 12, K, blank)); lens.append(SINGLE_T)
    for i, L in enumerate((4, 33)):
        rows.append([c[(5 * i + 2) % len(c)]] * L); lens.append(2 * L - 2)
    rows.append(random_labels(rng, 3, K, blank)); lens.append(0)
    rows.append(labels_with_repeats(rng, 30, K, blank, 4)); lens.append(66)
    return rows, lens


# (d) one batch that exists for every (K, blank), K = 2 included (one non-blank class):
# T*N = 350 frames, not a multiple of 4.
KB_T = 70
KB_LENS = [70, 64, 65, 33, 1]


def kb_rows(seed, K, blank):
    rng = np.random.default_rng(seed)
    c = classes(K, blank)
    if len(c) == 1:
        rows = [[c[0]] * 20, [c[0]] * 30]
    else:
        rows = [random_labels(rng, 20, K, blank), labels_with_repeats(rng, 30, K, blank, 6)]
    rows += [[], [c[-1]] * 17, [c[0]]]
    return rows


# (a) register-tile widths
def long_rows(Lmax, K=29, blank=28):
    rng = np.random.default_rng(Lmax)
    return [labels_with_repeats(rng, Lmax, K, blank, 20), labels_no_repeat(rng, Lmax - 1, K, blank),
            random_labels(rng, 1, K, blank)]


def long_lens(Lmax):
    T = Lmax + 40
    return [T, T - 3, T]


def expected_spl(Lmax):
    need = (2 * Lmax + 1 + 63) // 64
    return next(k for k in (4, 5, 6, 8, 12, 16, 32) if k >= need)


def all_tables():
    """(name, rows, lens, K, blank) of every table whose rows are feasible or not by design."""
    out = [("edge", edge_rows(0), EDGE_LENS, 29, 28)]
    r, l = single_path_rows(1)
    out.append(("single", r, l, 29, 28))
    for K, blank in KB_CASES:
        out.append(("kb%d_%d" % (K, blank), kb_rows(2, K, blank), KB_LENS, K, blank))
    for Lmax in LONG_LMAX:
        out.append(("long%d" % Lmax, long_rows(Lmax), long_lens(Lmax), 29, 28))
    return out


KB_CASES = [(29, 28), (29, 0), (29, 13), (32, 31), (5, 4), (2, 1)]
LONG_LMAX = [127, 159, 191, 255, 383, 511, 1023]
