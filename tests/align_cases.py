"""Input builders shared by tests/test_align.py (CPU) and tests/test_align_gpu.py."""
import numpy as np
import torch


def random_lp(T, N, K, seed, sharp=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(sharp * torch.randn(T, N, K, generator=g), -1)


def quantised_lp(T, N, K, seed):
    """'Log-probs' that are multiples of 0.25 in [-4, 0]: sums of them are exact in fp32, so
    equal-scoring paths tie exactly and only the tie rule decides between them."""
    g = torch.Generator().manual_seed(seed)
    return -0.25 * torch.randint(0, 17, (T, N, K), generator=g).float()


def labels_no_repeat(rng, L, K, blank):
    """L label ids in [0, K) without the blank and without adjacent repeats."""
    out = []
    while len(out) < L:
        c = int(rng.integers(0, K))
        if c != blank and (not out or out[-1] != c):
            out.append(c)
    return out


def pad_labels(rows, width=0):
    L = max(1, width, max(len(r) for r in rows))
    lab = np.zeros((len(rows), L), np.int32)
    for i, r in enumerate(rows):
        lab[i, :len(r)] = r
    return torch.from_numpy(lab), torch.tensor([len(r) for r in rows], dtype=torch.int32)


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def path_score(lp_tk, path):
    """fp32 sum of lp along a frame path, in frame order (the Viterbi recursion's order)."""
    acc = np.float32(0.0)
    for t, c in enumerate(path):
        acc = np.float32(acc + np.float32(lp_tk[t, c])) if t else np.float32(lp_tk[0, c])
    return acc
