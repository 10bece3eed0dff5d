"""SpecAugment test cases: the grid, the oracle glue and the checkers (pure torch / numpy; the
extension is not imported here).

The oracle is deepspeech_amd/ops/reference.py: specaug_plan_ref in exact integer arithmetic,
specaug_apply_ref / specaug_mean_ref on an fp64 copy of the input.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Tuple

import torch

from deepspeech_amd.ops import reference as R

EPS = 2.0 ** -24


@dataclass(frozen=True)
class Case:
    idx: int
    F: int
    T: int
    lens: Tuple[int, ...]
    W: int
    nF: int
    Fw: int
    nT: int
    Tw: int
    p_ppm: int
    seed: int
    step: int
    first_utt: int
    fill: str

    @property
    def B(self):
        return len(self.lens)

    @property
    def policy(self):
        return SimpleNamespace(nF=self.nF, Fw=self.Fw, nT=self.nT, Tw=self.Tw, p_ppm=self.p_ppm, W=self.W,
                               fill=self.fill)

    @property
    def id(self):
        return "c%02d-F%d-T%d-B%d-W%d-nF%dx%d-nT%dx%d-p%d-%s" % (
            self.idx, self.F, self.T, self.B, self.W, self.nF, self.Fw, self.nT, self.Tw, self.p_ppm, self.fill)


def _lens(B: int, T: int, W: int, salt: int) -> Tuple[int, ...]:
    """Ragged lengths: T, 1, 0, a value above T and the values either side of 2W + 4 first (as
    many as fit in B, rotated by salt so that B = 1 and B = 3 see different ones), then a fixed
    scramble over [0, T]."""
    edge = [T, 2 * W + 4, 1, 2 * W + 3, 0, T + 3, 2 * W + 5, max(T - 1, 0)]
    edge = edge[salt % len(edge):] + edge[:salt % len(edge)]
    out = []
    for k in range(B):
        out.append(edge[k] if k < len(edge) else (salt * 7919 + k * 104729) % (T + 1))
    return tuple(out)


def _grid():
    Fs, Bs, Ws = (161, 1, 8, 257), (3, 1, 33), (0, 1, 5, 40)
    nFs, nTs = (1, 2, 0, 8), (2, 1, 0, 16)
    Tws, ps = (100, 1, 0), (1000000, 200000, 0)
    seeds, steps, firsts = (1234, 2 ** 40 + 7), (0, 1, 2 ** 32 + 5), (0, 64)
    cases = []
    for i in range(60):
        W = Ws[i % 4]
        Ts = (1, 2, 3, 2 * W + 3, 2 * W + 4, 2 * W + 5, 67, 130)
        F = Fs[(i // 4 + i) % 4]
        T = Ts[(i * 3 + i // 8) % 8]
        B = Bs[(i + i // 3) % 3]
        Fws = (27, 1, F, 0, F + 5)
        cases.append(Case(idx=i, F=F, T=T, lens=_lens(B, T, W, i), W=W, nF=nFs[(i // 2) % 4], Fw=Fws[i % 5],
                          nT=nTs[(i + i // 4) % 4], Tw=Tws[(i // 5) % 3], p_ppm=ps[(i // 7 + i) % 3],
                          seed=seeds[i % 2], step=steps[(i // 2) % 3], first_utt=firsts[(i // 6) % 2],
                          fill=("mean", "zero")[(i // 3) % 2]))
    return cases


CASES = _grid()
IDS = [c.id for c in CASES]


@functools.lru_cache(maxsize=None)
def oracle_plan(idx: int) -> torch.Tensor:
    c = CASES[idx]
    return R.specaug_plan_ref(torch.tensor(c.lens, dtype=torch.int32), c.T, c.F, c.policy, c.seed, c.step,
                              c.first_utt)


@functools.lru_cache(maxsize=None)
def inputs(idx: int):
    """(x fp32 [B, T, F] with data in the padding too, lens int32 [B]); never modified."""
    c = CASES[idx]
    g = torch.Generator().manual_seed(1000 + idx)
    x = torch.randn(c.B, c.T, c.F, generator=g) * 3.0 + 1.5
    return x, torch.tensor(c.lens, dtype=torch.int32)


def ramp(c: Case) -> torch.Tensor:
    return torch.arange(c.T, dtype=torch.float32)[None, :, None].expand(c.B, c.T, c.F).contiguous()


def time_constant(c: Case) -> torch.Tensor:
    g = torch.Generator().manual_seed(77 + c.idx)
    return torch.randn(c.B, 1, c.F, generator=g).expand(c.B, c.T, c.F).contiguous()


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def check_mean(got: torch.Tensor, x: torch.Tensor, lens: torch.Tensor) -> None:
    """|got - mean64| <= eps S + eps |mean| per element, S = sum |x| over the L terms: a
    sequential fp32 sum of L terms errs by at most (L eps S), the division by L brings that to
    eps S and rounds once more."""
    want = R.specaug_mean_ref(x.double(), lens)
    L = lens.long().clamp(0, x.shape[1])
    valid = torch.arange(x.shape[1])[None, :] < L[:, None]
    S = (x.double().abs() * valid[:, :, None]).sum(1)
    err = (got.double().cpu() - want).abs()
    bound = EPS * S + EPS * want.abs()
    assert bool((err <= bound).all()), "mean: worst excess %g" % float((err - bound).max())
    assert bool((got.cpu()[L == 0] == 0).all())


def check_apply(got: torch.Tensor, x: torch.Tensor, lens: torch.Tensor, plan: torch.Tensor, fill, nF: int) -> dict:
    """``got`` against the fp64 oracle under (plan, fill). Padding, masked cells and cells whose
    source is one frame (r == 0) must hold the oracle's bits; interpolated cells must lie within
    7 eps (|a| + |b|) of a + (r / den)(b - a) in fp64 (4 eps on the quotient, 1 on b - a, 1 on the
    FMA, and the result is bounded by max(|a|, |b|))."""
    got, plan = got.cpu(), plan.cpu()
    fill = None if fill is None else fill.cpu()
    B, T, F = x.shape
    x64 = x.double()
    want = R.specaug_apply_ref(x64, lens, plan, None if fill is None else fill.double(), nF)
    i, r, den, valid = R.specaug_warp_index(lens, plan, T)
    tm, fm = R.specaug_masks(lens, plan, T, F, nF)
    masked = (tm[:, :, None] | fm[:, None, :]) & valid[:, :, None]
    exact = masked | (r == 0)[:, :, None].expand(B, T, F)
    w32 = want.float()
    assert bool((w32.double() == want)[exact & ~torch.isnan(want)].all())          # exact cells are fp32 values
    same = bits(got) == bits(w32)
    assert bool(same[exact].all()), "%d exact cells differ" % int((~same[exact]).sum())
    a = torch.gather(x64, 1, i[:, :, None].expand(B, T, F)).abs()
    b = torch.gather(x64, 1, (i + 1).clamp(max=T - 1)[:, :, None].expand(B, T, F)).abs()
    err = (got.double() - want).abs()
    bound = 7 * EPS * (a + b)
    bad = ~exact & ~(err <= bound)
    assert not bool(bad.any()), "%d interpolated cells out of bound, worst excess %g" % (
        int(bad.sum()), float((err - bound)[bad].max()))
    return dict(exact=int(exact.sum()), interpolated=int((~exact).sum()))


def preconditions() -> dict:
    """Coverage of the grid, from the oracle's own plans: raises if a branch the kernels have is
    not reached by any case."""
    seen = dict.fromkeys(("bin0", "binlast", "zero_width", "overlap", "time_to_end", "w_neg", "w_pos", "w_zero",
                          "forced_identity", "p_cut", "len_above_T", "len_zero", "interpolated"), 0)
    for c in CASES:
        plan = oracle_plan(c.idx).long()
        L = torch.tensor(c.lens).clamp(0, c.T)
        seen["len_above_T"] += int(sum(l > c.T for l in c.lens))
        seen["len_zero"] += int(sum(l == 0 for l in c.lens))
        for b in range(c.B):
            row, Lb = plan[b], int(L[b])
            fmasks = [(int(row[2 + 2 * k]), int(row[3 + 2 * k])) for k in range(c.nF)]
            tmasks = [(int(row[2 + 2 * c.nF + 2 * k]), int(row[3 + 2 * c.nF + 2 * k])) for k in range(c.nT)]
            for f0, fw in fmasks:
                assert 0 <= f0 and f0 + fw <= c.F and 0 <= fw <= min(c.Fw, c.F)
                seen["bin0"] += fw > 0 and f0 == 0
                seen["binlast"] += fw > 0 and f0 + fw == c.F
                seen["zero_width"] += fw == 0
            cap = min(c.Tw, Lb * c.p_ppm // 1000000)
            seen["p_cut"] += bool(tmasks) and cap < min(c.Tw, Lb)
            for t0, tw in tmasks:
                assert 0 <= t0 and t0 + tw <= Lb and 0 <= tw <= cap
                seen["time_to_end"] += tw > 0 and t0 + tw == Lb
                seen["zero_width"] += tw == 0
            for spans in (fmasks, tmasks):
                live = [(s, s + n) for s, n in spans if n > 0]
                seen["overlap"] += any(a0 < b1 and b0 < a1 for k, (a0, a1) in enumerate(live)
                                       for (b0, b1) in live[k + 1:])
            w0, w = int(row[0]), int(row[1])
            if c.W > 0 and Lb - 2 * c.W - 2 < 1:
                assert w0 == 0 and w == 0
                seen["forced_identity"] += 1
            elif c.W > 0:
                assert c.W + 1 <= w0 <= Lb - c.W - 2 and -c.W <= w <= c.W and 1 <= w0 + w <= Lb - 2
                seen["w_neg"] += w < 0
                seen["w_pos"] += w > 0
                seen["w_zero"] += w == 0
        _, r, _, _ = R.specaug_warp_index(torch.tensor(c.lens), oracle_plan(c.idx), c.T)
        seen["interpolated"] += int((r != 0).sum())
    missing = [k for k, v in seen.items() if not v]
    assert not missing, "the grid reaches no %s" % ", ".join(missing)
    return seen
