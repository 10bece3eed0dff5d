"""Oracles, checkers, guard-banded buffers, case tables and case drivers of the small streaming
kernels that run around every training step: csrc/optim.hip (Adam + EMA in its three launch forms,
grad_norm, cast_bf16), csrc/quant.hip (fp8_quant2), csrc/reduce.hip (col_sum, fc_bias_grad) and
csrc/fill.hip (multi_fill, multi_copy, prep_inputs, transpose_bf16). Pure torch, device-agnostic,
does not import the extension. The idioms and constants are those of tests/conv_cases.py and
tests/gemm_cases.py.

Drivers. Every run_*(impl, dev, ...) builds the buffers of one case on `dev`, calls the kernel
through `impl`, an object with the extension's functions (the extension itself on the GPU, the
step-by-step fp32 emulation of tests/test_stream_oracle.py on the CPU) and checks everything the
launch may and may not have written. A planted error is an emulation with one step changed.

Buffers (Band, gemm_cases.Plane). Every output and every in-place array is a slice of a larger
buffer prefilled with the sentinel NaN pattern: the payload starts 16-B aligned (multi_fill also
takes bases that are only 4-B aligned), 64 guard elements lie directly before it and directly after
its last element, whatever n % 4 is. After a launch the guards are bit-identical and read-only
inputs are unchanged.

Adam + EMA. Oracle: TF Adam (epsilon-hat) in fp64 from the stored fp32 arrays and the fp32-rounded
hyper-parameters the kernel receives (1 - b1 and 1 - b2 are exact in fp32 for b in [0.5, 1]):
    gj = g gscale    m' = b1 m + (1 - b1) gj    v' = b2 v + (1 - b2) gj^2
    p' = p - lr_t m' / (sqrt(v') + eps)         ema' = p' + keep (ema - p')
adam1 / ema1 (csrc/common.h) spell out every rounding, each correctly rounded (relative error
u = 2^-24 = EPS; TINY = 2^-149, one subnormal step, is added to every bound). Counting them:
    m: 3 roundings (gj, its product, the fma): dm <= 3 u Sm, Sm = |b1 m| + (1 - b1) |gj|; bound 4 u Sm
    v: 4 roundings (gj enters twice: 2 u; two products; the fma): dv <= 5 u v'; bound 6 u v'
       (the extra u in both covers the second-order terms)
    sqrt: |sqrt(v' +- dv) - sqrt(v')| evaluated exactly (it is not Lipschitz at 0), + u for its
       rounding: ds;   the sum with eps: dden = ds + u (sqrt(v' + dv) + eps)
    the division q = m' / den: dq = (dm + |q| dden) / (den - dden), + u (|q| + dq) for its rounding
    p: dp = lr_t dq + u (|p| + lr_t (|q| + dq))   (the fma's rounding)
    ema, from the p the kernel stored: 2 roundings, de = 3 u (keep |ema - p| + |p|)
p16 must equal RNE-bf16 of the stored p bitwise. A NaN g makes p, m, v (and ema, p16) NaN at its
element only. Derived, not measured; the CPU emulation (torch fp32 op by op, fma through fp64) must
lie inside the bound for every table entry.

grad_norm. Sum of the partials (in fp64) against the fp64 sum S of (fp32(g gscale))^2. A lane's
chain has L = ceil(n / (256 blocks)) terms (one product and one add each), then 6 wave-reduction
levels and 4 adds across the waves: bound (L + 12) u S.

fp8_quant2. Bitwise the fp32 steps amax -> s = max(amax / 448, 1e-12) -> inv = 1 / s ->
e4m3(clamp(x inv)), scales = {s_a, s_b alpha}; and independently in fp64: with y = x / s,
|q s - x| <= s (h(|y| (1 + 3 u)) + 3 u |y|), h half an e4m3 step (2^(max(e, -6) - 4) at 2^e <= y <
2^(e+1)), 3 u for the roundings of inv and of the product. A NaN element comes out as an e4m3 NaN
byte; everything else is as if it were zero.

col_sum, fc_bias_grad: fixed summation order, so the fp32 emulation is bitwise (fc_bias_grad's
accumulate form may contract out + t alpha into one fma: either rounding of that last step is
accepted per element), plus an fp64 check with (terms + 2) u S_abs.
"""
import functools
import math

import torch

from conv_cases import EPS, SENT16, SENT32, Mismatch, _coords, hulp, rne_bf16  # noqa: F401
from gemm_cases import SENT8, Plane, cdiv

F64, F32, BFT, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn
I32, I16, U8 = torch.int32, torch.int16, torch.uint8
TINY = 2.0 ** -149
GUARD = 64
WORST = {}                      # kernel -> worst err/tol seen (profiles/stream_oracle_coverage.md)
COUNTS = {}                     # kernel -> launches checked
_ITY = {F32: (I32, SENT32), I32: (I32, SENT32), BFT: (I16, SENT16), F8: (U8, SENT8), U8: (U8, SENT8)}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def f32r(x):
    """x rounded to fp32, as a Python float (what a kernel receives for a scalar argument)"""
    return float(torch.tensor(x, dtype=F32))


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _count(kernel, n=1):
    COUNTS[kernel] = COUNTS.get(kernel, 0) + n


# ------------------------------------------------------------------------------ guard bands
class Band:
    """A 1-D payload `t` of n elements inside a buffer prefilled with the sentinel: GUARD elements
    before it (+ `shift` bytes, for a base that is only 4-B aligned) and GUARD after its last."""

    def __init__(self, n, dtype, device, shift=0):
        self.ity, self.sent = _ITY[dtype]
        es = torch.empty(0, dtype=dtype).element_size()
        assert shift % es == 0 and (GUARD * es) % 16 == 0
        self.n, self.lo = int(n), GUARD + shift // es
        self.buf = torch.empty(self.lo + self.n + GUARD, dtype=dtype, device=device)
        self.buf.view(self.ity).fill_(self.sent)
        self.t = self.buf[self.lo:self.lo + self.n]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == shift % 16

    def put(self, x):
        if self.n:
            self.t.copy_(x.reshape(-1))
        return self

    def bits(self):
        return self.buf.view(self.ity).cpu().clone()

    def payload(self):
        return self.bits()[self.lo:self.lo + self.n]

    def values(self):
        return self.t.detach().cpu().clone()

    def verify(self, name):
        """the guards on both sides are bit-identical to the sentinel"""
        iv = self.bits()
        for side, part, base in (("before", iv[:self.lo], -self.lo), ("after", iv[self.lo + self.n:], self.n)):
            bad = part != self.sent
            if bool(bad.any()):
                i = int(bad.to(U8).argmax())
                raise Mismatch("%s: %d guard elements %s the payload were written; first at i=%d (payload of %d)" % (
                    name, int(bad.sum()), side, base + i, self.n), dict(i=base + i))

    def same(self, name, snap, mask=None):
        """the payload (where mask) is bit-identical to the snapshot"""
        bad = self.payload() != snap
        if mask is not None:
            bad &= mask
        if bool(bad.any()):
            i = int(bad.to(U8).argmax())
            raise Mismatch("%s: %d elements changed that must be bit-unchanged; first at i=%d: 0x%x -> 0x%x" % (
                name, int(bad.sum()), i, int(snap[i]) & 0xFFFFFFFF, int(self.payload()[i]) & 0xFFFFFFFF), dict(i=i))

    def written(self, name, mask=None):
        left = self.payload() == self.sent
        if mask is not None:
            left &= mask
        if bool(left.any()):
            i = int(left.to(U8).argmax())
            raise Mismatch("%s: %d of %d elements were never written; first at i=%d" % (name, int(left.sum()), self.n, i),
                           dict(i=i))


# ------------------------------------------------------------------------------ checkers
def check_vals(name, got, want, tol, kernel=None, mask=None):
    """Per element |got - want| <= tol; a NaN want demands a NaN got; any other non-finite got
    fails. Names the worst element."""
    got = got.detach().cpu().to(F64).reshape(want.shape)
    mask = torch.ones_like(want, dtype=torch.bool) if mask is None else mask
    nan = torch.isnan(want)
    lost = nan & ~torch.isnan(got) & mask
    if bool(lost.any()):
        i = int(lost.reshape(-1).to(U8).argmax())
        raise Mismatch("%s: element %d must be NaN, got %r" % (name, i, got.reshape(-1)[i].item()), dict(i=i))
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    err = torch.where(nan | ~mask, torch.zeros_like(err), err)
    ratio = torch.where(err > 0, err / torch.nan_to_num(tol, nan=0.0).clamp_min(1e-300), torch.zeros_like(err))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if kernel is not None and math.isfinite(worst):
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        raise Mismatch("%s: %d of %d elements beyond tolerance; worst at i=%d: got %r want %r err %.3e tol %.3e" % (
            name, int((ratio > 1).sum()), ratio.numel(), i, got.reshape(-1)[i].item(), want.reshape(-1)[i].item(),
            err.reshape(-1)[i].item(), tol.reshape(-1)[i].item()), dict(i=i))
    return worst


def check_bits(name, got, want, dims=("i",), either=None):
    """integer views equal element by element (either: a second accepted value per element)"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    bad = got != want
    if either is not None:
        bad &= got != either.cpu()
    if bool(bad.any()):
        i = int(bad.reshape(-1).to(U8).argmax())
        c = _coords(i, want.shape, dims)
        raise Mismatch("%s: %d of %d elements differ bitwise; first at %s: got 0x%x want 0x%x" % (
            name, int(bad.sum()), bad.numel(), ", ".join("%s=%d" % kv for kv in c.items()),
            int(got.reshape(-1)[i]) & 0xFFFFFFFF, int(want.reshape(-1)[i]) & 0xFFFFFFFF), c)


def bf16_rne_bits(x):
    """fp32 -> bf16 bits by integer arithmetic (RNE; NaN -> the quiet NaN 0x7FC0 | sign): the
    reference of the casts, independent of torch's own conversion"""
    b = x.detach().cpu().contiguous().view(I32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    nan = torch.isnan(x.detach().cpu())
    r = torch.where(nan, ((b >> 16) & 0x8000) | 0x7FC0, r) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(I16)


def check_bf16(name, got16, x32, mask=None):
    """got16 (bf16) is RNE of x32 bitwise (where mask); where x32 is NaN any NaN is accepted"""
    want = bf16_rne_bits(x32)
    gb = got16.detach().cpu().contiguous().view(I16)
    nan = torch.isnan(x32.detach().cpu())
    ok = nan & torch.isnan(got16.detach().cpu().float())
    if mask is not None:
        ok |= ~mask
    check_bits(name, torch.where(ok, want, gb), want)


# ------------------------------------------------------------------------------ optim.hip: Adam + EMA
HYP = {k: f32r(v) for k, v in dict(lr_t=1e-3, b1=0.9, b2=0.999, eps=1e-8, keep=0.99).items()}
GSCALES = (1.0, 0.5, f32r(1.0 / 3.0))
STRIDE = 3 * 256                   # float4 groups per sweep of a max_grid = 3 launch
ADAM_GS_N4 = (700, STRIDE + 1, 2 * STRIDE, 2 * STRIDE + 5, 5 * STRIDE + 17)
ADAM_GS_N = tuple(4 * n4 + t for n4 in ADAM_GS_N4 for t in range(4)) + (1, 3, 4, 5)
# block-contiguous: (n, max_grid); chunk4() gives 234 (< 256, 3 blocks, ragged), 301 (between 256
# and 512, ragged), 221, the whole array in one block, and one block per 256 groups
ADAM_CHUNK = ((4 * 700 + 3, -7), (4 * 2101 + 1, -7), (4 * (2 * STRIDE + 5) + 2, -7), (4 * 700 + 3, -1),
              (4 * (5 * STRIDE + 17) + 3, -1), (4 * 2101 + 1, -2048), (4 * (5 * STRIDE + 17) + 3, -2048), (5, -7), (3, -2048))
ADAM_LDS_N = (4 * (STRIDE + 1) + 3, 5)
ADAM_OPT_N = 4 * (2 * STRIDE + 5) + 3
# options, each run grid-strided (max_grid 3) and block-contiguous (-7)
ADAM_OPTIONS = (dict(ema=False), dict(p16=False), dict(ema=False, p16=False), dict(gscale=GSCALES[1]),
                dict(gscale=GSCALES[2]), dict(skip=0), dict(skip=1), dict(hyper=True),
                dict(hyper=True, skip=0, gscale=GSCALES[1]), dict(hyper=True, skip=1, ema=False))
ARENA = 4800


def chunk4(n, max_grid):
    """(grid, float4 groups per block) of the block-contiguous launch (csrc/optim.hip ds2_adam_ema)"""
    n4 = n // 4
    grid = max(1, min(-max_grid, cdiv(n4, 256)))
    return grid, cdiv(n4, grid)


def _ranges64():
    r = [(0, 16), (ARENA - 12, ARENA), (100, 200), (200, 260), (300, 300), (0, 0), (ARENA, ARENA), (1000, 4000)]
    i = 0
    while len(r) < 64:
        lo = 400 + 8 * i
        r.append((lo, lo + (8, 4, 0)[i % 3]))     # 8 long and touching the next, 4 long, empty
        i += 1
    g = _g(64)
    return [r[i] for i in torch.randperm(64, generator=g).tolist()]


ADAM_RANGES = {"none": [], "one": [(8, 4000)], "whole": [(0, ARENA)], "sixty-four": _ranges64()}


@functools.lru_cache(maxsize=None)
def adam_inputs(n):
    """fp32 p, g, m, v (>= 0), ema of one size, with the edge elements mixed in (n >= 16). Cached
    and shared: never modified."""
    g_ = _g(7919 * n + 13)
    p = torch.randn(n, generator=g_, dtype=F64)
    g = torch.randn(n, generator=g_, dtype=F64)
    m = 0.1 * torch.randn(n, generator=g_, dtype=F64)
    v = 0.01 * torch.rand(n, generator=g_, dtype=F64)
    e = p + 0.01 * torch.randn(n, generator=g_, dtype=F64)
    d = dict(zero=[], nan=[], v0=[], big=[])
    if n >= 16:
        d.update(zero=[1, n - 1], nan=[4, n - 2], v0=[3, n - 3], big=[6])
        for i in d["zero"]:
            g[i] = m[i] = v[i] = 0.0
            e[i] = p[i]
        for i in d["v0"]:
            v[i], m[i] = 0.0, 0.05
        g[n - 3] = 0.0                               # v' = 0: the quotient is m' / eps
        g[6] = 1e18
        for i in d["nan"]:
            g[i] = float("nan")
    d.update(p=p.to(F32), g=g.to(F32), m=m.to(F32), v=v.to(F32), e=e.to(F32))
    return d


def adam_oracle(inp, gscale, hyp=HYP):
    """fp64 p', m', v' and their bounds (module docstring)"""
    p, g, m, v = (inp[k].to(F64) for k in "pgmv")
    lr, b1, b2, eps, u = hyp["lr_t"], hyp["b1"], hyp["b2"], hyp["eps"], EPS
    gj = g * gscale
    Sm = (b1 * m).abs() + (1 - b1) * gj.abs()
    m1, dm = b1 * m + (1 - b1) * gj, 4 * u * Sm + TINY
    v1 = b2 * v + (1 - b2) * gj * gj
    dv = 6 * u * v1 + TINY
    s, s_hi, s_lo = v1.sqrt(), (v1 + dv).sqrt(), (v1 - dv).clamp_min(0).sqrt()
    ds = torch.maximum(s_hi - s, s - s_lo) + u * s_hi
    den, dden = s + eps, ds + u * (s_hi + eps)
    q = m1 / den
    dq = (dm + q.abs() * dden) / (den - dden)
    dq = dq + u * (q.abs() + dq)
    p1 = p - lr * q
    dp = lr * dq + u * (p.abs() + lr * (q.abs() + dq)) + TINY
    return dict(p=p1, m=m1, v=v1), dict(p=dp, m=dm, v=dv)


def ema_oracle(e0, p_stored, keep=HYP["keep"]):
    e0, ps = e0.to(F64), p_stored.to(F64)
    return ps + keep * (e0 - ps), 3 * EPS * (keep * (e0 - ps).abs() + ps.abs()) + TINY


def adam_name(c, ranges=None):
    s = "adam n=%d" % c["n"]
    s += " ranges=%s" % ranges if ranges is not None else " max_grid=%d" % c.get("max_grid", 0)
    for k in ("lds", "gscale", "skip"):
        if c.get(k) not in (None, 0, 1.0) or (k == "skip" and c.get(k) is not None):
            s += " %s=%g" % (k, c[k])
    for k in ("ema", "p16"):
        s += "" if c.get(k, True) else " no-" + k
    return s + (" hyper" if c.get("hyper") else "")


def run_adam(impl, dev, c, ranges=None):
    """One launch of adam_ema (or, with the name of an ADAM_RANGES entry, adam_ema_ranges) on
    guard-banded arrays; returns the payload bits of every array, for the bitwise comparison of
    the launch forms."""
    n, gscale, skip = c["n"], c.get("gscale", 1.0), c.get("skip")
    use_e, use_16 = c.get("ema", True), c.get("p16", True)
    name = adam_name(c, ranges)
    inp = adam_inputs(n)
    B = {k: Band(n, F32, dev).put(inp[k]) for k in ("pgmve" if use_e else "pgmv")}
    if use_16:
        B["h"] = Band(n, BFT, dev)
    snap = {k: b.payload() for k, b in B.items()}
    lr, keep, hyper = HYP["lr_t"], HYP["keep"], None
    if c.get("hyper"):
        hyper = torch.tensor([lr, keep], dtype=F32, device=dev)
        lr = keep = float("nan")
    args = (B["p"].t, B["g"].t, B["m"].t, B["v"].t, B["e"].t if use_e else None, B["h"].t if use_16 else None)
    hy = (HYP["b1"], HYP["b2"], HYP["eps"], gscale, keep)
    mask = torch.ones(n, dtype=torch.bool)
    if ranges is None:
        skip_t = None if skip is None else torch.tensor([skip], dtype=I32, device=dev)
        impl.adam_ema(*args, lr, *hy, skip_t, c.get("max_grid", 0), hyper, c.get("lds", 0))
        kernel = "adam_ema chunk" if c.get("max_grid", 0) < 0 else "adam_ema"
    else:
        mask[:] = False
        for lo, hi in ADAM_RANGES[ranges]:
            mask[lo:hi] = True
        impl.adam_ema_ranges(*args, [x for r in ADAM_RANGES[ranges] for x in r], lr, *hy, hyper)
        kernel = "adam_ema_ranges"
    _sync(dev)
    _count(kernel)
    for k, b in B.items():
        b.verify("%s: %s" % (name, k))
    B["g"].same(name + ": g (read-only)", snap["g"])
    if skip == 1:
        for k, b in B.items():
            b.same("%s: %s under skip = 1" % (name, k), snap[k])
        return {k: b.payload() for k, b in B.items()}
    for k, b in B.items():                            # outside the ranges nothing moves
        b.same("%s: %s outside the ranges" % (name, k), snap[k], ~mask)
    want, tol = adam_oracle(inp, gscale)
    got = {k: B[k].values() for k in B}
    for k in "mvp":
        check_vals("%s: %s" % (name, k), got[k], want[k], tol[k], "%s %s" % (kernel, k), mask)
    if use_e:
        we, te = ema_oracle(inp["e"], got["p"])
        check_vals(name + ": ema", got["e"], we, te, kernel + " ema", mask)
    if use_16:
        B["h"].written(name + ": p16", mask)
        check_bf16(name + ": p16 against RNE of the stored p", got["h"], got["p"], mask)
    zero = torch.zeros(n, dtype=torch.bool)
    zero[inp["zero"]] = True
    for k in ("p", "e") if use_e else ("p",):         # g = m = v = 0: p and ema keep their bits
        B[k].same("%s: %s at a g = m = v = 0 element" % (name, k), snap[k], zero)
    for k in "pmv":                                  # a NaN g poisons its own element only
        gk = got[k]
        extra = torch.isnan(gk) & ~torch.isnan(inp["g"])
        assert not bool(extra.any()), "%s: %s is NaN at element %d, whose g is finite" % (name, k, int(extra.to(U8).argmax()))
    return {k: b.payload() for k, b in B.items()}


def same_forms(name, a, b):
    for k in a:
        check_bits("%s: %s differs between launch forms" % (name, k), b[k], a[k])


# ------------------------------------------------------------------------------ optim.hip: grad_norm, cast_bf16
GN_N = (1, 255, 256, 257, 1000, 70001)
GN_PARTS = (None, 1, 3)             # None: grad_norm_blocks(n)
# (value, gscale): every one must raise the flag, at the first, a middle and the last element
GN_POISON = ((float("nan"), 1.0), (float("inf"), 0.5), (float("-inf"), 1.0), (3e38, 2.0), (float("inf"), 0.0))


def gn_blocks(n):
    return max(1, min(16384, cdiv(n // 4, 256)))


def run_grad_norm(impl, dev, n, nparts, gscale, poison=None, where=0, flag0=0):
    name = "grad_norm n=%d parts=%s gscale=%g%s flag0=%d" % (n, nparts, gscale, "" if poison is None else " %r at %d" % (poison, where), flag0)
    nb = int(impl.grad_norm_blocks(n)) if nparts is None else nparts
    assert nparts is not None or nb == gn_blocks(n), (name, nb)
    g = torch.randn(n, generator=_g(n), dtype=F32)
    if poison is not None:
        g[where] = poison
    G, part = Band(n, F32, dev).put(g), Band(nb, F32, dev)
    bad = Band(1, I32, dev).put(torch.tensor([flag0], dtype=I32))
    snap = G.payload()
    impl.grad_norm(G.t, gscale, part.t, bad.t)
    _sync(dev)
    _count("grad_norm")
    for b_, k in ((G, "g"), (part, "part"), (bad, "bad")):
        b_.verify("%s: %s" % (name, k))
    G.same(name + ": g (read-only)", snap)
    part.written(name + ": part")
    flag = int(bad.values()[0])
    if poison is not None:
        assert flag == 1, "%s: the non-finite flag is %d, want 1" % (name, flag)
        return
    assert flag == flag0, "%s: the non-finite flag is %d, want %d" % (name, flag, flag0)
    x = (g * torch.tensor(gscale, dtype=F32)).to(F64)
    S = (x * x).sum().reshape(1)
    L = cdiv(n, 256 * nb)
    check_vals(name, part.values().to(F64).sum().reshape(1), S, (L + 12) * EPS * S, "grad_norm")


CAST_SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38,
                 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 2.0 ** -7 + 2.0 ** -8),
                 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 1e-40, 3.3895313892515355e38)
CAST_N = (1, 255, 1025)


def cast_input(n, first=0):
    sp = torch.tensor(CAST_SPECIALS, dtype=F32)
    x = torch.cat([sp.roll(-first), torch.randn(max(0, n - len(sp)), generator=_g(n), dtype=F32)])[:n]
    if n > len(sp):
        x[n - 1] = sp[8]                             # a tie that rounds up, on the last element
    return x


def run_cast(impl, dev, n, first=0):
    name = "cast_bf16 n=%d first=%d" % (n, first)
    x = cast_input(n, first)
    X, Y = Band(n, F32, dev).put(x), Band(n, BFT, dev)
    snap = X.payload()
    impl.cast_bf16(X.t, Y.t)
    _sync(dev)
    _count("cast_bf16")
    X.verify(name + ": x")
    Y.verify(name + ": y")
    X.same(name + ": x (read-only)", snap)
    check_bf16(name, Y.values(), x)


# ------------------------------------------------------------------------------ quant.hip
Q_SHAPES = ((1, 1, 8, 8), (3, 5, 8, 128), (5, 300, 136, 136), (5, 300, 136, 256), (257, 2, 24, 128))
Q_VARIANTS = ("random", "amax first +", "amax first -", "amax last +", "amax last -", "zero a", "zero b", "sum")
Q_NONFINITE = ("nan a", "nan b", "nan both", "inf a", "-inf b", "sum inf-inf", "sum nan")
Q_ALPHA = f32r(0.3)


def q_blocks(na, nb_el):
    return max(1, min(1024, cdiv(max(na, nb_el) // 8, 256)))


@functools.lru_cache(maxsize=None)
def quant_operands(sh, variant):
    """bf16 a [rows_a, K], b [rows_b, K] (and a2, or None) of one case"""
    ra, rb, K, Kp = sh
    g_ = _g(ra * 1009 + rb * 31 + K + Kp)
    a = (3.0 * torch.randn(ra, K, generator=g_)).to(BFT)
    b = (0.02 * torch.randn(rb, K, generator=g_)).to(BFT)
    a2 = None
    if variant.startswith("amax"):
        _, pos, sign = variant.split()
        for x, big in ((a, 40.0), (b, 2.5)):
            idx = (0, 0) if pos == "first" else (x.shape[0] - 1, K - 1)
            x[idx] = big if sign == "+" else -big
    elif variant == "zero a":
        a.zero_()
    elif variant == "zero b":
        b.zero_()
    elif variant.startswith("sum"):
        a2 = (2.0 * torch.randn(ra, K, generator=g_)).to(BFT)
    mid_a, mid_b = (ra // 2, K // 2), (rb - 1, K - 1)
    if variant in ("nan a", "nan both"):
        a[mid_a] = float("nan")
    if variant in ("nan b", "nan both"):
        b[mid_b] = float("nan")
        b[0, 0] = float("nan")
    if variant == "inf a":
        a[mid_a] = float("inf")
    if variant == "-inf b":
        b[mid_b] = float("-inf")
    if variant == "sum inf-inf":
        a[mid_a], a2[mid_a] = float("inf"), float("-inf")
    if variant == "sum nan":
        a2[0, 0] = float("nan")
    return a, b, a2


def quant_ref(x, Kp):
    """The fp32 steps of the quantiser on one stored operand: (s as an fp32 0-d tensor, bytes
    [rows, Kp] uint8 with e4m3 NaN 0x7F where x is NaN)"""
    xf = x.to(F32)
    nan = torch.isnan(xf)
    amax = torch.where(nan, torch.zeros_like(xf), xf.abs()).max() if xf.numel() else torch.zeros((), dtype=F32)
    s = torch.maximum(amax / 448.0, torch.tensor(1e-12, dtype=F32))
    inv = 1.0 / s
    y = (xf * inv).clamp(-448.0, 448.0)
    q = torch.where(torch.isnan(y), torch.zeros_like(y), y).to(F8).view(U8)
    q = torch.where(torch.isnan(y), torch.full_like(q, SENT8), q)
    out = torch.zeros(x.shape[0], Kp, dtype=U8)
    out[:, :x.shape[1]] = q
    return s, out


def e4m3_half_step(y):
    _, e = torch.frexp(y)
    return torch.where(y > 0, torch.ldexp(torch.ones_like(y), (e - 1).clamp_min(-6) - 4), torch.zeros_like(y))


def _check_quant_operand(name, x, s, got8, Kp, finite_scale):
    """got8 [rows, Kp] uint8 of operand x (bf16, CPU) against quant_ref and the fp64 bound"""
    rows, K = x.shape
    xf = x.to(F32)
    nan = torch.isnan(xf)
    gk = got8[:, :K]
    lost = nan & ((gk & 0x7F) != 0x7F)
    if bool(lost.any()):
        i = int(lost.reshape(-1).to(U8).argmax())
        r, c = i // K, i % K
        byte = int(gk[r, c])
        val = float(gk[r, c].reshape(1).view(F8).float())
        raise Mismatch("%s: the NaN at [%d, %d] was stored as byte 0x%02X (%g, dequantised %g), want an e4m3 NaN" % (
            name, r, c, byte, val, val * float(s)), dict(m=r, n=c))
    pad = got8[:, K:]
    if bool((pad != 0).any()):
        i = int((pad != 0).reshape(-1).to(U8).argmax())
        raise Mismatch("%s: padding column [%d, %d] holds 0x%02X, want zero" % (
            name, i // (Kp - K), K + i % (Kp - K), int(pad.reshape(-1)[i])), dict(m=i // (Kp - K), n=K + i % (Kp - K)))
    deq = gk.contiguous().view(F8).to(F64) * float(s)
    inf = torch.isinf(xf)
    if bool(inf.any()):                                # an infinite element: only that it does not come out finite
        fin = inf & torch.isfinite(deq)
        assert not bool(fin.any()), "%s: an infinite element dequantises to a finite value" % name
        return 0.0
    assert finite_scale
    s_ref, want8 = quant_ref(x, Kp)
    want8 = torch.where((want8 == SENT8) & ((got8 & 0x7F) == 0x7F), got8, want8)      # either NaN byte
    check_bits(name + ": e4m3 bytes", got8, want8, ("m", "n"))
    y = torch.where(nan, torch.zeros_like(xf), xf).to(F64) / float(s)
    tol = float(s) * (e4m3_half_step(y.abs() * (1 + 3 * EPS)) + 3 * EPS * y.abs())
    return check_vals(name + ": q s against x", torch.where(nan, torch.zeros_like(deq), deq),
                      torch.where(nan, torch.zeros_like(y), xf.to(F64)), tol, "fp8_quant2")


def run_quant(impl, dev, sh, variant, alpha=Q_ALPHA, ops=None):
    """One fp8_quant2 launch on the operands of `variant` (or on ops = (a, b, a2)); returns
    (a8 bits, b8 bits, scales bits, asum bits or None)"""
    ra, rb, K, Kp = sh
    name = "fp8_quant2 %dx%d, %dx%d -> Kp %d, %s" % (ra, K, rb, K, Kp, variant)
    a, b, a2 = ops or quant_operands(sh, variant)
    nb = int(impl.fp8_quant_blocks(ra * Kp, rb * Kp))
    assert nb == q_blocks(ra * Kp, rb * Kp), (name, nb)
    A, Bm = Band(ra * K, BFT, dev).put(a), Band(rb * K, BFT, dev).put(b)
    A2 = None if a2 is None else Band(ra * K, BFT, dev).put(a2)
    AS = None if a2 is None else Band(ra * K, BFT, dev)
    a8, b8 = Band(ra * Kp, F8, dev), Band(rb * Kp, F8, dev)
    part, scales = Band(2 * nb, F32, dev), Band(2, F32, dev)
    ro = [(k, x, x.payload()) for k, x in (("a", A), ("b", Bm), ("a2", A2)) if x is not None]
    impl.fp8_quant2(A.t.view(ra, K), Bm.t.view(rb, K), alpha, a8.t.view(ra, Kp), b8.t.view(rb, Kp), part.t, scales.t,
                    None if A2 is None else A2.t.view(ra, K), None if AS is None else AS.t.view(ra, K))
    _sync(dev)
    _count("fp8_quant2")
    for k, x in (("a", A), ("b", Bm), ("a2", A2), ("asum", AS), ("a8", a8), ("b8", b8), ("part", part), ("scales", scales)):
        if x is not None:
            x.verify("%s: %s" % (name, k))
    for k, x, s0 in ro:
        x.same("%s: %s (read-only)" % (name, k), s0)
    xa = a
    if a2 is not None:
        xa = torch.add(a, a2)
        nan = torch.isnan(xa.float())
        gs = AS.values().view(ra, K)
        check_bits(name + ": asum against torch.add", torch.where(nan & torch.isnan(gs.float()), xa, gs).view(I16),
                   xa.view(I16))
    sc = scales.values()
    sa, sb = quant_ref(xa, Kp)[0], quant_ref(b, Kp)[0]
    check_bits(name + ": scales {s_a, s_b alpha}", sc.view(I32), torch.stack([sa, sb * torch.tensor(alpha, dtype=F32)]).view(I32))
    w = 0.0
    for k, x, s, q in (("a", xa, sa, a8), ("b", b, sb, b8)):
        if bool(torch.isfinite(x.float()).all()):      # 0x7F is the sentinel and the NaN byte
            q.written("%s: %s8" % (name, k))
        w = max(w, _check_quant_operand("%s: %s" % (name, k), x, s, q.payload().view(x.shape[0], Kp), Kp, bool(torch.isfinite(s))))
    if "zero a" == variant:
        assert float(sa) == f32r(1e-12) and not bool(a8.payload().any()), name + ": an all-zero operand: scale floor, zero bytes"
    return a8.payload(), b8.payload(), scales.payload(), None if AS is None else AS.payload()


# ------------------------------------------------------------------------------ reduce.hip
WRAP = (1, 2, 262144 + 513)        # R * C past 1024 blocks of 256: the grid wraps
CS_SHAPES = ((1, 1, 1), (2, 4, 7), (3, 16, 300))
# jobs of one launch: (R, B, C, acc)
CS_CASES = ([(1, 1, 1, 0)], [(1, 1, 1, 1)], [(2, 4, 7, 1), (3, 16, 300, 0)], [(1, 1, 1, 0), (3, 16, 300, 1), (2, 4, 7, 0)],
            [(2, 4, 7, 0), (1, 1, 1, 1), (3, 16, 300, 0), (2, 4, 7, 1)], [(1, 1, 1, 1), WRAP + (0,), (2, 4, 7, 1)],
            [WRAP + (1,)])


def run_col_sum(impl, dev, jobs):
    name = "col_sum " + " ".join("%dx%dx%d%s" % (R, B, C, "+" if acc else "") for R, B, C, acc in jobs)
    ins, outs, snaps, x0, o0 = [], [], [], [], []
    for j, (R, B, C, acc) in enumerate(jobs):
        g_ = _g(R * 7 + B * 13 + C + j)
        x = torch.randn(R, B, C, generator=g_, dtype=F32)
        o = torch.randn(R * C, generator=g_, dtype=F32)
        ins.append(Band(R * B * C, F32, dev).put(x))
        outs.append(Band(R * C, F32, dev).put(o) if acc else Band(R * C, F32, dev))
        snaps.append(ins[-1].payload())
        x0.append(x)
        o0.append(o)
    impl.col_sum([b.t.view(R, B, C) for b, (R, B, C, _) in zip(ins, jobs)], [b.t for b in outs], [bool(j[3]) for j in jobs])
    _sync(dev)
    _count("col_sum")
    for j, (R, B, C, acc) in enumerate(jobs):
        nm = "%s: job %d" % (name, j)
        ins[j].verify(nm + " in")
        outs[j].verify(nm + " out")
        ins[j].same(nm + " in (read-only)", snaps[j])
        outs[j].written(nm + " out")
        s = torch.zeros(R, C, dtype=F32)
        for b in range(B):
            s = s + x0[j][:, b, :]
        want = (o0[j].view(R, C) + s) if acc else s
        got = outs[j].values().view(R, C)
        check_bits(nm, got.view(I32), want.view(I32), ("r", "c"))
        r64 = x0[j].to(F64).sum(1) + (o0[j].view(R, C).to(F64) if acc else 0.0)
        S = x0[j].to(F64).abs().sum(1) + (o0[j].view(R, C).to(F64).abs() if acc else 0.0)
        check_vals(nm + " (fp64)", got, r64, (B + 2) * EPS * S + TINY, "col_sum")


FC_M = (0, 1, 255, 256, 257, 1000)
FC_K = (1, 7, 8, 9, 29, 32)
FC_LDG = (32, 40, 64)
FC_SCALE, FC_ALPHA = f32r(0.37), f32r(1.0 / 7.0)


def fc_cases():
    return [(M, K, FC_LDG[(i + j) % 3], acc) for i, M in enumerate(FC_M) for j, K in enumerate(FC_K) for acc in (0, 1)]


class GBuf:
    """G [M, ldg] bf16, contiguous (the binding takes whole rows), inside a sentinel buffer:
    `before` rows above and 3 below; columns K..31 and the gap past column 32 hold the sentinel
    too. shift: elements by which the base is moved off its 16-B alignment."""

    def __init__(self, M, K, ldg, dev, vals=None, before=2, shift=0):
        self.buf = torch.empty((before + M + 3) * ldg, dtype=BFT, device=dev)
        self.buf.view(I16).fill_(SENT16)
        lo = before * ldg + shift
        self.G = self.buf[lo:lo + M * ldg].view(M, ldg)
        if vals is not None and M:
            self.G[:, :K].copy_(vals)
        self.snap = self.buf.view(I16).cpu().clone()

    def same(self, name):
        assert torch.equal(self.buf.view(I16).cpu(), self.snap), name + ": G (read-only) changed"


def fc_bias_ref(vals, out0):
    """fp32 emulation in the kernel's order: (result, result with the last step fused)"""
    M, K = vals.shape
    part = torch.zeros(256, K, dtype=F32)
    for r0 in range(0, M, 256):
        rows = vals[r0:r0 + 256].to(F32)
        part[:rows.shape[0]] = part[:rows.shape[0]] + rows
    t = torch.zeros(K, dtype=F32)
    for r in range(256):
        t = t + part[r]
    ts = t * torch.tensor(FC_SCALE, dtype=F32)
    t = ts * torch.tensor(FC_ALPHA, dtype=F32)
    if out0 is None:
        return t, t
    return out0 + t, (ts.to(F64) * FC_ALPHA + out0.to(F64)).to(F32)


def run_fc_bias(impl, dev, M, K, ldg, acc):
    name = "fc_bias_grad M=%d K=%d ldg=%d acc=%d" % (M, K, ldg, acc)
    g_ = _g(M * 37 + K)
    vals = torch.randn(M, K, generator=g_).to(BFT)
    o0 = torch.randn(K, generator=g_, dtype=F32)
    gb = GBuf(M, K, ldg, dev, vals)
    out = Band(K, F32, dev).put(o0) if acc else Band(K, F32, dev)
    scale = torch.tensor([FC_SCALE], dtype=F32, device=dev)
    impl.fc_bias_grad(gb.G, K, scale, FC_ALPHA, out.t, bool(acc))
    _sync(dev)
    _count("fc_bias_grad")
    out.verify(name + ": out")
    gb.same(name)
    got = out.values()
    if M == 0 and acc:
        check_bits(name + ": M = 0 with acc leaves out unchanged", got.view(I32), o0.view(I32))
        return
    out.written(name + ": out")
    want, fused = fc_bias_ref(vals, o0 if acc else None)
    check_bits(name, got.view(I32), want.view(I32), ("k",), either=fused.view(I32))
    sa = FC_SCALE * FC_ALPHA
    r64 = vals.to(F64).sum(0) * sa + (o0.to(F64) if acc else 0.0)
    S = vals.to(F64).abs().sum(0) * abs(sa) + (o0.to(F64).abs() if acc else 0.0)
    check_vals(name + " (fp64)", got, r64, (cdiv(max(M, 1), 256) + 256 + 4) * EPS * S + TINY, "fc_bias_grad")


# ------------------------------------------------------------------------------ fill.hip
MF_SIZES = (4, 12, 16, 4100)
MF_PATTERNS = (0, 0xFFFFFFFF, 0x7FC00000)
MF_DTYPES = (I32, F32, BFT, U8)


def mf_cases():
    """region lists of 0..8 regions: (dtype, bytes, shift, pattern)"""
    out = []
    k = 0
    for nreg in range(9):
        regs = []
        for _ in range(nreg):
            regs.append((MF_DTYPES[k % 4], MF_SIZES[(k // 4 + k) % 4], 4 * ((k // 2) % 2), MF_PATTERNS[k % 3]))
            k += 1
        out.append(regs)
    # every size on an aligned and on a 4-B aligned base, in one launch
    out.append([(I32, s, sh, MF_PATTERNS[(i + sh // 4) % 3]) for i, s in enumerate(MF_SIZES) for sh in (0, 4)])
    return out


def run_multi_fill(impl, dev, regs):
    name = "multi_fill " + " ".join("%s/%dB/+%d/0x%X" % (str(d).split(".")[1], nb, sh, pat) for d, nb, sh, pat in regs)
    bands = [Band(nb // torch.empty(0, dtype=d).element_size(), d, dev, shift=sh) for d, nb, sh, _ in regs]
    impl.multi_fill([b.t for b in bands], [pat for *_, pat in regs])
    _sync(dev)
    _count("multi_fill")
    for i, (b, (d, nb, sh, pat)) in enumerate(zip(bands, regs)):
        nm = "%s: region %d" % (name, i)
        b.verify(nm)
        es = torch.empty(0, dtype=d).element_size()
        words = b.buf.view(U8).cpu()[b.lo * es:b.lo * es + nb].clone().view(I32)
        want = pat - (1 << 32) if pat >= 1 << 31 else pat
        check_bits(nm, words, torch.full_like(words, want), ("word",))


def _fill_vals(shape, dtype, seed):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=F32) * 0.25 + seed + 1.0).view(*shape).to(dtype)       # never zero, never the sentinel


# pairs: ("1d", dtype, n_src, n_dst) or ("2d", dtype, rows, src_cols, dst_cols)
MC_PAIRS = (("1d", F32, 5, 5), ("2d", F32, 3, 7, 7), ("2d", BFT, 4, 6, 10), ("1d", BFT, 4, 10), ("2d", F32, 0, 3, 5),
            ("2d", F32, 300, 5, 9), ("1d", F32, 0, 3), ("2d", BFT, 2, 2, 2))
MC_CASES = [(list(MC_PAIRS[:k]), k % 5) for k in range(9)] + [([], ns) for ns in range(1, 5)] + [(list(MC_PAIRS[4:]), 0)]


def run_multi_copy(impl, dev, pairs, ns):
    name = "multi_copy %d pairs, %d scalars" % (len(pairs), ns)
    dsts, srcs, keep = [], [], []
    for i, pr in enumerate(pairs):
        if pr[0] == "1d":
            _, dt, n_s, n_d = pr
            v = _fill_vals((n_s,), dt, i)
            s, d = Band(n_s, dt, dev).put(v), Band(n_d, dt, dev)
            srcs.append(s.t)
            dsts.append(d.t)
        else:
            _, dt, rows, sc, dc = pr
            v = _fill_vals((rows, sc), dt, i)
            s, d = Plane(1, rows, sc, dt, dev, pad=16 + 8 * (i % 2)), Plane(1, rows, dc, dt, dev, pad=24)
            s.put(v) if rows else None
            srcs.append(s.t)
            dsts.append(d.t)
        keep.append((pr, v, s, d, s.buf.view(_ITY[dt][0]).cpu().clone()))
    vals = [0.5, -3.0, 1e-3, 7.0][:ns]
    sd = Band(4, F32, dev) if ns else None
    impl.multi_copy(dsts, srcs, None if sd is None else sd.t, vals)
    _sync(dev)
    _count("multi_copy")
    if sd is not None:
        sd.verify(name + ": scalars")
        want = torch.full((4,), SENT32, dtype=I32)
        want[:ns] = torch.tensor(vals, dtype=F32).view(I32)
        check_bits(name + ": scalar slot", sd.payload(), want)
    for i, (pr, v, s, d, s0) in enumerate(keep):
        nm = "%s: pair %d %s" % (name, i, pr)
        ity = _ITY[pr[1]][0]
        assert torch.equal(s.buf.view(ity).cpu(), s0), nm + ": the source changed"
        if pr[0] == "1d":
            d.verify(nm)
            want = torch.zeros(pr[3], dtype=pr[1])
            want[:pr[2]] = v
            check_bits(nm, d.payload(), want.view(ity))
        else:
            d.verify(nm)                             # bands and pitch gap untouched, payload written
            want = torch.zeros(pr[2], pr[4], dtype=pr[1])
            want[:, :pr[3]] = v
            check_bits(nm, d.t.cpu().contiguous().view(ity), want.view(ity), ("row", "col"))


PREP_N = (1, 3, 4, 5, 2055)
PREP_LENS = (-5, 0, 33, 34, 35, 37, 38, 100000)
PREP_NL = (1, 256, 257, 300)        # with n = 8: more lengths than n / 4 sized grid's threads


def run_prep(impl, dev, n, nl):
    name = "prep_inputs n=%d nl=%d" % (n, nl)
    x = cast_input(n, 5)                             # starts at the tie cases, no NaN before element 14
    x = torch.where(torch.isnan(x), torch.ones_like(x), x)
    li = torch.tensor([PREP_LENS[i % len(PREP_LENS)] for i in range(nl)], dtype=I32)
    X, Y = Band(n, F32, dev).put(x), Band(n, BFT, dev)
    LI, LO = Band(nl, I32, dev).put(li), Band(nl, I32, dev)
    sx, sl = X.payload(), LI.payload()
    impl.prep_inputs(X.t, Y.t, LI.t, LO.t)
    _sync(dev)
    _count("prep_inputs")
    for b, k in ((X, "x"), (Y, "y"), (LI, "lens_in"), (LO, "lens_out")):
        b.verify("%s: %s" % (name, k))
    X.same(name + ": x (read-only)", sx)
    LI.same(name + ": lens_in (read-only)", sl)
    check_bf16(name + ": cast", Y.values(), x)
    LO.written(name + ": lens_out")
    check_bits(name + ": lens_out against (t - 34) // 4", LO.payload(),
               torch.tensor([(int(t) - 34) // 4 for t in li.tolist()], dtype=I32))


TR_SIZES = (1, 7, 8, 63, 64, 65, 72, 129)


def run_transpose(impl, dev, R, C):
    name = "transpose_bf16 %dx%d" % (R, C)
    x = torch.randn(R, C, generator=_g(R * 131 + C)).to(BFT)
    pin, pout = Plane(1, R, C, BFT, dev, pad=24).put(x), Plane(1, C, R, BFT, dev, pad=16)
    assert pin.ld > C and pout.ld > R
    s0 = pin.buf.view(I16).cpu().clone()
    impl.transpose_bf16(pin.t, pout.t)
    _sync(dev)
    _count("transpose_bf16")
    pout.verify(name)
    assert torch.equal(pin.buf.view(I16).cpu(), s0), name + ": the source changed"
    check_bits(name, pout.t.cpu().contiguous().view(I16), x.t().contiguous().view(I16), ("c", "r"))


# ------------------------------------------------------------------------------ host refusals
def refusals(impl, dev):
    """(name, thunk, buffers) of calls that the host must refuse without launching anything; the
    buffers (Band / GBuf) must be bit-identical afterwards"""
    out = []
    n = 64
    h = (HYP["lr_t"], HYP["b1"], HYP["b2"], HYP["eps"], 1.0, HYP["keep"])

    def arrays(n=n, **kw):
        """p, g, m, v, ema, p16 bands; kw: name -> Band replacing one"""
        b = dict(p=Band(n, F32, dev), g=Band(n, F32, dev), m=Band(n, F32, dev), v=Band(n, F32, dev), e=Band(n, F32, dev),
                 h=Band(n, BFT, dev))
        b.update(kw)
        return b

    def adam(b, *tail):
        return lambda: impl.adam_ema(b["p"].t, b["g"].t, b["m"].t, b["v"].t, b["e"].t, b["h"].t, *h, *tail)

    def ranges(b, lohi):
        return lambda: impl.adam_ema_ranges(b["p"].t, b["g"].t, b["m"].t, b["v"].t, b["e"].t, b["h"].t, lohi, *h)

    class Strided:                                    # every second element of a band twice as long
        def __init__(self, n, dt):
            self.band = Band(2 * n, dt, dev)
            self.t = self.band.t[::2]

    for what, kw in (("ema of n - 4 elements", dict(e=Band(n - 4, F32, dev))), ("p16 of n + 4 elements", dict(h=Band(n + 4, BFT, dev))),
                     ("m of n - 4 elements", dict(m=Band(n - 4, F32, dev))), ("ema in bf16", dict(e=Band(n, BFT, dev))),
                     ("p16 in fp32", dict(h=Band(n, F32, dev))), ("p 4-B aligned", dict(p=Band(n, F32, dev, shift=4))),
                     ("g 8-B aligned", dict(g=Band(n, F32, dev, shift=8))), ("v 4-B aligned", dict(v=Band(n, F32, dev, shift=4))),
                     ("ema 4-B aligned", dict(e=Band(n, F32, dev, shift=4))), ("p16 4-B aligned", dict(h=Band(n, BFT, dev, shift=4))),
                     ("p16 2-B aligned", dict(h=Band(n, BFT, dev, shift=2)))):
        b = arrays(**kw)
        out.append(("adam_ema: " + what, adam(b, None, 0), list(b.values())))
        b = arrays(**kw)
        out.append(("adam_ema_ranges: " + what, ranges(b, [0, 8]), list(b.values())))
    for k, dt in (("p", F32), ("m", F32), ("v", F32), ("e", F32), ("h", BFT)):
        st = Strided(n, dt)
        b = arrays(**{k: st})
        out.append(("adam_ema: strided " + k, adam(b, None, 0), [x.band if isinstance(x, Strided) else x for x in b.values()]))
        st = Strided(n, dt)
        b = arrays(**{k: st})
        out.append(("adam_ema_ranges: strided " + k, ranges(b, [0, 8]), [x.band if isinstance(x, Strided) else x for x in b.values()]))
    b = arrays()
    out.append(("adam_ema: lds_reserve past 64 KB", adam(b, None, 0, None, 65537), list(b.values())))
    for what, lohi in (("65 ranges", [x for i in range(65) for x in (0, 0)]), ("a bound not on a multiple of 4", [0, 8, 12, 18]),
                       ("a start not on a multiple of 4", [2, 8]), ("overlapping ranges", [0, 16, 12, 24]),
                       ("a range inside another", [0, 32, 8, 12]), ("a bound past n", [0, n + 4]), ("an odd count", [0, 8, 12]),
                       ("hi < lo", [16, 8])):
        b = arrays()
        out.append(("adam_ema_ranges: " + what, ranges(b, lohi), list(b.values())))
    # grad_norm
    g = Band(n, F32, dev)
    for what, part, bad in (("an empty part", Band(0, F32, dev), Band(1, I32, dev)), ("a bf16 part", Band(4, BFT, dev), Band(1, I32, dev)),
                            ("a two-element bad", Band(1, F32, dev), Band(2, I32, dev)), ("an fp32 bad", Band(1, F32, dev), Band(1, F32, dev))):
        out.append(("grad_norm: " + what, (lambda p_=part, b_=bad: impl.grad_norm(g.t, 1.0, p_.t, b_.t)), [g, part, bad]))
    if torch.device(dev).type == "cuda":
        part, bad = Band(1, F32, dev), torch.zeros(1, dtype=I32)
        out.append(("grad_norm: bad on the host", (lambda: impl.grad_norm(g.t, 1.0, part.t, bad)), [g, part]))
    # multi_fill
    st = Strided(8, I32)
    out.append(("multi_fill: a strided view", (lambda: impl.multi_fill([st.t], [0])), [st.band]))
    b2 = Band(18, I32, dev)
    out.append(("multi_fill: 9 regions", (lambda: impl.multi_fill([b2.t[2 * i:2 * i + 1] for i in range(9)], [0] * 9)), [b2]))
    b3 = Band(3, BFT, dev)
    out.append(("multi_fill: 6 bytes", (lambda: impl.multi_fill([b3.t], [0])), [b3]))
    # fp8_quant2
    def quant(a8=None, b8=None, part=None, K=8, Kp=8):
        A, Bq = Band(2 * K, BFT, dev).put(torch.ones(2 * K)), Band(2 * K, BFT, dev).put(torch.ones(2 * K))
        a8 = a8 or Band(2 * Kp, F8, dev)
        b8 = b8 or Band(2 * Kp, F8, dev)
        part = part or Band(2, F32, dev)
        sc = Band(2, F32, dev)
        pt = part.t if isinstance(part, (Band, Strided)) else part
        return (lambda: impl.fp8_quant2(A.t.view(2, K), Bq.t.view(2, K), 1.0, a8.t.view(2, Kp), b8.t.view(2, Kp), pt, sc.t, None, None),
                [A, Bq, a8, b8, part.band if isinstance(part, Strided) else part, sc])
    out.append(("fp8_quant2: a8 4-B aligned",) + quant(a8=Band(16, F8, dev, shift=4)))
    out.append(("fp8_quant2: b8 4-B aligned",) + quant(b8=Band(16, F8, dev, shift=4)))
    out.append(("fp8_quant2: a strided part",) + quant(part=Strided(2, F32)))
    out.append(("fp8_quant2: part too short",) + quant(part=Band(1, F32, dev)))
    # col_sum
    cin, cout = Band(2 * 3 * 4, F32, dev), Band(8, F32, dev)
    out.append(("col_sum: 5 jobs", (lambda: impl.col_sum([cin.t.view(2, 3, 4)] * 5, [cout.t] * 5, [False] * 5)), [cin, cout]))
    out.append(("col_sum: a non-contiguous in", (lambda: impl.col_sum([cin.t.view(2, 4, 3).transpose(1, 2)], [cout.t], [False])), [cin, cout]))
    out.append(("col_sum: no jobs", (lambda: impl.col_sum([], [], [])), [cin, cout]))
    # fc_bias_grad
    scale = torch.tensor([1.0], dtype=F32, device=dev)
    for what, K, ldg, shift in (("K = 0", 0, 32, 0), ("K = 33", 33, 40, 0), ("fewer than 32 columns", 8, 24, 0),
                                ("ldg % 8 != 0", 8, 36, 0), ("a misaligned G", 8, 40, 4)):
        gb = GBuf(5, 0, ldg, dev, shift=shift)
        ob = Band(max(K, 1), F32, dev)
        out.append(("fc_bias_grad: " + what, (lambda gb=gb, ob=ob, K=K: impl.fc_bias_grad(gb.G, K, scale, 1.0, ob.t[:K] if K <= ob.n else ob.t, False)), [gb, ob]))
    gb = GBuf(5, 0, 40, dev)
    ob = Band(8, F32, dev)
    out.append(("fc_bias_grad: a pitched view of G", (lambda: impl.fc_bias_grad(gb.G[:, :32], 8, scale, 1.0, ob.t, False)), [gb, ob]))
    return out


def run_refusal(name, thunk, bufs, exc=RuntimeError):
    snaps = [b.snap if isinstance(b, GBuf) else b.bits() for b in bufs]
    try:
        thunk()
    except exc:
        pass
    else:
        raise AssertionError(name + ": not refused")
    _count("refusals")
    for b, s in zip(bufs, snaps):
        now = b.buf.view(I16).cpu() if isinstance(b, GBuf) else b.bits()
        assert torch.equal(now, s), name + ": a buffer changed although the call was refused"


# ------------------------------------------------------------------------------ coverage
def coverage():
    """What the tables reach, computed from them (asserted by tests/test_stream_oracle.py)"""
    c = {}
    c["adam_gs_n4"] = {n // 4 for n in ADAM_GS_N}
    c["adam_gs_tails"] = {(n // 4, n % 4) for n in ADAM_GS_N}
    c["adam_chunks"] = [chunk4(n, mg) + (n // 4,) for n, mg in ADAM_CHUNK]
    c["adam_chunk_grids"] = {mg for _, mg in ADAM_CHUNK}
    r = ADAM_RANGES["sixty-four"]
    srt = sorted(x for x in r if x[1] > x[0])
    c["ranges"] = dict(n=len(r), empty=sum(1 for lo, hi in r if lo == hi), adjacent=sum(1 for a, b in zip(srt, srt[1:]) if a[1] == b[0]),
                       start=any(lo == 0 and hi > 0 for lo, hi in r), end=any(hi == ARENA and lo < hi for lo, hi in r),
                       unsorted=r != sorted(r), disjoint=all(a[1] <= b[0] for a, b in zip(srt, srt[1:])),
                       gaps=any(a[1] < b[0] for a, b in zip(srt, srt[1:])), groups=sum(hi - lo for lo, hi in r) // 4)
    c["mf"] = dict(counts={len(x) for x in mf_cases()}, sizes={r_[1] for x in mf_cases() for r_ in x},
                   shifts={(r_[1], r_[2]) for x in mf_cases() for r_ in x}, patterns={r_[3] for x in mf_cases() for r_ in x},
                   dtypes={r_[0] for x in mf_cases() for r_ in x})
    c["mc"] = dict(counts={len(p) for p, _ in MC_CASES}, scalars={(ns, bool(p)) for p, ns in MC_CASES},
                   kinds={p[0] for p in MC_PAIRS}, narrower=any(p[0] == "2d" and p[3] < p[4] for p in MC_PAIRS),
                   zero_rows=any(p[0] == "2d" and p[2] == 0 for p in MC_PAIRS))
    c["fc"] = dict(M={x[0] for x in fc_cases()}, K={x[1] for x in fc_cases()}, ldg={x[2] for x in fc_cases()},
                   acc={x[3] for x in fc_cases()})
    c["cs"] = dict(jobs={len(j) for j in CS_CASES}, shapes={j[:3] for js in CS_CASES for j in js},
                   mixed=any(len({j[3] for j in js}) == 2 for js in CS_CASES),
                   boundaries_off_256=all(sum(j[0] * j[2] for j in js[:k]) % 256 != 0 for js in CS_CASES for k in range(1, len(js))))
    return c
