"""Step-local fp64 oracle, per-element checker, guard-banded buffers and case tables of the conv
front-end kernels (csrc/conv1.hip, conv2.hip, bn_cl.hip) and the NCHW BatchNorm kernels (csrc/bn_act.hip).
Pure torch, device-agnostic, does not import the extension.

Geometry: F1 = (F0-5)//2+1, F2 = F1-4, T1 = (T-20)//2+1, T2 = (T1-10)//2+1. Layouts are the
kernels': feats [N,T,F0], activations channels-last [N,T*,F*,32], weights OIHW, the RNN input
time-major [T2, N, 32*F2] with feature index c*F2 + f.

Method. Every kernel is checked from the inputs it actually read: conv2 from the z1 handed to
it, the statistics from the bf16 values the conv stored, the BatchNorm apply / backward from
the fp32 mean / invstd / dbeta / dgamma handed to it (the GPU's own, in a chained test). No
free-running fp64 chain, so no error is inherited and no clip mask flips by an upstream rounding.

Family A, exact integers. All operands are small integers (or powers of two) exact in bf16,
sparse enough that every product and every partial sum IN ANY ORDER is an integer below 2^24
(asserted by preconditions() from sum |x||w| for the outputs and from sum v^2 per channel for the
statistics). fp32 accumulation is then exact whatever the order, so bf16 outputs equal RNE-bf16
of the fp64 result, fp32 weight gradients and the statistics partials summed over workgroups
equal it bit for bit, and dbeta is exact. For dgamma and the fused sums of the data-gradient
epilogue mean = 0, invstd and gamma are powers of two with gamma*invstd = 1 and beta is an
integer, so xh, zz = y + beta and dd*xh (multiples of 1/8) are exact too; y takes the values
-beta and 20-beta, so the strict inequalities of the mask are exercised at zz == 0 and zz == 20
exactly. One dropped, doubled or misplaced term is visible at any K. Compared with torch.equal.

Family B, random reals: the rounding sites. Tolerances per element, eps = 2^-24 (fp32 unit
roundoff), r the fp64 result, S the same operation on absolute values (|bias| included), K the
number of terms, and h(v) = 2^(floor(log2 v) - 8), half a bf16 unit in the last place at magnitude
v: what one RNE store to bf16 (8 significand bits) can move a value by. h(v) lies between
2^-9 v (top of a binade) and 2^-8 v (bottom). A flat 2^-9 |r| is below the format's rounding error:
the correctly rounded emulation of tests/test_conv_oracle.py misses it on a fifth of the elements
(1.0039 stores as 1.0, 3.9e-3 off, against 2^-9 = 1.95e-3), so the exact half-ulp is used.
  K = 100 (conv1), 1600 (conv2 and its data gradient), N*T*F positions (weight gradients)
  d = 2 K eps S      the factor 2 because MFMA's internal accumulation rounding is undocumented
  fp32 outputs: d;   bf16 outputs: d + h(|r| + d)
  statistics partials (sum v, sum v^2 of the M stored values, v^2 exact in fp32): M eps sum|terms|
  BN apply z = clip(y sc + sh), sc = invstd*gamma, sh = beta - mean*sc in fp32:
      d = 4 eps (|y sc| + |sh|), tolerance d + h(|z| + d). clip is 1-Lipschitz, so an element within d
      of 0 or 20 may land on either side of the clip and still meets the bound: nothing to excuse.
  BN backward apply dy = g is (dd - dbeta/M - xh dgamma/M) from the dbeta / dgamma handed in:
      d = 8 eps g is (|dd| + |dbeta/M| + |xh dgamma/M|), tolerance d + h(|dy| + d)
  dbeta = sum dd, dgamma = sum dd xh:  M eps sum|terms| (+ the terms of mask-ambiguous elements)
  mask-ambiguous: fp64 zz within 8 eps (|xh g| + |beta|) of 0 or 20. Such elements are excused in
      dy (cap: 0.1 % of a tensor, asserted on the CPU for every case) and their |dz|, |dz xh|
      are added to the dbeta / dgamma tolerance.
  mean from the partials: M eps mean|v| + 2^-23 |mean|. invstd: relative 2^-11 (a quarter bf16 ulp
      of what the scale multiplies) at |mean|/std <= 8. Running statistics: 1e-6 + 2^-23 relative
      against the update from the fp64 statistics (unbiased variance, M - 1).
BN parameters of both families put >= 5 % of the elements below 0 and >= 5 % above 20
(gamma ~ 8, beta ~ 10 on a standardised input: ~10 % each), asserted by preconditions().

Exact zeros: data-gradient rows t1 > 2 (T2-1) + 9, which no output row reads; conv1's weight
gradient when the input is nonzero only where conv1 never reads (the frame an odd T leaves over,
the last bin of an even F0). Guard bands: every output and partials buffer is a view into a
larger buffer prefilled with a sentinel bit pattern (a NaN); the bands must come back untouched
and no payload element may still hold the sentinel.
"""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
CLIP = 20.0
BN_EPS = 1e-3
BN_MOM = 0.01
CC = 32
F64 = torch.float64
GUARD = 64                      # elements on each side: keeps the payload 16-B aligned
SENT16 = 0x7FA5                 # bf16 NaN with a payload no kernel produces
SENT32 = 0x7FC5A5A5             # fp32 NaN, likewise
EXCUSE_CAP = 1e-3
WORST = {}                      # kernel -> worst err/tol seen (profiles/conv_oracle_coverage.md)


def geom(T, F0):
    T1, F1 = (T - 20) // 2 + 1, (F0 - 5) // 2 + 1
    return T1, F1, (T1 - 10) // 2 + 1, F1 - 4


# ------------------------------------------------------------------------------ oracle (fp64)
def conv1_fwd(x, w, b):
    """x [N,T,F0], w [32,1,20,5], b [32] -> [N,T1,F1,32]"""
    return F.conv2d(x.unsqueeze(1), w, b, stride=(2, 2)).permute(0, 2, 3, 1).contiguous()


def conv2_fwd(z, w, b):
    """z [N,T1,F1,32], w [32,32,10,5], b [32] -> [N,T2,F2,32]"""
    return F.conv2d(z.permute(0, 3, 1, 2), w, b, stride=(2, 1)).permute(0, 2, 3, 1).contiguous()


def conv2_dgrad(dy, w, T1):
    """dx[n,t1,f1,ci] = sum dy[n,(t1-kt)/2,f1-kf,co] w[co,ci,kt,kf]; rows past 2(T2-1)+9 are zero"""
    N, T2, F2, _ = dy.shape
    dx = torch.zeros(N, T1, F2 + 4, CC, dtype=dy.dtype)
    for kt in range(10):
        for kf in range(5):
            dx[:, kt:kt + 2 * T2 - 1:2, kf:kf + F2] += torch.einsum("ntfo,oi->ntfi", dy, w[:, :, kt, kf])
    return dx


def conv2_wgrad(dy, x):
    """dw[co,ci,kt,kf] = sum_{n,t2,f2} dy[n,t2,f2,co] x[n,2 t2+kt,f2+kf,ci]"""
    N, T2, F2, _ = dy.shape
    dw = torch.zeros(CC, CC, 10, 5, dtype=dy.dtype)
    for kt in range(10):
        for kf in range(5):
            dw[:, :, kt, kf] = torch.einsum("ntfo,ntfi->oi", dy, x[:, kt:kt + 2 * T2 - 1:2, kf:kf + F2])
    return dw


def conv1_wgrad(dy, x):
    """dw[co,0,kt,kf] = sum_{n,t1,f1} dy[n,t1,f1,co] x[n,2 t1+kt,2 f1+kf]"""
    N, T1, F1, _ = dy.shape
    dw = torch.zeros(CC, 1, 20, 5, dtype=dy.dtype)
    for kt in range(20):
        for kf in range(5):
            dw[:, 0, kt, kf] = torch.einsum("ntfo,ntf->o", dy, x[:, kt:kt + 2 * T1 - 1:2, kf:kf + 2 * F1 - 1:2])
    return dw


def part_sums(y):
    """(sum v, sum v^2) per channel of the stored values, [32, 2]"""
    v = y.to(F64).reshape(-1, y.shape[-1])
    return torch.stack([v.sum(0), (v * v).sum(0)], 1)


def stats(y, eps=BN_EPS):
    """mean, biased variance, invstd, M of the stored values"""
    v = y.to(F64).reshape(-1, y.shape[-1])
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    return mean, var, (var + eps).rsqrt(), v.shape[0]


def running(rm, rv, mean, var, M, mom=BN_MOM):
    unb = var * M / (M - 1) if M > 1 else var
    return (1 - mom) * rm.to(F64) + mom * mean, (1 - mom) * rv.to(F64) + mom * unb


def to_tmaj(z):
    """channels-last [N,T,F,C] -> time-major [T, N, C*F] (feature c*F + f)"""
    N, T, Fd, C = z.shape
    return z.permute(1, 0, 3, 2).reshape(T, N, C * Fd)


def from_tmaj(z, Fd):
    T, N, CF = z.shape
    return z.reshape(T, N, CF // Fd, Fd).permute(1, 0, 3, 2)


def bn_zz(y, p):
    xh = (y - p["mean"]) * p["inv"]
    return xh, xh * p["gamma"] + p["beta"]


def store_err(v, store):
    """what the final store can move a value of magnitude v by"""
    return hulp(v) if store == "bf16" else EPS * v


def bn_apply(y, p, store="bf16", dy_in=None):
    """-> z (channels-last), per-element tolerance. dy_in: bound on an error already in y
    (a chained check): it reaches z scaled by |sc|."""
    sc = p["inv"] * p["gamma"]
    sh = p["beta"] - p["mean"] * sc
    z = (y * sc + sh).clamp(0, CLIP)
    d = 4 * EPS * ((y * sc).abs() + sh.abs())
    if dy_in is not None:
        d = d + sc.abs() * dy_in
    return z, d + store_err(z.abs() + d, store)


def bn_bwd(dz, y, p, dbeta=None, dgamma=None, store="bf16"):
    """dz, y channels-last fp64. dy is formed from the dbeta / dgamma handed in (the kernel's own);
    without them from the oracle's."""
    xh, zz = bn_zz(y, p)
    C = y.shape[-1]
    M = y.numel() // C
    m = (zz > 0) & (zz < CLIP)
    a = 8 * EPS * ((xh * p["gamma"]).abs() + p["beta"].abs())
    amb = (zz.abs() <= a) | ((zz - CLIP).abs() <= a)
    dd = dz * m
    red = lambda t: t.reshape(-1, C).sum(0)
    db, dg = red(dd), red(dd * xh)
    tol_db = M * EPS * red(dd.abs()) + red(dz.abs() * amb)
    tol_dg = M * EPS * red((dd * xh).abs()) + red((dz * xh).abs() * amb)
    dbu = db if dbeta is None else dbeta.to(F64)
    dgu = dg if dgamma is None else dgamma.to(F64)
    k = p["gamma"] * p["inv"]
    dy = k * (dd - dbu / M - xh * dgu / M)
    d = 8 * EPS * k.abs() * (dd.abs() + (dbu / M).abs() + (xh * dgu / M).abs())
    return dict(dbeta=db, dgamma=dg, tol_dbeta=tol_db, tol_dgamma=tol_dg, dy=dy, tol_dy=d + store_err(dy.abs() + d, store),
                amb=amb, mask=m, zz=zz)


def hulp(v):
    """half a bf16 unit in the last place at magnitude v >= 0 (0 at 0)"""
    _, e = torch.frexp(v.to(F64))                   # v = m 2^e, m in [0.5, 1)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v, dtype=F64), e - 9), torch.zeros_like(v, dtype=F64))


def chained_stats(r, tol_y, eps=BN_EPS):
    """Batch statistics of an output known only as r +- tol_y (a chained check): fp64 mean / invstd
    of r and bounds on how far the kernel's own may lie. |d mean| <= mean(tol_y); with e the
    error, d var <= 2 std rms(e) + rms(e)^2 (Cauchy-Schwarz), and d inv / inv <= d var / (var + eps)
    (the first-order factor 1/2 left out to cover the curvature), plus 2^-11 for the one-pass
    sums."""
    mean, var, inv, M = stats(r)
    e = tol_y.reshape(-1, r.shape[-1])
    rms = e.pow(2).mean(0).sqrt()
    dvar = 2 * var.sqrt() * rms + rms * rms
    return mean, inv, e.mean(0) + 2.0 ** -22 * mean.abs(), dvar / (var + eps) + 2.0 ** -11


def tol_f32(S, K):
    return 2 * K * EPS * S


def tol_bf16(r, S, K):
    d = 2 * K * EPS * S
    return d + hulp(r.abs() + d)


# ------------------------------------------------------------------------------ checker
class Mismatch(AssertionError):
    def __init__(self, msg, coords):
        super().__init__(msg)
        self.coords = coords


def _coords(idx, shape, dims):
    out = {}
    for name, size in zip(reversed(dims), reversed(shape)):
        out[name] = int(idx % size)
        idx //= size
    return {k: out[k] for k in dims}


def check(name, got, want, tol, dims, excused=None, kernel=None):
    """Per element |got - want| <= tol (non-finite got fails). Names the worst element."""
    got = got.detach().to("cpu").to(F64)
    want = want.to(F64)
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    tol = torch.as_tensor(tol, dtype=F64).expand_as(want)
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    if excused is not None:
        share = excused.double().mean().item()
        assert share <= EXCUSE_CAP, "%s: %.4f %% of the elements are mask-ambiguous (cap 0.1 %%)" % (name, 100 * share)
        ratio = torch.where(excused.expand_as(ratio), torch.zeros_like(ratio), ratio)
    worst = ratio.max().item() if ratio.numel() else 0.0
    if kernel is not None and math.isfinite(worst):
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        c = _coords(i, want.shape, dims)
        raise Mismatch("%s: %d of %d elements beyond tolerance; worst at %s: got %r want %r err %.3e tol %.3e" % (
            name, int((ratio > 1).sum()), ratio.numel(), ", ".join("%s=%d" % kv for kv in c.items()),
            got.reshape(-1)[i].item(), want.reshape(-1)[i].item(), err.reshape(-1)[i].item(),
            tol.reshape(-1)[i].item()), c)
    return worst


def check_equal(name, got, want, dims, origin=None):
    """Bitwise-level equality of values (family A, zero regions). want fp64, exact in got's type."""
    got = got.detach().to("cpu")
    w = want.to(got.dtype)
    assert got.shape == w.shape, (name, tuple(got.shape), tuple(w.shape))
    assert torch.equal(w.to(F64), want.to(F64)), "%s: the expected value is not exact in %s" % (name, got.dtype)
    if torch.equal(got, w):
        return
    bad = ~(got == w)
    i = int(bad.reshape(-1).to(torch.uint8).argmax())
    c = _coords(i, w.shape, dims)
    for k, v in (origin or {}).items():          # got / want are slices starting there
        c[k] += v
    raise Mismatch("%s: %d of %d elements differ; first at %s: got %r want %r" % (
        name, int(bad.sum()), bad.numel(), ", ".join("%s=%d" % kv for kv in c.items()),
        got.reshape(-1)[i].item(), w.reshape(-1)[i].item()), c)


def rne_bf16(r):
    """fp64 -> bf16 by one RNE rounding (the values used here are exact in fp32 first)"""
    r32 = r.to(torch.float32)
    assert torch.equal(r32.to(F64), r), "value not exact in fp32"
    return r32.to(torch.bfloat16)


def old_ratio(a, b):
    """the whole-tensor figure of tests/test_conv_gpu.py"""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------------ guard bands
class Guarded:
    """A contiguous tensor `t` inside a larger buffer; everything prefilled with a sentinel."""

    def __init__(self, shape, dtype, device):
        n = 1
        for s in shape:
            n *= int(s)
        self.n = n
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=device)
        self.ity, self.sent = (torch.int16, SENT16) if dtype == torch.bfloat16 else (torch.int32, SENT32)
        assert dtype in (torch.bfloat16, torch.float32)
        self.buf.view(self.ity).fill_(self.sent)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)

    def verify(self, name, written=True):
        """bands untouched; payload fully overwritten (or, written=False, fully untouched)"""
        iv = self.buf.view(self.ity).cpu()
        lo, mid, hi = iv[:GUARD], iv[GUARD:GUARD + self.n], iv[GUARD + self.n:]
        assert bool((lo == self.sent).all()), "%s: the guard band below the buffer was written" % name
        assert bool((hi == self.sent).all()), "%s: the guard band above the buffer was written" % name
        left = int((mid == self.sent).sum())
        if written:
            assert left == 0, "%s: %d of %d payload elements were never written" % (name, left, self.n)
        else:
            assert left == self.n, "%s: %d payload elements were written, none should be" % (name, self.n - left)


# ------------------------------------------------------------------------------ inputs
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, lo, hi, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v


def _bf(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def _f32(t):
    return t.to(torch.float32).to(F64)


A_PAIRS = ((0.25, 4.0), (0.5, 2.0), (1.0, 1.0), (0.125, 8.0))      # (invstd, gamma), product 1


@functools.lru_cache(maxsize=8)
def make(fam, N, T, F0):
    """All operands of one geometry, fp64 CPU tensors holding bf16-exact (activations, weights) or
    fp32-exact (biases, BN vectors) values. Cached: the tests share them and must not modify them."""
    T1, F1, T2, F2 = geom(T, F0)
    g = _g(1000003 * N + 1009 * T + F0 + (0 if fam == "A" else 7))
    d = dict(fam=fam, N=N, T=T, F0=F0, T1=T1, F1=F1, T2=T2, F2=F2)
    if fam == "A":
        d["x"] = _ints(g, (N, T, F0), -1, 1, 0.25)            # conv1 forward
        d["xd"] = _ints(g, (N, T, F0), -8, 8)                  # conv1 weight gradient
        d["w1"] = _ints(g, (CC, 1, 20, 5), -4, 4)
        d["b1"] = _ints(g, (CC,), -3, 3)
        d["z1"] = _ints(g, (N, T1, F1, CC), -1, 1, 1 / 16)     # conv2 forward
        d["z1d"] = _ints(g, (N, T1, F1, CC), -8, 8)            # conv2 weight gradient
        d["w2"] = _ints(g, (CC, CC, 10, 5), -4, 4)
        d["b2"] = _ints(g, (CC,), -3, 3)
        d["dy2"] = _ints(g, (N, T2, F2, CC), -1, 1, 1 / 16)    # conv2 data gradient
        d["dy2d"] = _ints(g, (N, T2, F2, CC), -8, 8)
        d["dy1"] = _ints(g, (N, T1, F1, CC), -8, 8)
        for tag, sh in (("1", (N, T1, F1, CC)), ("2", (N, T2, F2, CC))):
            beta = torch.tensor([9.0, 10.0, 11.0, 10.0] * 8, dtype=F64)
            y = _ints(g, sh, -13, 13)
            # the mask boundaries themselves: zz == 0 and zz == 20 exactly, a few per channel
            edge = torch.rand(sh, generator=g)
            y = torch.where(edge < 0.02, -beta.expand(sh), y)
            y = torch.where(edge > 0.98, (CLIP - beta).expand(sh), y)
            d["y" + tag] = y
            d["bn" + tag] = dict(mean=torch.zeros(CC, dtype=F64),
                                 inv=torch.tensor([A_PAIRS[c % 4][0] for c in range(CC)], dtype=F64),
                                 gamma=torch.tensor([A_PAIRS[c % 4][1] for c in range(CC)], dtype=F64), beta=beta)
    else:
        rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
        d["x"] = d["xd"] = _bf(rn(N, T, F0))
        d["w1"] = _bf(0.1 * rn(CC, 1, 20, 5))
        d["b1"] = _f32(0.1 * rn(CC))
        d["z1"] = d["z1d"] = _bf(torch.rand(N, T1, F1, CC, generator=g, dtype=F64))
        d["w2"] = _bf(0.05 * rn(CC, CC, 10, 5))
        d["b2"] = _f32(0.1 * rn(CC))
        d["dy2"] = d["dy2d"] = _bf(rn(N, T2, F2, CC))
        d["dy1"] = _bf(rn(N, T1, F1, CC))
        for tag, sh in (("1", (N, T1, F1, CC)), ("2", (N, T2, F2, CC))):
            y = _bf(2 * rn(*sh) + 0.5 * rn(CC))
            mean, _, inv, _ = stats(y)
            d["y" + tag] = y
            d["bn" + tag] = dict(mean=_f32(mean), inv=_f32(inv), gamma=_f32(8 + 0.5 * rn(CC)),
                                 beta=_f32(10 + rn(CC)))
    return d


def conditioned(ratio, N=2, T=100, F0=161, seed=5):
    """conv1 operands whose output has std ~ 1 and |mean|/std = ratio per channel (the bias sets
    the mean). M = N*T1*F1 = 6478."""
    g = _g(seed)
    x = _bf(torch.randn(N, T, F0, generator=g, dtype=F64))
    w = _bf(0.1 * torch.randn(CC, 1, 20, 5, generator=g, dtype=F64))
    std = conv1_fwd(x, w, None).reshape(-1, CC).std(0)
    sign = torch.where(torch.arange(CC) % 2 == 0, 1.0, -1.0).to(F64)
    return x, w, _f32(ratio * std * sign)


def preconditions(d):
    """What the families promise, asserted from the operands (CPU)."""
    lim = 2.0 ** 24
    for tag in ("1", "2"):
        y, p = d["y" + tag], d["bn" + tag]
        _, zz = bn_zz(y, p)
        lo, hi = (zz <= 0).double().mean().item(), (zz >= CLIP).double().mean().item()
        assert lo >= 0.05 and hi >= 0.05, ("clip regions", tag, lo, hi)
    if d["fam"] != "A":
        return
    a = lambda k: d[k].abs()
    y1, y2 = conv1_fwd(d["x"], d["w1"], d["b1"]), conv2_fwd(d["z1"], d["w2"], d["b2"])
    assert conv1_fwd(a("x"), a("w1"), a("b1")).max() < lim and conv2_fwd(a("z1"), a("w2"), a("b2")).max() < lim
    for y in (y1, y2):                       # statistics of the stored (integer) outputs
        assert torch.equal(rne_bf16(y).to(F64), y) and part_sums(y)[:, 1].max() < lim
    assert conv2_dgrad(a("dy2"), a("w2"), d["T1"]).max() < lim
    assert conv2_wgrad(a("dy2d"), a("z1d")).max() < lim and conv1_wgrad(a("dy1"), a("xd")).max() < lim
    # fused sums over the stored data gradient and the BatchNorm backward sums: multiples of 1/8
    dx = rne_bf16(conv2_dgrad(d["dy2"], d["w2"], d["T1"])).to(F64)
    for dz, tag in ((dx, "1"), (d["dy1"], "1"), (d["dy2d"], "2")):
        xh, _ = bn_zz(d["y" + tag], d["bn" + tag])
        assert torch.equal((xh * 8).round(), xh * 8)
        assert 8 * (dz.abs() * xh.abs()).reshape(-1, CC).sum(0).max() < lim
        assert dz.abs().reshape(-1, CC).sum(0).max() < lim


# ------------------------------------------------------------------------------ verifiers
# (shared by the CPU emulation test and the GPU test: `got` tensors may live on any device)
NTFC = ("n", "t", "f", "c")


def verify_fwd(which, d, y, psum, kernel=None):
    """conv1 / conv2 forward with bias: output [N,T*,F*,32] bf16 and the statistics partials summed
    over workgroups in fp64, psum [32, 2]"""
    if which == 1:
        fn, ops, K = conv1_fwd, ("x", "w1", "b1"), 100
    else:
        fn, ops, K = conv2_fwd, ("z1", "w2", "b2"), 1600
    kernel = kernel or "conv%d_fwd" % which
    r = fn(*(d[k] for k in ops))
    name = "%s %s N=%d T=%d F0=%d" % (kernel, d["fam"], d["N"], d["T"], d["F0"])
    want_p = part_sums(y.detach().cpu())
    M = y.numel() // CC
    if d["fam"] == "A":
        check_equal(name + " y", y, r, NTFC)
        check_equal(name + " partials", psum.to(F64), want_p, ("c", "k"))
    else:
        S = fn(*(d[k].abs() for k in ops))
        check(name + " y", y, r, tol_bf16(r, S, K), NTFC, kernel=kernel)
        v = y.detach().cpu().to(F64).reshape(-1, CC)
        tol = M * EPS * torch.stack([v.abs().sum(0), (v * v).sum(0)], 1)
        check(name + " partials", psum, want_p, tol, ("c", "k"), kernel=kernel + " partials")


def verify_finalize(name, y, mean, inv, rm0=None, rv0=None, rm=None, rv=None, inv_rel=2.0 ** -11):
    """batch statistics (bn_cl_finalize, bn_stats) against the fp64 statistics of the stored values
    y [..., C]; returns the worst relative invstd error"""
    m64, var, i64, M = stats(y.detach().cpu())
    v = y.detach().cpu().to(F64).reshape(-1, y.shape[-1])
    check(name + " mean", mean, m64, M * EPS * v.abs().mean(0) + 2.0 ** -23 * m64.abs(), ("c",), kernel="bn_cl_finalize mean")
    if inv_rel is not None:
        check(name + " invstd", inv, i64, inv_rel * i64, ("c",), kernel="bn_cl_finalize invstd")
    if rm is not None:
        wm, wv = running(rm0, rv0, m64, var, M)
        check(name + " running_mean", rm, wm, 1e-6 + 2.0 ** -23 * wm.abs(), ("c",))
        check(name + " running_var", rv, wv, 1e-6 + 2.0 ** -23 * wv.abs(), ("c",))
    return ((inv.detach().cpu().to(F64) - i64).abs() / i64).max().item()


def verify_dgrad(d, dx, kernel="conv2_dgrad"):
    r = conv2_dgrad(d["dy2"], d["w2"], d["T1"])
    name = "%s %s N=%d T=%d F0=%d" % (kernel, d["fam"], d["N"], d["T"], d["F0"])
    first_zero = 2 * (d["T2"] - 1) + 10
    if first_zero < d["T1"]:
        assert float(r[:, first_zero:].abs().max()) == 0.0
        check_equal(name + " zero rows", dx[:, first_zero:], r[:, first_zero:], NTFC, origin=dict(t=first_zero))
    if d["fam"] == "A":
        check_equal(name + " dx", dx, r, NTFC)
    else:
        S = conv2_dgrad(d["dy2"].abs(), d["w2"].abs(), d["T1"])
        check(name + " dx", dx, r, tol_bf16(r, S, 1600), NTFC, kernel=kernel)


def verify_sums(name, fam, dz, y, p, psum, kernel):
    """BatchNorm-backward sums (sum dd, sum dd xh) per channel, psum [32, 2] = fp64 sum of the
    workgroup partials, or (dbeta, dgamma) stacked"""
    o = bn_bwd(dz.detach().cpu().to(F64), y, p)
    want = torch.stack([o["dbeta"], o["dgamma"]], 1)
    if fam == "A":
        check_equal(name, psum.detach().cpu().to(F64), want, ("c", "k"))
    else:
        check(name, psum, want, torch.stack([o["tol_dbeta"], o["tol_dgamma"]], 1), ("c", "k"), kernel=kernel)


def verify_wgrad(which, d, dw, dy=None, kernel=None):
    """dy: the gradient the kernel actually multiplied (default: the case's)"""
    kernel = kernel or "conv%d_wgrad" % which
    name = "%s %s N=%d T=%d F0=%d" % (kernel, d["fam"], d["N"], d["T"], d["F0"])
    if which == 1:
        fn, a, b, dims = conv1_wgrad, d["dy1"] if dy is None else dy, d["xd"], ("co", "ci", "kt", "kf")
    else:
        fn, a, b, dims = conv2_wgrad, d["dy2d"] if dy is None else dy, d["z1d"], ("co", "ci", "kt", "kf")
    r = fn(a, b)
    if d["fam"] == "A" and dy is None:
        check_equal(name, dw, r, dims)
    else:
        K = a.numel() // CC
        check(name, dw, r, tol_f32(fn(a.abs(), b.abs()), K), dims, kernel=kernel)


def verify_apply(name, fam, y, p, out, tmaj, kernel, store="bf16", dy_in=None):
    z, tol = bn_apply(y, p, store, dy_in)
    if tmaj:
        z, tol, dims = to_tmaj(z), to_tmaj(tol), ("t", "n", "cf")
    else:
        dims = NTFC
    if fam == "A":
        check_equal(name, out, z, dims)
    else:
        check(name, out, z, tol, dims, kernel=kernel)


def verify_bwd(name, fam, dz, y, p, dg, db, dy, kernel, store="bf16"):
    """dz, y fp64 channels-last; dg, db, dy the kernel's (dy may be None: part_ready == 2)"""
    verify_sums(name + " dbeta/dgamma", fam, dz, y, p, torch.stack([db, dg], 1).to(F64), kernel + " sums")
    if dy is None:
        return
    o = bn_bwd(dz, y, p, db.detach().cpu(), dg.detach().cpu(), store)
    # family A: xh and zz are exact in fp32 too, so the mask is decided, at zz == 0 and 20 as well
    check(name + " dy", dy, o["dy"], o["tol_dy"], NTFC, excused=None if fam == "A" else o["amb"],
          kernel=kernel + " dy")


# ------------------------------------------------------------------------------ case tables
# (N, T, F0[, grid]). T in {38, 39, 40, 42, 44, 61, 100}: 38 the minimum (T1 10, T2 1); 39 one
# unread frame; 40: T1 = 11, odd, so the data gradient's last row pair is single, z1 row 10 is
# never read by conv2 and conv1's last workgroup has 3 live waves; 42, 44: T2 = 2; 61: T1 21,
# T2 6; 100: T1 41, T2 16. F0 in {22, 67, 69, 75, 77, 131, 133, 161, 162, 163}: F1 = 9, 32, 33,
# 36, 37, 64, 65, 79, 79, 80 (the m-tile edges of F1 and of F2 = F1 - 4, the capacity edge 80, an
# even bin count).
CONV1_FWD = [(1, 38, 22), (2, 39, 67), (3, 40, 69), (1, 42, 75), (2, 44, 77), (1, 61, 131), (2, 100, 133),
             (3, 40, 161), (1, 38, 162), (2, 40, 163), (1, 100, 163), (3, 61, 161)]
# grids {1, 7, 8, 64}: 64 exceeds the tile count N*T2 of every small T, 8 splits by XCD
CONV2_FWD = [(1, 38, 22, 1), (2, 39, 67, 7), (3, 40, 69, 8), (1, 42, 75, 64), (2, 44, 77, 1), (1, 61, 131, 7),
             (2, 100, 133, 8), (3, 61, 161, 64), (1, 40, 162, 8), (2, 38, 163, 64), (3, 100, 163, 7),
             (1, 44, 161, 1), (2, 42, 133, 64), (1, 39, 163, 8)]
# grids {1, 3, 64}
CONV2_WGRAD = [(1, 38, 22, 1), (2, 39, 67, 3), (3, 40, 69, 64), (1, 42, 75, 3), (2, 44, 77, 64), (1, 61, 131, 1),
               (2, 100, 133, 3), (3, 61, 161, 64), (1, 40, 162, 1), (2, 38, 163, 3), (1, 100, 163, 64),
               (3, 44, 161, 3)]
CONV1_WGRAD = [(1, 38, 22, 64), (2, 39, 67, 1), (3, 40, 69, 3), (1, 42, 75, 1), (2, 44, 77, 3), (1, 61, 131, 64),
               (2, 100, 133, 1), (3, 61, 161, 3), (1, 40, 162, 64), (2, 38, 163, 1), (1, 100, 163, 3),
               (3, 44, 161, 64)]
# fused BatchNorm backward in the staging: the widths the data gradient that feeds it admits
CONV1_WGRAD_BN = [(1, 38, 133, 1), (2, 39, 161, 3), (3, 40, 162, 64), (1, 42, 163, 3), (2, 44, 133, 64),
                  (1, 61, 162, 1), (2, 100, 163, 64)]
# grids {1, 5, 8, 16, 512}; N = 1, T = 38 has 5 tiles, so a grid of 8 or 16 leaves XCD ranges
# empty; each case runs without and with the BatchNorm epilogue
CONV2_DGRAD = [(1, 38, 161, 8), (1, 38, 163, 5), (1, 38, 133, 16), (2, 39, 162, 1), (3, 40, 163, 8),
               (1, 40, 133, 512), (2, 42, 161, 5), (1, 44, 162, 16), (2, 44, 163, 1), (1, 61, 133, 8),
               (3, 61, 163, 512), (2, 100, 161, 16), (1, 100, 162, 5), (2, 100, 133, 512)]
# (N, T, F0, time-major): channels-last applies run on conv1's geometry [N,T1,F1], time-major
# ones on conv2's [N,T2,F2]
BN_APPLY = [(n, t, f0, tm) for tm in (False, True) for (n, t, f0) in
            [(1, 38, 22), (2, 39, 67), (3, 40, 69), (1, 42, 75), (2, 44, 77), (1, 61, 131), (2, 100, 133),
             (3, 61, 161), (1, 40, 162), (2, 100, 163)]]
# (N, T, F0, time-major, nb); every case also replays its partials with part_ready 1 and 2
# where the layout allows it (channels-last only)
BN_BWD = [(1, 38, 22, False, 1), (2, 39, 67, True, 13), (3, 40, 69, False, 1024), (1, 42, 75, True, 1),
          (2, 44, 77, False, 13), (1, 61, 131, True, 1024), (2, 100, 133, False, 1), (3, 61, 161, True, 13),
          (1, 40, 162, False, 1024), (2, 100, 163, True, 1), (1, 100, 163, False, 13), (2, 61, 161, True, 1024),
          (3, 100, 161, False, 13)]
STAT_RATIOS = (0, 4, 8, 32, 128)
TABLES = dict(conv1_fwd=CONV1_FWD, conv2_fwd=CONV2_FWD, conv2_wgrad=CONV2_WGRAD, conv1_wgrad=CONV1_WGRAD,
              conv1_wgrad_bn=CONV1_WGRAD_BN, conv2_dgrad=CONV2_DGRAD, bn_apply=BN_APPLY, bn_bwd=BN_BWD)


def geometries():
    """every (N, T, F0) of the tables"""
    return sorted({c[:3] for t in TABLES.values() for c in t})


def ident(c):
    return "-".join(str(int(v)) if not isinstance(v, bool) else ("tmaj" if v else "cl") for v in c)
