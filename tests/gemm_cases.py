"""fp64 oracle, per-element checker, guard-banded buffers and case tables of the GEMM kernels
(csrc/gemm.hip: nine tile configurations, four operand layouts; csrc/gemm8.hip: bf16 and fp8,
column-mode operands, split-K, the external reduce, grouped launches) and of ops/gemm.py's
routing. Pure torch, device-agnostic, does not import the extension. The idioms and constants are
those of tests/conv_cases.py.

Oracle. r = alpha a_dev a_dev2 (A B^T) + bias + c0 in fp64 from the STORED operands exactly as the
kernel reads them: A(m,k) = A[m][k] (row mode) or A[k][m] (column mode), likewise B; a batch; a
column-mode operand padded to Ml columns (columns M..Ml are poison) or holding only Kl k-rows (the
other operand then holds zeros in k >= Kl: the Kl contract). S_abs is the same operation on
absolute values.

Family A, exact integers. Every operand element is a nonzero integer in +-{1, 2, 3} (exact in bf16
and in e4m3; no term is zero, so a dropped, doubled or misplaced term changes the result), alpha
and the device scalars are powers of two, the bias and the initial C (epi 2) are integers.
preconditions() asserts S_abs < 2^24, so fp32 accumulation is exact in any order and with any
split: fp32 outputs equal the oracle bit for bit, bf16 outputs equal RNE-bf16 of it. A third of
the bias entries have magnitude 256..512, so the stored sums are odd integers and half-integers
that bf16 cannot hold and the store's rounding (ties included) is exercised.

Family B, random reals. A ~ N(0,1), B ~ 0.05 N(0,1) + 0.01, bias ~ N(0,1), alpha = 0.75, device
scalars 1.3 and 0.7 (fp32). With K terms and S k-slices, per element
    d = (2 (K + S) + 8) EPS S_abs          fp32 outputs: d      bf16 outputs: d + h(|r| + d)
EPS = 2^-24, h(v) half a bf16 ulp at v. The factor 2 is the project's allowance for MFMA's
undocumented internal accumulation order; + 8 covers the fp32 product of the scales and the
epilogue fma (csrc/gemm.hip leaves contraction to the compiler, csrc/gemm8.hip spells its
roundings out). Derived, not measured; validated by the CPU emulations of
tests/test_gemm_oracle.py. Nothing is excused.

Buffers (Plane). Every output is a view with ldc > N into a larger buffer prefilled with the
sentinel NaN: guard rows before and after, guard columns on both sides, payload offset 16-B
aligned, ldc % 8 == 0. After a launch every band is bit-identical to the sentinel and no payload
element still holds it (epi 2: the payload starts as c0). Every operand is likewise a view into a
sentinel-filled buffer (ld = extent + 8..64, poisoned rows before the first and after the last):
the row gaps, the rows past M / N, the k-rows past K or Kl of a column-mode operand and the
columns M..Ml. Any such value that enters a product shows up as a NaN in the payload.
"""
import functools
import math

import torch

from conv_cases import EPS, SENT16, SENT32, Mismatch, _coords, hulp, old_ratio, rne_bf16  # noqa: F401

F64 = torch.float64
BFT, F32, F8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
SENT8 = 0x7F                    # e4m3fn NaN
WORST = {}                      # kernel / output type -> worst err/tol seen (profiles/gemm_oracle_coverage.md)
LAUNCHED = set()                # kernel instantiations the GPU file launched
BMN = ("b", "m", "n")

# cfg -> (BM, BN) of csrc/gemm.hip (ds2_gemm_tile; asserted against the extension on the GPU)
TILES = {0: (256, 256), 1: (128, 256), 2: (256, 128), 3: (128, 128), 4: (128, 128), 5: (128, 128),
         6: (256, 256), 7: (128, 256), 8: (256, 128)}
PERSISTENT = (6, 7, 8)

# scalars: (alpha, alpha_dev, alpha_dev2)
SCAL = {"A": (0.5, 0.25, 8.0),
        "B": (0.75, float(torch.tensor(1.3, dtype=F32)), float(torch.tensor(0.7, dtype=F32)))}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------ guard bands
class Plane:
    """A [batch, rows, cols] (batch 1: [rows, cols]) view `t` with ld > cols inside a buffer
    [batch, before + rows + after, ld] prefilled with a sentinel bit pattern."""

    def __init__(self, batch, rows, cols, dtype, device, pad=8, before=2, after=3):
        unit = 16 if dtype == F8 else 8
        self.ity, self.sent = {BFT: (torch.int16, SENT16), F32: (torch.int32, SENT32), F8: (torch.uint8, SENT8)}[dtype]
        self.left = unit
        self.ld = cdiv(self.left + cols + max(pad - self.left, 1), unit) * unit
        self.batch, self.rows, self.cols, self.before = batch, rows, cols, before
        self.buf = torch.empty(batch, before + rows + after, self.ld, dtype=dtype, device=device)
        self.buf.view(self.ity).fill_(self.sent)
        v = self.buf[:, before:before + rows, self.left:self.left + cols]
        self.t = v if batch > 1 else v[0]
        assert self.t.data_ptr() % 16 == 0 and self.ld % unit == 0 and self.ld > cols

    def put(self, x):
        """x: [batch, rows', cols'] values; written to the top-left corner of the payload, the rest
        of it stays poison (a column-mode operand's columns M..Ml)"""
        x = x if x.dim() == 3 else x.unsqueeze(0)
        v = self.buf[:, self.before:self.before + x.shape[1], self.left:self.left + x.shape[2]]
        if self.buf.dtype == F8:
            v.view(torch.uint8).copy_(x.view(torch.uint8))
        else:
            v.copy_(x.to(self.buf.dtype))
        return self

    def vec(self):
        """a 1-row plane as a contiguous vector"""
        return self.buf[0, self.before, self.left:self.left + self.cols]

    def verify(self, name, written=True, initial=None):
        """bands untouched; payload fully overwritten, or (written=False) bit-identical to what it
        held: the sentinel, or `initial`"""
        iv = self.buf.view(self.ity).cpu()
        pay = iv[:, self.before:self.before + self.rows, self.left:self.left + self.cols]
        band = iv != self.sent
        band[:, self.before:self.before + self.rows, self.left:self.left + self.cols] = False
        if bool(band.any()):
            i = int(band.reshape(-1).to(torch.uint8).argmax())
            c = _coords(i, iv.shape, ("b", "row", "col"))
            r, cc = c["row"] - self.before, c["col"] - self.left
            where = ("above row 0" if r < 0 else "past the last row" if r >= self.rows else
                     "left of column 0" if cc < 0 else "right of the last column")
            raise Mismatch("%s: %d guard-band elements were written; first %s at b=%d, m=%d, n=%d" % (
                name, int(band.sum()), where, c["b"], r, cc), dict(b=c["b"], m=r, n=cc))
        if initial is not None and not written:
            same = torch.equal(pay, initial.to(self.buf.dtype).view(self.ity).reshape(pay.shape))
            assert same, "%s: the payload changed, nothing should have been written" % name
            return
        left = pay == self.sent
        n = int(left.sum())
        if written and n:
            c = _coords(int(left.reshape(-1).to(torch.uint8).argmax()), pay.shape, BMN)
            raise Mismatch("%s: %d of %d payload elements were never written; first at b=%d, m=%d, n=%d" % (
                name, n, pay.numel(), c["b"], c["m"], c["n"]), c)
        if not written:
            assert n == pay.numel(), "%s: %d payload elements were written, none should be" % (name, pay.numel() - n)


# ------------------------------------------------------------------------------ inputs
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ints123(g, shape):
    return (torch.randint(1, 4, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).to(F64)


def _bf(t):
    return t.to(F32).to(BFT).to(F64)


def _f32(t):
    return t.to(F32).to(F64)


def shape_of(M, N, K, a_col=False, b_col=False, batch=1, Ml=0, Kl=0, fp8=False):
    return (M, N, K, bool(a_col), bool(b_col), batch, Ml, Kl, bool(fp8))


@functools.lru_cache(maxsize=4)
def problem(fam, sh):
    """Logical operands of one shape (fp64 CPU tensors of bf16- / e4m3-exact values): A [b,M,K],
    B [b,N,K], bias [N] (bf16-exact), c0 [b,M,N] (fp32-exact), P = A B^T and Pabs = |A| |B|^T.
    Cached: the launches of a shape share them and must not modify them."""
    M, N, K, a_col, b_col, batch, Ml, Kl, fp8 = sh
    g = _g(1000003 * M + 1009 * N + 7 * K + 3 * batch + (0 if fam == "A" else 5) + (11 if fp8 else 0))
    d = dict(fam=fam, sh=sh, sA=1.0, sB=1.0)
    has_c0 = batch * M * N <= 1 << 21          # the seam shapes never accumulate: no c0
    if fam == "A":
        A, B = _ints123(g, (batch, M, K)), _ints123(g, (batch, N, K))
        sgn = (2 * torch.randint(0, 2, (N,), generator=g) - 1).to(F64)
        small = torch.randint(1, 7, (N,), generator=g).to(F64)
        big = 256.0 + 2 * torch.randint(0, 128, (N,), generator=g).to(F64)
        d["bias"] = sgn * torch.where(torch.arange(N) % 3 == 0, big, small)
        d["c0"] = torch.randint(-7, 8, (batch, M, N), generator=g).to(F64) if has_c0 else None
    else:
        A = torch.randn(batch, M, K, generator=g, dtype=F64)
        B = 0.05 * torch.randn(batch, N, K, generator=g, dtype=F64) + 0.01
        if fp8:
            # per-tensor scales of a quantiser (amax -> 448), folded into alpha_dev / alpha_dev2
            d["sA"] = float(_f32(A.abs().max() / 448.0))
            d["sB"] = float(_f32(B.abs().max() / 448.0))
            A = (A / d["sA"]).to(F32).to(F8).to(F64)
            B = (B / d["sB"]).to(F32).to(F8).to(F64)
        else:
            A, B = _bf(A), _bf(B)
        d["bias"] = _bf(torch.randn(N, generator=g, dtype=F64))
        d["c0"] = _f32(torch.randn(batch, M, N, generator=g, dtype=F64)) if has_c0 else None
    if Kl:                                   # the Kl contract: zeros meet the k-rows never loaded
        (A if b_col else B)[:, :, Kl:] = 0.0
    d["A"], d["B"] = A, B
    d["P"] = A @ B.transpose(1, 2)
    d["Pabs"] = A.abs() @ B.abs().transpose(1, 2)
    return d


def scalars(d, spec):
    """(alpha, alpha_dev or None, alpha_dev2 or None) of a launch, as fp32-exact floats. fp8
    family B: the device scalars are the quantiser's scales."""
    al, a1, a2 = SCAL[d["fam"]]
    al = spec.get("alpha", al)
    if d["sh"][8] and d["fam"] == "B":
        a1, a2 = d["sA"], d["sB"]
    return al, (a1 if spec.get("adev") else None), (a2 if spec.get("adev2") else None)


def expected(d, spec):
    """fp64 result r [b,M,N] and S_abs of a launch"""
    al, a1, a2 = scalars(d, spec)
    s = al * (a1 if a1 is not None else 1.0) * (a2 if a2 is not None else 1.0)
    r, S = s * d["P"], abs(s) * d["Pabs"]
    if spec.get("bias"):
        r, S = r + d["bias"], S + d["bias"].abs()
    if spec["epi"] == 2:
        r, S = r + d["c0"], S + d["c0"].abs()
    return r, S


def tolerance(r, S, K, slices, bf16):
    dd = (2 * (K + slices) + 8) * EPS * S
    return dd + hulp(r.abs() + dd) if bf16 else dd


def preconditions(d):
    """What family A promises, asserted from the operands (CPU)."""
    if d["fam"] != "A":
        return
    A, B = d["A"], d["B"]
    Kl = d["sh"][7]
    for t in (A, B):
        live = t if not Kl else t[:, :, :Kl]
        assert bool(((live.abs() >= 1) & (live.abs() <= 3) & (live == live.round())).all())
    for spec in (dict(epi=0, bias=True, adev=True, adev2=True), dict(epi=2, adev=True), dict(epi=1)):
        r, S = expected(d, spec)
        assert float(S.max()) < 2.0 ** 24
        assert torch.equal(r.to(F32).to(F64), r)


def stored(d, device, pad_a=24, pad_b=40):
    """The operands as the kernel reads them: guard-banded planes of A ([M,K] or [Kx,Mx]) and
    B ([N,K] or [Kx,Nx]), the bias [N] and the device scalars' values."""
    M, N, K, a_col, b_col, batch, Ml, Kl, fp8 = d["sh"]
    dt = F8 if fp8 else BFT
    Kx, Mx = (Kl or K), (Ml or M)

    def one(X, col, ext, pad):
        if col:
            p = Plane(batch, Kx, ext, dt, device, pad)
            return p.put(X[:, :, :Kx].transpose(1, 2).to(F32).to(dt))
        return Plane(batch, X.shape[1], K, dt, device, pad).put(X.to(F32).to(dt))

    pa, pb = one(d["A"], a_col, Mx, pad_a), one(d["B"], b_col, N, pad_b)
    bias = Plane(1, 1, N, BFT, device, 16).put(d["bias"].reshape(1, 1, N))
    return pa, pb, bias


def output(d, spec, device, pad=16):
    M, N, _, _, _, batch = d["sh"][:6]
    p = Plane(batch, M, N, BFT if spec["epi"] == 0 else F32, device, pad)
    if spec["epi"] == 2:
        p.put(d["c0"])
    return p


# ------------------------------------------------------------------------------ checker
def check(name, got, want, tol, kernel=None):
    """Per element |got - want| <= tol (a non-finite got fails). Names the worst element."""
    got = got.detach().to("cpu").to(F64).reshape(want.shape)
    err = (got - want).abs_()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = err / tol.clamp_min(1e-300)
    ratio = torch.where(err > 0, ratio, torch.zeros_like(ratio))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if kernel is not None and math.isfinite(worst):
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        c = _coords(i, want.shape, BMN)
        raise Mismatch("%s: %d of %d elements beyond tolerance; worst at b=%d, m=%d, n=%d: got %r want %r err %.3e tol %.3e" % (
            name, int((ratio > 1).sum()), ratio.numel(), c["b"], c["m"], c["n"], got.reshape(-1)[i].item(),
            want.reshape(-1)[i].item(), err.reshape(-1)[i].item(), tol.reshape(-1)[i].item()), c)
    return worst


def check_equal(name, got, want):
    """Family A: got equals the oracle bit for bit (fp32) or RNE-bf16 of it"""
    got = got.detach().to("cpu").reshape(want.shape)
    w = rne_bf16(want) if got.dtype == BFT else want.to(F32)
    if got.dtype != BFT:
        assert torch.equal(w.to(F64), want), "%s: the expected value is not exact in fp32" % name
    if torch.equal(got, w):
        return
    bad = ~(got == w)
    i = int(bad.reshape(-1).to(torch.uint8).argmax())
    c = _coords(i, w.shape, BMN)
    raise Mismatch("%s: %d of %d elements differ; first at b=%d, m=%d, n=%d: got %r want %r" % (
        name, int(bad.sum()), bad.numel(), c["b"], c["m"], c["n"], got.reshape(-1)[i].item(), w.reshape(-1)[i].item()), c)


def spec_name(spec):
    s = spec["kern"] + ("" if spec.get("cfg") is None else " cfg%d" % spec["cfg"]) + " epi%d" % spec["epi"]
    for k in ("bias", "adev", "adev2", "ext"):
        s += " " + k if spec.get(k) else ""
    if spec.get("S", 1) > 1 or spec.get("req"):
        s += " S=%d(req %d)" % (spec.get("S", 1), spec.get("req", spec.get("S", 1)))
    if spec.get("max_grid"):
        s += " max_grid=%d" % spec["max_grid"]
    return s


def case_name(d, spec):
    return "%s %s %s" % (spec_name(spec), d["fam"], ident(d["sh"]))


def verify(d, spec, got, kernel=None):
    """One launch's payload against the oracle: family A bitwise, family B within the tolerance"""
    name = case_name(d, spec)
    r, S = expected(d, spec)
    if d["fam"] == "A":
        check_equal(name, got, r)
        return 0.0
    bf16 = spec["epi"] == 0
    kernel = kernel or "%s %s" % (spec["kern"], "bf16" if bf16 else "fp32")
    return check(name, got, r, tolerance(r, S, d["sh"][2], spec.get("S", 1), bf16), kernel)


# ------------------------------------------------------------------------------ case tables
def ident(sh):
    M, N, K, a_col, b_col, batch, Ml, Kl, fp8 = sh
    s = "%s%s-%dx%dx%d" % ("c" if a_col else "r", "c" if b_col else "r", M, N, K)
    s += "-b%d" % batch if batch > 1 else ""
    s += "-Ml%d" % Ml if Ml else ""
    s += "-Kl%d" % Kl if Kl else ""
    return s + ("-fp8" if fp8 else "")


LAYOUTS = ((False, False), (False, True), (True, False), (True, True))

# ---- csrc/gemm.hip. M, N: every residue asked for of BM, BN in {128, 256} at once: 257, 271, 272,
# 273, 511 are 1, 15, 16, 17, BM-1 of both tile heights; 260, 268, 276, 508 are 4, 12, 20, BN-4 of
# both widths; a column-mode side keeps its multiple of 8: 264 (8) and 504 (BN-8); 5 / 4 / 8: tiny.
G_M, G_N = (257, 271, 272, 273, 511, 5), (260, 268, 276, 508, 4)
G_MC, G_NC = (264, 504, 8), (264, 504, 8)
G_K = (8, 24, 32, 40, 64, 72, 96, 104, 128, 136, 192, 200)
G_KCC = G_K + (5, 63, 65)


def _gemm_shapes():
    out = []
    for a_col, b_col in LAYOUTS:
        ks = G_KCC if (a_col and b_col) else G_K
        ms, ns = (G_MC if a_col else G_M), (G_NC if b_col else G_N)
        for i, K in enumerate(ks):
            out.append(shape_of(ms[i % len(ms)], ns[(i + i // len(ns)) % len(ns)], K, a_col, b_col))
    return out


GEMM_SHAPES = _gemm_shapes()
# batch 3 (distinct batch strides: the planes' ld and row counts differ per operand)
GEMM_BATCH = [shape_of(145, 132, 72, a, b, 3) if not (a or b) else shape_of(144, 136, 72, a, b, 3) for a, b in LAYOUTS]
# nine m-tiles, the ntm % 8 == 1 group: (configurations, shape)
GEMM_NINE = [((3, 7), shape_of(8 * 128 + 17, 132, 40)), ((0, 8), shape_of(8 * 256 + 17, 132, 40))]
# as ops/ctc.py calls it: dh = G W (row A / col B, Kl) and dW = G^T h (col-col, Ml), alpha_dev
GEMM_CTC = [shape_of(145, 264, 32, False, True, Kl=29), shape_of(29, 264, 72, True, True, Ml=32),
            shape_of(29, 136, 200, True, True, 3, Ml=32)]


def gemm_launches(sh, cfgs=range(9)):
    """every configuration x epi 0 (without / with bias), 1, 2; alpha_dev on half of them.
    Configurations 6..8 refuse epi 2 (asserted by the GPU file)."""
    Kl, Ml = sh[7], sh[6]
    out = []
    for cfg in cfgs:
        for epi, bias, adev in ((0, False, False), (0, True, True), (1, False, False), (2, False, True)):
            if cfg in PERSISTENT and epi == 2:
                continue
            if Kl and epi != 0 or Ml and epi == 0:
                continue
            out.append(dict(kern="gemm", cfg=cfg, epi=epi, bias=bias, adev=adev or bool(Kl or Ml)))
    return out


def seam_shapes(cus):
    """The persistent seam: more tiles than workgroups, so a workgroup issues its next tile's
    prologue under this tile's stores. Two n-tiles (the second ragged), cus // 2 + 1 full
    m-tiles and a ragged one; K = 40 and 136; row-row and row-col."""
    out = []
    for cfg in PERSISTENT:
        bm, bn = TILES[cfg]
        M, N = (cus // 2 + 1) * bm + 17, bn + 72
        assert cdiv(M, bm) * cdiv(N, bn) > cus
        for K in (40, 136):
            for b_col in (False, True):
                out.append((cfg, shape_of(M, N, K, False, b_col)))
    return out


# ---- csrc/gemm8.hip, bf16. A column-mode side takes the neighbouring multiples of 8.
G8_M, G8_N = (1, 127, 128, 129, 255, 256, 257, 300), (4, 124, 128, 132, 252, 256, 260)
G8_MC, G8_NC = (8, 120, 128, 136, 248, 256, 264, 304), (8, 120, 128, 136, 248, 256, 264)
G8_K, G8_KCC = (32, 64, 96, 128, 160, 192, 224, 288), (1, 5, 8, 63, 64, 65, 100, 129)


def _gemm8_shapes():
    out = []
    for a_col, b_col in LAYOUTS:
        ks = G8_KCC if (a_col and b_col) else G8_K
        ms, ns = (G8_MC if a_col else G8_M), (G8_NC if b_col else G8_N)
        for i in range(8):
            out.append(shape_of(ms[i], ns[(i + 3) % 7], ks[(3 * i) % 8], a_col, b_col))
        out.append(shape_of(ms[7], ns[6], ks[7], a_col, b_col))      # 2 x 2 tiles, the longest K
    return out


GEMM8_SHAPES = _gemm8_shapes()
G8_VARIANTS = ((0, True, True, True), (0, False, False, False), (1, False, True, False), (2, False, False, True))


def slices_of(K, req, fp8=False):
    """k-slices ds2_gemm8 runs for a request (no empty slice) and the k-tiles of each"""
    nkt = cdiv(K * (1 if fp8 else 2), 128)
    kps = cdiv(nkt, req)
    S = cdiv(nkt, kps)
    return S, [min(kps, nkt - s * kps) for s in range(S)]


def gemm8_launches(sh):
    return [dict(kern="gemm8", epi=e, bias=b, adev=a1, adev2=a2, S=1, req=1) for e, b, a1, a2 in G8_VARIANTS]


# forced plans: (shape, requested S). K = 96, S = 5 runs as 2 slices; 160 / 2: the ragged k-tile
# alone in the last slice; 288 / 2: 3 + 2 k-tiles (odd and even, the last shorter); 288 / 3: 2 + 2 +
# 1; 224 / 4: one k-tile each; column-column 129 / 2 and 100 / 2
GEMM8_SPLIT = [(shape_of(300, 260, 96), 5), (shape_of(257, 264, 160, False, True), 2),
               (shape_of(264, 132, 288, True, False), 2), (shape_of(129, 252, 288), 3),
               (shape_of(255, 124, 224), 4), (shape_of(136, 264, 129, True, True), 2),
               (shape_of(304, 8, 100, True, True), 2)]


def split_launches(sh, req):
    S, _ = slices_of(sh[2], req, sh[8])
    out = []
    for ext in (False, True):
        for e, b, a1, a2 in (((0, True, True, True), (1, False, True, False)) if sh[8] else G8_VARIANTS[:1] + G8_VARIANTS[2:]):
            out.append(dict(kern="gemm8", epi=e, bias=b, adev=a1, adev2=a2, S=S, req=req, ext=ext))
    return out


# max_grid = 8: 12 units (3 members x 4 tiles: the workgroup loop), 1 unit (idle workgroups)
GEMM8_MAXGRID = [shape_of(300, 260, 64, batch=3), shape_of(127, 124, 64)]
GEMM8_BATCH = [shape_of(129, 132, 96, batch=3), shape_of(136, 136, 96, False, True, 3),
               shape_of(136, 132, 96, True, False, 3), shape_of(136, 136, 65, True, True, 3),
               shape_of(17, 12, 32, batch=24), shape_of(16, 8, 5, True, True, 24)]
GEMM8_17 = shape_of(16 * 256 + 1, 132, 32)           # 17 m-tiles x 1 n-tile: the short last group
# grouped launches: (M, N, K, requested S, epi), column-column
GROUP_MIXED = [(136, 264, 129, 2, 1), (8, 8, 5, 1, 2), (304, 136, 288, 3, 2), (264, 504, 64, 1, 1), (120, 248, 100, 2, 2)]
GROUP_MANY = [(8 * (i % 5 + 1), 16, 40 + i, 1, 1) for i in range(25)]

# ---- csrc/gemm8.hip, fp8 (row mode, K % 128 == 0)
FP8_SHAPES = [shape_of(m, n, (128, 256, 384)[i % 3], fp8=True) for i, (m, n) in enumerate(
    [(1, 4), (127, 124), (128, 128), (129, 132), (255, 252), (256, 256), (257, 260), (300, 132)])]
FP8_SPLIT = [(shape_of(255, 252, 256, fp8=True), 2), (shape_of(300, 132, 384, fp8=True), 2)]


def fp8_launches(sh):
    return [dict(kern="gemm8", epi=0, bias=True, adev=True, adev2=True, S=1, req=1),
            dict(kern="gemm8", epi=1, adev=True, adev2=True, S=1, req=1)]


# ---- ops/gemm.py matmul: (a transposed view, b transposed view, M, N, K, fp32 out, accumulate,
# bias, splits, max_grid). a [M,K] is unit-stride K unless transposed, b [K,N] unit-stride N.
ROUTING = [(ta, tb, 304, 264, K, f32o, acc, bias, sp, mg)
           for ta, tb in ((False, True), (False, False), (True, True), (True, False))
           for K, f32o, acc, bias, sp, mg in ((96, False, False, True, None, 0), (96, True, False, False, 2, 0),
                                              (72, True, True, False, None, 8), (72, False, False, False, None, 0))]


def all_launches():
    """(shape, spec) of every table entry with a fixed shape: what the CPU emulations must pass"""
    out = []
    for sh in GEMM_SHAPES + GEMM_BATCH + GEMM_CTC:
        out += [(sh, s) for s in gemm_launches(sh)]
    for cfgs, sh in GEMM_NINE:
        out += [(sh, s) for s in gemm_launches(sh, cfgs)]
    for sh in GEMM8_SHAPES + GEMM8_BATCH + GEMM8_MAXGRID + [GEMM8_17]:
        out += [(sh, s) for s in gemm8_launches(sh)]
    for sh, req in GEMM8_SPLIT + FP8_SPLIT:
        out += [(sh, s) for s in split_launches(sh, req)]
    for sh in FP8_SHAPES:
        out += [(sh, s) for s in fp8_launches(sh)]
    return out


def coverage():
    """What the tables reach, computed from them (asserted by tests/test_gemm_oracle.py)"""
    c = dict(gemm={}, gemm8={})
    for cfg, (bm, bn) in TILES.items():
        e = dict(mrem=set(), nrem=set(), mrem_col=set(), nrem_col=set(), small_m=False, n4=False, two_by_two=False,
                 layouts=set(), epis=set())
        for sh in GEMM_SHAPES:
            M, N, K, a_col, b_col = sh[:5]
            (e["mrem_col"] if a_col else e["mrem"]).add(M % bm)
            (e["nrem_col"] if b_col else e["nrem"]).add(N % bn)
            e["small_m"] |= M < 16
            e["n4"] |= N == 4
            e["two_by_two"] |= M > bm and N > bn
            e["layouts"].add((a_col, b_col))
            e["epis"] |= {(s["epi"], s["bias"]) for s in gemm_launches(sh, (cfg,))}
        c["gemm"][cfg] = e
    kt = lambda K: (cdiv(K, 64), "<32" if (K - 1) % 64 + 1 < 32 else "32" if (K - 1) % 64 + 1 == 32 else
                    "32..64" if (K - 1) % 64 + 1 < 64 else "64")
    c["gemm_k_row"] = {kt(sh[2]) for sh in GEMM_SHAPES if not (sh[3] and sh[4])}
    c["gemm_k_cc"] = {sh[2] for sh in GEMM_SHAPES if sh[3] and sh[4]}
    c["gemm_nine"] = {(cfg, cdiv(sh[0], TILES[cfg][0])) for cfgs, sh in GEMM_NINE for cfg in cfgs}
    c["gemm_ctc"] = {(sh[3], sh[4], sh[6], sh[7], s["epi"], s["adev"]) for sh in GEMM_CTC for s in gemm_launches(sh)}
    c["gemm_batch"] = {(sh[3], sh[4], sh[5]) for sh in GEMM_BATCH}
    g8 = c["gemm8"]
    g8["m_row"] = {sh[0] for sh in GEMM8_SHAPES if not sh[3]}
    g8["n_row"] = {sh[1] for sh in GEMM8_SHAPES if not sh[4]}
    g8["m_col"] = {sh[0] for sh in GEMM8_SHAPES if sh[3]}
    g8["n_col"] = {sh[1] for sh in GEMM8_SHAPES if sh[4]}
    g8["k_row"] = {sh[2] for sh in GEMM8_SHAPES if not (sh[3] and sh[4])}
    g8["k_cc"] = {sh[2] for sh in GEMM8_SHAPES if sh[3] and sh[4]}
    g8["layouts"] = {(sh[3], sh[4]) for sh in GEMM8_SHAPES}
    g8["splits"] = {(sh[2], req, ) + (tuple(slices_of(sh[2], req)[1]),) for sh, req in GEMM8_SPLIT}
    g8["maxgrid_units"] = sorted(cdiv(sh[0], 256) * cdiv(sh[1], 256) * sh[5] for sh in GEMM8_MAXGRID)
    g8["batches"] = {sh[5] for sh in GEMM8_BATCH}
    g8["m_tiles_17"] = (cdiv(GEMM8_17[0], 256), cdiv(GEMM8_17[1], 256), GEMM8_17[2])
    g8["group"] = dict(Ms={m[0] for m in GROUP_MIXED}, Ns={m[1] for m in GROUP_MIXED}, Ks={m[2] for m in GROUP_MIXED},
                       S={slices_of(m[2], m[3])[0] for m in GROUP_MIXED}, epis={m[4] for m in GROUP_MIXED},
                       many=len(GROUP_MANY))
    g8["fp8_k"] = {sh[2] for sh in FP8_SHAPES}
    g8["fp8_mn"] = {(sh[0], sh[1]) for sh in FP8_SHAPES}
    g8["fp8_splits"] = {tuple(slices_of(sh[2], req, True)[1]) for sh, req in FP8_SPLIT}
    return c
