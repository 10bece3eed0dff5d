"""fp64 oracle, per-element checker and case grid of the lookahead convolution kernels
(csrc/lookahead.hip). Pure torch, device-agnostic, does not import the extension. The guard
bands, the exact bf16 half-ulp and the per-element checker are those of tests/conv_cases.py.

Definition. h, r, dr, dh [T, B, H] time-major, w [H, tau+1], valid(t, b) = t < min(lens[b], T):

    r[t,b,i]  = valid(t,b) ? sum_{j=0..tau, valid(t+j,b)} w[i,j] h[t+j,b,i] : 0
    dh[t,b,i] = valid(t,b) ? sum_{j=0..min(tau,t)} w[i,j] dr[t-j,b,i]       : 0
    dw[i,j]   = sum_b sum_{t : valid(t+j,b)} dr[t,b,i] h[t+j,b,i]

h and dr are nonzero at invalid positions too: the kernels must not read them (h) or trust them
(dr). Invalid outputs must be exact zeros.

Family A, exact. h, dr and w are small integers, sparse enough that every sum of |terms| is
below 2^24 (asserted by preconditions()). fp32 accumulation is then exact in any order: r and
dh must torch.equal the RNE-bf16 value of the fp64 result, dw the fp64 result bit for bit. One
dropped, doubled or misplaced tap is visible.

Family B, random reals rounded to bf16 first. eps = 2^-24; S the same sum over absolute values;
K the number of terms actually summed for the element. A product of two bf16 values is exact in
fp32 and an FMA rounds once, so only the K - 1 additions round, each by at most eps times a
partial sum that S bounds (to (1 + eps)^K, which K eps S absorbs for K <= 2^12):
    r, dh (bf16):  d = K eps S,  tolerance d + hulp(|ref| + d)   (hulp: exact bf16 half-ulp)
    dw (fp32):     M eps S,  M <= T B its term count (any summation order or tree)
Derived, not measured; no element is excused. An element with K = 0 (an invalid position, a tap
no frame reaches) has tolerance 0.

Grid. tau in {1, 2, 7, 20, 31} x T in {1, 2, tau, tau+1, tau+2, 67, 130}, and for each (tau, T)
three (B, H) pairs that between them hold every B in {1, 3, 9} and every H in {8, 40, 800} (a
rotating Latin square, so each (B, H) pair meets every tau): 8 is one lane, 40 a partial wave,
800 the production width (more than one workgroup of columns in every kernel); T = 67 and 130
cross several time tiles of 8. EXTRA adds B = 33 and 35, which cross the 32 batch rows one
weight-gradient workgroup sums. lens are ragged and hold T, 1, a value inside the last window, 0
and a value above T where B has room.
"""
import functools

import torch

import conv_cases as CO

F64 = torch.float64
EPS = CO.EPS
WORST = {}                      # kernel -> worst err/tol seen (profiles/lookahead.md)
DIMS = ("t", "b", "i")

TAUS = (1, 2, 7, 20, 31)
BS = (1, 3, 9)
HS = (8, 40, 800)


def t_values(tau):
    return sorted({1, 2, tau, tau + 1, tau + 2, 67, 130})


def grid():
    out = []
    for a, tau in enumerate(TAUS):
        for c, T in enumerate(t_values(tau)):
            for k in range(3):
                out.append((tau, T, BS[k], HS[(k + a + c) % 3]))
    return out


GRID = grid()
EXTRA = [(7, 20, 33, 8), (20, 67, 35, 40)]
SMALL = [c for c in GRID if c[1] * c[2] * c[3] <= 3000]          # the CPU triple loop's share


def ident(c):
    return "tau%d-T%d-B%d-H%d" % tuple(c)


def case_lens(tau, T, B, g):
    """ragged lengths: T, 1, one inside the last window, 0, one above T, then random"""
    mid = max(1, T - (tau + 1) // 2)
    fixed = [T, 1, mid, 0, T + 3]
    if B == 1:
        return torch.tensor([mid if (tau + T) % 2 else T], dtype=torch.int32)
    rest = torch.randint(1, T + 1, (max(0, B - len(fixed)),), generator=g).tolist()
    return torch.tensor((fixed + rest)[:B], dtype=torch.int32)


def valid_mask(lens, T):
    L = lens.to(torch.long).clamp(min=0, max=T)
    return (torch.arange(T).unsqueeze(1) < L.unsqueeze(0)).unsqueeze(-1)          # [T, B, 1]


# ------------------------------------------------------------------------------ oracle (fp64)
def oracle(h, dr, w, lens):
    """(r, dh, dw) of the definition, in the dtype of the operands (fp64 here)."""
    T, B, H = h.shape
    taps = w.shape[1]
    m = valid_mask(lens, T).to(h.dtype)
    hm, dm = h * m, dr * m
    r, dh = torch.zeros_like(h), torch.zeros_like(h)
    dw = torch.zeros(H, taps, dtype=h.dtype)
    for j in range(min(taps, T)):
        r[:T - j] += w[:, j] * hm[j:]
        dh[j:] += w[:, j] * dm[:T - j]
        dw[:, j] = (dm[:T - j] * hm[j:]).sum((0, 1))
    return r * m, dh * m, dw


def loops(h, dr, w, lens):
    """the definition as literal loops (small shapes only)"""
    T, B, H = h.shape
    tau = w.shape[1] - 1
    L = [max(0, min(int(v), T)) for v in lens]
    r, dh = torch.zeros_like(h), torch.zeros_like(h)
    dw = torch.zeros(H, tau + 1, dtype=h.dtype)
    for b in range(B):
        for t in range(L[b]):
            for j in range(tau + 1):
                if t + j < L[b]:
                    r[t, b] += w[:, j] * h[t + j, b]
                    dw[:, j] += dr[t, b] * h[t + j, b]
                if j <= t:
                    dh[t, b] += w[:, j] * dr[t - j, b]
    return r, dh, dw


def term_counts(tau, T, lens):
    """K of r and dh [T, B, 1] and M of dw [tau+1]"""
    L = lens.to(torch.long).clamp(min=0, max=T).unsqueeze(0)          # [1, B]
    t = torch.arange(T).unsqueeze(1)                                  # [T, 1]
    v = t < L
    kr = torch.where(v, (L - t).clamp(max=tau + 1), torch.zeros_like(L - t))
    kd = torch.where(v, (t + 1).clamp(max=tau + 1).expand_as(v), torch.zeros_like(L - t))
    j = torch.arange(tau + 1).unsqueeze(1)
    md = (L - j).clamp(min=0).sum(1)
    return kr.unsqueeze(-1).to(F64), kd.unsqueeze(-1).to(F64), md.to(F64)


# ------------------------------------------------------------------------------ inputs
def _bf(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


@functools.lru_cache(maxsize=4)
def make(fam, tau, T, B, H):
    """Operands (fp64 CPU tensors holding bf16-exact values), the oracle's results, the sums over
    absolute values and the term counts. Cached: the tests share them and must not modify them."""
    g = torch.Generator().manual_seed(7919 * tau + 104729 * T + 1299709 * B + H + (0 if fam == "A" else 3))
    lens = case_lens(tau, T, B, g)
    if fam == "A":
        ints = lambda shape, lo, hi, dens: (torch.randint(lo, hi + 1, shape, generator=g).to(F64) *
                                            (torch.rand(shape, generator=g) < dens))
        h, dr, w = ints((T, B, H), -8, 8, 0.5), ints((T, B, H), -8, 8, 0.5), ints((H, tau + 1), -4, 4, 0.75)
    else:
        rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
        h, dr, w = _bf(rn(T, B, H)), _bf(rn(T, B, H)), _bf(rn(H, tau + 1) * (tau + 1) ** -0.5)
    r, dh, dw = oracle(h, dr, w, lens)
    Sr, Sd, Sw = oracle(h.abs(), dr.abs(), w.abs(), lens)
    Kr, Kd, Mw = term_counts(tau, T, lens)
    return dict(fam=fam, tau=tau, T=T, B=B, H=H, lens=lens, h=h, dr=dr, w=w, r=r, dh=dh, dw=dw, Sr=Sr, Sd=Sd, Sw=Sw,
                Kr=Kr, Kd=Kd, Mw=Mw, valid=valid_mask(lens, T))


def preconditions(d):
    """What the families promise, asserted from the operands (CPU)."""
    for k in ("h", "dr", "w"):
        assert torch.equal(_bf(d[k]), d[k]), k + " is not exact in bf16"
    inv = ~d["valid"].expand_as(d["h"])
    if inv.any():                       # the mask is exercised: data sits where nothing may read it
        assert d["h"][inv].abs().sum() > 0 and d["dr"][inv].abs().sum() > 0
        assert float(d["r"][inv].abs().max()) == 0.0 and float(d["dh"][inv].abs().max()) == 0.0
    assert float(d["Mw"].max()) <= d["T"] * d["B"]
    if d["fam"] == "A":
        lim = 2.0 ** 24
        assert d["Sr"].max() < lim and d["Sd"].max() < lim and d["Sw"].max() < lim
        for k in ("r", "dh", "dw"):
            assert torch.equal(d[k], d[k].round())


# ------------------------------------------------------------------------------ verifiers
def _name(kernel, d):
    return "%s %s tau=%d T=%d B=%d H=%d" % (kernel, d["fam"], d["tau"], d["T"], d["B"], d["H"])


def _verify_act(kernel, d, got, want, S, K):
    name = _name(kernel, d)
    inv = ~d["valid"].expand_as(want)
    g = got.detach().cpu()
    assert bool((g[inv] == 0).all()), "%s: nonzero output at an invalid position" % name
    if d["fam"] == "A":
        CO.check_equal(name, got, CO.rne_bf16(want).to(F64), DIMS)
    else:
        dd = K * EPS * S
        worst = CO.check(name, got, want, dd + CO.hulp(want.abs() + dd), DIMS)
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)


def verify_fwd(d, r, kernel="lookahead_fwd"):
    _verify_act(kernel, d, r, d["r"], d["Sr"], d["Kr"])


def verify_bwd_data(d, dh, kernel="lookahead_bwd_data"):
    _verify_act(kernel, d, dh, d["dh"], d["Sd"], d["Kd"])


def verify_bwd_weight(d, dw, kernel="lookahead_bwd_weight"):
    name = _name(kernel, d)
    if d["fam"] == "A":
        CO.check_equal(name, dw, d["dw"], ("i", "j"))
    else:
        worst = CO.check(name, dw, d["dw"], d["Mw"].unsqueeze(0) * EPS * d["Sw"], ("i", "j"))
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
