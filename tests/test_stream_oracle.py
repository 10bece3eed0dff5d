"""The oracles and drivers of tests/stream_cases.py, checked on the CPU:

  * the case tables keep their edges (coverage());
  * Emu, a step-by-step fp32 emulation of every kernel and of the host checks of its binding
    (torch fp32 op by op, an fma through fp64, the reductions in the kernels' order), passes every
    driver on every table entry: the bounds are not too tight. The worst err/tol per kernel is
    printed (run with -s) for profiles/stream_oracle_coverage.md;
  * each planted error, an Emu with one step changed, is caught by the drivers.
"""
import pytest
import torch

import stream_cases as SC
from stream_cases import BFT, F32, F64, F8, I16, I32, U8

DEV = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(SC.WORST.items()):
        print("STREAMEMU %-28s worst err/tol %.3f" % (k, v))
    for k, v in sorted(SC.COUNTS.items()):
        print("STREAMCOUNT %-20s %d" % (k, v))


# ------------------------------------------------------------------------------ emulation
def _t(x):
    return torch.tensor(x, dtype=F32)


def _fma(a, b, c):
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _ext(t, k):
    """the n + k elements starting where the 1-D view t starts (a store past the end)"""
    return torch.as_strided(t, (t.numel() + k,), (1,), t.storage_offset())


def _need(ok, msg):
    if not ok:
        raise RuntimeError(msg)


def _aligned(t, a):
    return t.data_ptr() % a == 0


class Emu:
    def __init__(self, mut=None):
        self.mut = mut

    # ---- optim.hip
    def _adam_check(self, p, g, m, v, ema, p16, hyper):
        n = p.numel()
        for x in (p, g, m, v):
            _need(x.is_contiguous() and x.dtype == F32 and x.numel() == n and _aligned(x, 16), "fp32 arrays of n, 16-B aligned")
        if ema is not None:
            _need(ema.is_contiguous() and ema.dtype == F32 and ema.numel() == n and _aligned(ema, 16), "ema")
        if p16 is not None:
            _need(p16.is_contiguous() and p16.dtype == BFT and p16.numel() == n and _aligned(p16, 8), "p16")
        if hyper is not None:
            _need(hyper.dtype == F32 and hyper.numel() >= 2, "hyper")

    def _adam(self, idx, p, g, m, v, ema, p16, lr, b1, b2, eps, gs, keep, hyper):
        """adam1 / ema1 (csrc/common.h) on the elements idx (a slice or an index tensor)"""
        if hyper is not None and self.mut != "hyper":
            lr, keep = float(hyper[0]), float(hyper[1])
        lr, b1, b2, eps, gs, keep = (_t(x) for x in (lr, b1, b2, eps, gs, keep))
        p0 = p[idx].clone()
        gj = g[idx] * gs
        m1 = _fma(b1, m[idx], (1.0 - b1) * gj)
        v1 = _fma(b2, v[idx], ((1.0 - b2) * gj) * gj)
        p1 = _fma(-lr, m1 / (v1.sqrt() + eps), p0)
        p[idx], m[idx], v[idx] = p1, m1, v1
        if ema is not None:
            src = p0 if self.mut == "ema old p" else p1
            ema[idx] = _fma(keep, ema[idx] - src, src)
        if p16 is not None:
            if self.mut == "p16 truncated":
                p16[idx] = (p1.view(I32) >> 16).to(I16).view(BFT)
            else:
                p16[idx] = p1.to(BFT)

    def adam_ema(self, p, g, m, v, ema, p16, lr_t, b1, b2, eps, gscale, ema_keep, skip, max_grid, hyper=None, lds_reserve=0):
        _need(0 <= lds_reserve <= 65536, "lds_reserve")
        self._adam_check(p, g, m, v, ema, p16, hyper)
        if skip is not None:
            _need(skip.dtype == I32 and skip.numel() >= 1, "skip")
            if int(skip[0]) and self.mut != "skip ignored":
                return
        n = p.numel()
        arrs = [p, g, m, v, ema, p16]
        if self.mut == "tail dropped":
            n = n // 4 * 4
        if self.mut == "group past the end" and n // 4 > 0:
            arrs = [None if x is None else _ext(x, 4) for x in arrs]
            n = n // 4 * 4 + 4
        if n:
            self._adam(slice(0, n), *arrs, lr_t, b1, b2, eps, gscale, ema_keep, hyper)

    def adam_ema_ranges(self, p, g, m, v, ema, p16, lohi, lr_t, b1, b2, eps, gscale, ema_keep, hyper=None):
        self._adam_check(p, g, m, v, ema, p16, hyper)
        n = p.numel()
        _need(len(lohi) % 2 == 0 and all(0 <= x <= n for x in lohi), "pairs inside the arena")
        rs = list(zip(lohi[::2], lohi[1::2]))
        srt = sorted(r for r in rs if r[1] > r[0])
        _need(all(a[1] <= b[0] for a, b in zip(srt, srt[1:])), "ranges overlap")
        _need(len(rs) <= 64 and all(lo % 4 == 0 and hi % 4 == 0 and hi >= lo for lo, hi in rs), "<= 64 ranges on multiples of 4")
        mask = torch.zeros(n, dtype=torch.bool)
        for lo, hi in rs:
            mask[lo:hi + (4 if self.mut == "range runs on" and hi > lo and hi + 4 <= n else 0)] = True
        idx = mask.nonzero().flatten()
        if idx.numel():
            self._adam(idx, p, g, m, v, ema, p16, lr_t, b1, b2, eps, gscale, ema_keep, hyper)

    def grad_norm_blocks(self, n):
        return SC.gn_blocks(n)

    def grad_norm(self, g, gscale, part, bad):
        _need(g.dtype == F32 and g.is_contiguous(), "g")
        _need(part.dtype == F32 and part.numel() >= 1 and part.is_contiguous(), "part")
        _need(bad.dtype == I32 and bad.numel() == 1, "bad")
        n, nb = g.numel(), part.numel()
        x = g * _t(gscale)
        seen = x[:-1] if self.mut == "flag skips the last element" else x
        if not bool(torch.isfinite(seen).all()):
            bad[0] = int(bad[0]) | 1
        L = SC.cdiv(n, 256 * nb)
        xp = torch.zeros(L * nb * 256, dtype=F32)
        xp[:n] = x
        xp = xp.view(L, nb, 256)
        s = torch.zeros(nb, 256, dtype=F32)
        for k in range(L):
            s = s + xp[k] * xp[k]
        s = s.view(nb, 4, 64)
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ o]
        t = torch.zeros(nb, dtype=F32)
        for w in range(3 if self.mut == "a wave's partial dropped" else 4):
            t = t + s[:, w, 0]
        part.copy_(t)

    def cast_bf16(self, x, y):
        _need(x.numel() == y.numel(), "size")
        if self.mut == "cast truncates":
            y.copy_((x.view(I32) >> 16).to(I16).view(BFT))
        else:
            y.copy_(x.to(BFT))

    # ---- quant.hip
    def fp8_quant_blocks(self, na, nb_el):
        return SC.q_blocks(na, nb_el)

    def fp8_quant2(self, a, b, alpha, a8, b8, part, scales, a2=None, asum=None):
        _need((a2 is None) == (asum is None), "a2 and asum go together")
        K, Kp = a.shape[1], a8.shape[1]
        nb = SC.q_blocks(a.shape[0] * Kp, b.shape[0] * Kp)
        _need(_aligned(a, 16) and _aligned(b, 16) and _aligned(a8, 8) and _aligned(b8, 8), "alignment")
        _need(part.is_contiguous() and part.dtype == F32 and part.numel() >= 2 * nb and scales.numel() >= 2, "part / scales")
        _need(K % 8 == 0 and Kp % 8 == 0 and Kp >= K and b.shape[1] == K and b8.shape[1] == Kp, "shapes")
        if a2 is not None:
            asum.copy_((a.to(F32) + a2.to(F32)).to(BFT))
            a = asum
        s = []
        for k, x in enumerate((a, b)):
            ax = x.to(F32).abs().reshape(-1)
            blocks = torch.zeros(nb, dtype=F32)              # per-block partial maxima; fmaxf drops a NaN
            for blk in range(nb):
                mine = ax[blk * 2048:] if nb == 1 else torch.cat([ax[i:i + 2048] for i in range(blk * 2048, ax.numel(), nb * 2048)] or [ax[:0]])
                mine = torch.nan_to_num(mine, nan=0.0, posinf=float("inf"))
                blocks[blk] = mine.max() if mine.numel() else 0.0
            part[k * nb:(k + 1) * nb] = blocks
            s.append(torch.maximum(blocks.max() / 448.0, _t(1e-12)))
        scales[0] = s[0]
        scales[1] = s[1] if self.mut == "scale without alpha" else s[1] * _t(alpha)
        for x, y, sx in ((a, a8, s[0]), (b, b8, s[1])):
            inv = 1.0 / sx
            v = x.to(F32) * inv
            nan = torch.isnan(v)
            c = torch.where(nan, torch.full_like(v, -448.0), v).clamp(-448.0, 448.0)      # fmaxf(NaN, -448) = -448
            q = c.to(F8).view(U8)
            if self.mut != "nan to -448":
                q = torch.where(nan, torch.full_like(q, 0x7F), q)
            yb = y.view(U8)
            yb[:, :K] = q
            yb[:, K:] = 0
            if self.mut == "padding not zeroed" and Kp > K:
                yb[-1, Kp - 1] = 0x38

    # ---- reduce.hip
    def col_sum(self, ins, outs, acc):
        _need(1 <= len(ins) <= 4 and len(ins) == len(outs) == len(acc), "1..4 jobs")
        for x, o, a in zip(ins, outs, acc):
            _need(x.dim() == 3 and x.dtype == F32 and x.is_contiguous(), "in")
            _need(o.dtype == F32 and o.is_contiguous() and o.numel() == x.shape[0] * x.shape[2], "out")
        for x, o, a in zip(ins, outs, acc):
            s = torch.zeros(x.shape[0], x.shape[2], dtype=F32)
            for b in range(x.shape[1]):
                s = s + x[:, b, :]
            s = s.reshape(-1)
            o.copy_(o + s if a and self.mut != "col_sum assigns" else s)

    def fc_bias_grad(self, G, K, scale, alpha, out, acc):
        _need(G.dim() == 2 and G.dtype == BFT and G.is_contiguous(), "G")
        _need(1 <= K <= 32 and G.shape[1] >= 32 and G.stride(0) % 8 == 0 and _aligned(G, 16), "K, columns, stride, alignment")
        _need(out.dtype == F32 and out.numel() == K and out.is_contiguous(), "out")
        M = G.shape[0]
        cols = K + 1 if self.mut == "fc_bias sums column K" and K < 32 else K
        part = torch.zeros(256, cols, dtype=F32)
        for r0 in range(0, M, 256):
            rows = G[r0:r0 + 256, :cols].to(F32)
            part[:rows.shape[0]] = part[:rows.shape[0]] + rows
        t = torch.zeros(cols, dtype=F32)
        for r in range(256):
            t = t + part[r]
        if cols > K:
            t[K - 1] = t[K - 1] + t[K]
            t = t[:K]
        t = t * scale[0] * _t(alpha)
        out.copy_(out + t if acc else t)

    # ---- fill.hip
    def multi_fill(self, ts, pats):
        _need(len(ts) == len(pats) and len(ts) <= 8, "<= 8 regions")
        for x in ts:
            _need(x.is_contiguous() and (x.numel() * x.element_size()) % 4 == 0 and _aligned(x, 4), "contiguous words")
        for x, pat in zip(ts, pats):
            pat &= 0xFFFFFFFF
            w = x.view(U8).view(I32)
            if self.mut == "fill from the 16-B boundary below" and x.data_ptr() % 16:
                w = torch.as_strided(w, (w.numel() + 1,), (1,), w.storage_offset() - 1)
            w.fill_(pat - (1 << 32) if pat >= 1 << 31 else pat)

    def multi_copy(self, dsts, srcs, sdst=None, svals=()):
        _need(len(dsts) == len(srcs) <= 8 and len(svals) <= 4 and (not svals or sdst is not None), "<= 8 pairs, <= 4 scalars")
        for d, s in zip(dsts, srcs):
            _need(d.dtype == s.dtype and d.dim() == s.dim() and d.dim() in (1, 2), "same dtype, 1-D or 2-D")
            if d.dim() == 1:
                _need(d.is_contiguous() and s.is_contiguous() and s.numel() <= d.numel(), "1-D")
                d[:s.numel()] = s
                if self.mut != "rest of the row not zeroed":
                    d[s.numel():] = 0
            else:
                _need(d.shape[0] == s.shape[0] and s.shape[1] <= d.shape[1] and d.stride(1) == 1 and s.stride(1) == 1, "2-D")
                d[:, :s.shape[1]] = s
                if self.mut != "rest of the row not zeroed":
                    d[:, s.shape[1]:] = 0
        for i, x in enumerate(svals):
            sdst[i] = x

    def prep_inputs(self, x, y, li, lo):
        _need(x.dtype == F32 and y.dtype == BFT and x.numel() == y.numel() and _aligned(x, 16) and _aligned(y, 8), "feats")
        _need(li.dtype == I32 and lo.dtype == I32 and li.numel() == lo.numel(), "lengths")
        y.copy_(x.to(BFT))
        t = li.to(torch.int64) - 34
        r = torch.where(t >= 0, torch.div(t, 4, rounding_mode="trunc"), -torch.div(-t + 3, 4, rounding_mode="trunc")).to(I32)
        nl = li.numel()
        if self.mut == "length tail unwritten":
            nl = min(nl, max(1, SC.cdiv(x.numel() // 4, 256)) * 256)
        lo[:nl] = r[:nl]

    def transpose_bf16(self, a, out):
        _need(a.dtype == BFT and out.dtype == BFT and a.dim() == 2 and out.shape == (a.shape[1], a.shape[0]), "shapes")
        _need(a.stride(0) % 8 == 0 and out.stride(0) % 8 == 0 and _aligned(a, 16) and _aligned(out, 16), "strides")
        R, C = a.shape
        out.copy_(a.t())
        if self.mut == "tile edge one row too far" and R % 8:
            torch.as_strided(out, (C, R + 1), out.stride(), out.storage_offset())[:, R] = 0


EMU = Emu()


# ------------------------------------------------------------------------------ the tables keep their edges
def test_tables_cover_the_edges():
    c = SC.coverage()
    S = SC.STRIDE
    assert {S + 1, 2 * S, 2 * S + 5, 5 * S + 17} <= c["adam_gs_n4"] and min(c["adam_gs_n4"] - {0, 1}) < S
    for n4 in (700, S + 1, 2 * S, 2 * S + 5, 5 * S + 17):
        assert {(n4, t) for t in range(4)} <= c["adam_gs_tails"]
    assert {(0, 1), (0, 3), (1, 0), (1, 1)} <= c["adam_gs_tails"]                  # n = 1, 3, 4, 5
    ch = c["adam_chunks"]
    assert c["adam_chunk_grids"] == {-1, -7, -2048}
    assert any(g > 1 and k < 256 for g, k, _ in ch) and any(256 < k < 512 for g, k, _ in ch)
    assert any(g > 1 and g * k != n4 for g, k, n4 in ch) and any(g == 1 and k > 512 for g, k, _ in ch)
    r = c["ranges"]
    assert r["n"] == 64 and r["empty"] >= 3 and r["adjacent"] >= 2 and r["start"] and r["end"] and r["unsorted"]
    assert r["disjoint"] and r["gaps"] and r["groups"] > 512                      # more than one block of 256 groups
    assert SC.ARENA % 4 == 0 and all(lo % 4 == 0 and hi % 4 == 0 for lo, hi in SC.ADAM_RANGES["sixty-four"])
    assert set(SC.GN_N) == {1, 255, 256, 257, 1000, 70001} and SC.gn_blocks(70001) > 3
    mf = c["mf"]
    assert mf["counts"] >= set(range(9)) and mf["sizes"] == set(SC.MF_SIZES) and mf["patterns"] == set(SC.MF_PATTERNS)
    assert mf["dtypes"] == set(SC.MF_DTYPES) and mf["shifts"] >= {(s, sh) for s in SC.MF_SIZES for sh in (0, 4)}
    mc = c["mc"]
    assert mc["counts"] >= set(range(9)) and mc["kinds"] == {"1d", "2d"} and mc["narrower"] and mc["zero_rows"]
    assert mc["scalars"] >= {(ns, False) for ns in range(5)} | {(ns, True) for ns in range(1, 5)}
    fc = c["fc"]
    assert fc["M"] == set(SC.FC_M) and fc["K"] == set(SC.FC_K) and fc["ldg"] == set(SC.FC_LDG) and fc["acc"] == {0, 1}
    for K in SC.FC_K:                                     # every K meets every ldg
        assert {x[2] for x in SC.fc_cases() if x[1] == K} == set(SC.FC_LDG)
    cs = c["cs"]
    assert cs["jobs"] == {1, 2, 3, 4} and cs["shapes"] >= set(SC.CS_SHAPES) | {SC.WRAP} and cs["mixed"] and cs["boundaries_off_256"]
    assert SC.WRAP[0] * SC.WRAP[2] == 262144 + 513 and SC.WRAP[1] == 2
    assert set(SC.Q_SHAPES) == {(1, 1, 8, 8), (3, 5, 8, 128), (5, 300, 136, 136), (5, 300, 136, 256), (257, 2, 24, 128)}
    assert any(SC.q_blocks(ra * Kp, rb * Kp) > 1 and min(ra, rb) * Kp < 2048 for ra, rb, K, Kp in SC.Q_SHAPES)   # idle blocks


def test_bf16_reference_is_torchs_rne():
    x = torch.cat([SC.cast_input(1025), torch.randn(4096) * 1e-3, torch.randn(4096) * 1e30])
    fin = ~torch.isnan(x)
    assert torch.equal(SC.bf16_rne_bits(x)[fin], x.to(BFT).view(I16)[fin])
    assert bool(torch.isnan(SC.bf16_rne_bits(x)[~fin].view(BFT).float()).all())
    ties = SC.bf16_rne_bits(torch.tensor(SC.CAST_SPECIALS[7:11], dtype=F32)).view(BFT).float().tolist()
    assert ties == [1.0, 1.015625, -1.0, -1.015625]                    # down to even, up to even
    assert SC.bf16_rne_bits(torch.tensor([3.4028234663852886e38])).view(BFT).float().item() == float("inf")


def test_adam_inputs_hold_the_edges():
    for n in SC.ADAM_GS_N:
        d = SC.adam_inputs(n)
        assert bool((d["v"] >= 0).all())
        if n >= 16:
            for i in d["zero"]:
                assert d["g"][i] == 0 and d["m"][i] == 0 and d["v"][i] == 0 and d["e"][i] == d["p"][i]
            assert all(d["v"][i] == 0 and d["m"][i] != 0 for i in d["v0"]) and bool(torch.isnan(d["g"][d["nan"]]).all())
            assert float(d["g"][6]) == SC.f32r(1e18) and n - 1 in d["zero"] and n - 2 in d["nan"]
            want, tol = SC.adam_oracle(d, 1.0)
            fin = ~torch.isnan(d["g"])
            assert all(bool(torch.isfinite(want[k][fin]).all()) and bool((tol[k][fin] > 0).all()) for k in "pmv")


# ------------------------------------------------------------------------------ the emulations pass every case
@pytest.mark.parametrize("n", SC.ADAM_GS_N)
def test_emulated_adam_grid_strided(n):
    SC.run_adam(EMU, DEV, dict(n=n, max_grid=3))


def test_emulated_adam_forms_and_options():
    for n, mg in SC.ADAM_CHUNK:
        SC.same_forms("n=%d" % n, SC.run_adam(EMU, DEV, dict(n=n, max_grid=3)), SC.run_adam(EMU, DEV, dict(n=n, max_grid=mg)))
    for n in SC.ADAM_LDS_N:
        SC.same_forms("n=%d" % n, SC.run_adam(EMU, DEV, dict(n=n, lds=0)), SC.run_adam(EMU, DEV, dict(n=n, lds=32768)))
    for opt in SC.ADAM_OPTIONS:
        for mg in (3, -7):
            SC.run_adam(EMU, DEV, dict(n=SC.ADAM_OPT_N, max_grid=mg, **opt))
    for k in SC.ADAM_RANGES:
        SC.run_adam(EMU, DEV, dict(n=SC.ARENA), ranges=k)
        SC.run_adam(EMU, DEV, dict(n=SC.ARENA, hyper=True, ema=False, gscale=SC.GSCALES[1]), ranges=k)


def test_emulated_grad_norm_and_cast():
    for n in SC.GN_N:
        for parts in SC.GN_PARTS:
            for gs in (1.0, 0.5):
                SC.run_grad_norm(EMU, DEV, n, parts, gs)
        for val, gs in SC.GN_POISON:
            for where in sorted({0, n // 2, n - 1}):
                SC.run_grad_norm(EMU, DEV, n, None, gs, val, where)
        SC.run_grad_norm(EMU, DEV, n, None, 1.0, flag0=1)
    for n in SC.CAST_N:
        for first in range(len(SC.CAST_SPECIALS) if n == 1 else 1):
            SC.run_cast(EMU, DEV, n, first)


@pytest.mark.parametrize("sh", SC.Q_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_quant(sh):
    for variant in SC.Q_VARIANTS + SC.Q_NONFINITE:
        SC.run_quant(EMU, DEV, sh, variant)


def test_emulated_reductions():
    for jobs in SC.CS_CASES:
        SC.run_col_sum(EMU, DEV, jobs)
    for M, K, ldg, acc in SC.fc_cases():
        SC.run_fc_bias(EMU, DEV, M, K, ldg, acc)


def test_emulated_fill():
    for regs in SC.mf_cases():
        SC.run_multi_fill(EMU, DEV, regs)
    for pairs, ns in SC.MC_CASES:
        SC.run_multi_copy(EMU, DEV, pairs, ns)
    for n in SC.PREP_N:
        SC.run_prep(EMU, DEV, n, 3)
    for nl in SC.PREP_NL:
        SC.run_prep(EMU, DEV, 8, nl)
    for R in SC.TR_SIZES:
        for C in SC.TR_SIZES:
            SC.run_transpose(EMU, DEV, R, C)


def test_emulated_refusals():
    for name, thunk, bufs in SC.refusals(EMU, DEV):
        SC.run_refusal(name, thunk, bufs)


# ------------------------------------------------------------------------------ planted errors
N3 = 4 * 700 + 3
PLANTED = {
    "tail dropped": lambda e: SC.run_adam(e, DEV, dict(n=N3, max_grid=3)),
    "group past the end": lambda e: SC.run_adam(e, DEV, dict(n=N3, max_grid=3)),
    "hyper": lambda e: SC.run_adam(e, DEV, dict(n=N3, max_grid=3, hyper=True)),
    "skip ignored": lambda e: SC.run_adam(e, DEV, dict(n=N3, max_grid=3, skip=1)),
    "ema old p": lambda e: SC.run_adam(e, DEV, dict(n=N3, max_grid=3)),
    "p16 truncated": lambda e: SC.run_adam(e, DEV, dict(n=N3, max_grid=3)),
    "range runs on": lambda e: SC.run_adam(e, DEV, dict(n=SC.ARENA), ranges="sixty-four"),
    "flag skips the last element": lambda e: SC.run_grad_norm(e, DEV, 257, None, 1.0, float("inf"), 256),
    "a wave's partial dropped": lambda e: SC.run_grad_norm(e, DEV, 1000, None, 1.0),
    "cast truncates": lambda e: SC.run_cast(e, DEV, 255),
    "padding not zeroed": lambda e: SC.run_quant(e, DEV, (3, 5, 8, 128), "random"),
    "nan to -448": lambda e: SC.run_quant(e, DEV, (5, 300, 136, 256), "nan a"),
    "scale without alpha": lambda e: SC.run_quant(e, DEV, (3, 5, 8, 128), "random"),
    "col_sum assigns": lambda e: SC.run_col_sum(e, DEV, SC.CS_CASES[2]),
    "fc_bias sums column K": lambda e: SC.run_fc_bias(e, DEV, 257, 29, 40, 0),
    "fill from the 16-B boundary below": lambda e: SC.run_multi_fill(e, DEV, SC.mf_cases()[-1]),
    "rest of the row not zeroed": lambda e: SC.run_multi_copy(e, DEV, list(SC.MC_PAIRS[:3]), 0),
    "length tail unwritten": lambda e: SC.run_prep(e, DEV, 8, 257),
    "tile edge one row too far": lambda e: SC.run_transpose(e, DEV, 65, 7),
}


@pytest.mark.parametrize("mut", list(PLANTED))
def test_planted_error_is_caught(mut):
    PLANTED[mut](EMU)                                   # the same case passes unplanted
    worst, counts = dict(SC.WORST), dict(SC.COUNTS)
    with pytest.raises(AssertionError) as ei:
        PLANTED[mut](Emu(mut))
    SC.WORST.clear(), SC.WORST.update(worst), SC.COUNTS.clear(), SC.COUNTS.update(counts)      # the report is of right kernels
    print("STREAMPLANT %-36s %s" % (mut, str(ei.value)[:150]))


def test_planted_nan_message_names_the_byte():
    with pytest.raises(SC.Mismatch, match=r"NaN at \[2, 68\] was stored as byte 0xFE \(-448"):
        SC.run_quant(Emu("nan to -448"), DEV, (5, 300, 136, 256), "nan a")
