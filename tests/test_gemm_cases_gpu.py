"""GEMM kernels (csrc/gemm.hip, csrc/gemm8.hip) and ops/gemm.py's routing per element against the
fp64 oracle of tests/gemm_cases.py, whose docstring holds the method, the two input families and
the tolerance. Every launch runs on guard-banded operands and writes a guard-banded output; both
families run per case and the oracle of a shape is shared by its configurations.

Printed (run with -s): GEMMWORST lines, the worst err/tol per kernel and output type, and
GEMMLAUNCH lines, the kernel instantiations launched. profiles/gemm_oracle_coverage.md records them.
"""
import pytest
import torch

import gemm_cases as GC

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from deepspeech_amd.ops import _ext  # noqa: E402
from deepspeech_amd.ops import gemm as G  # noqa: E402

DEV = torch.device("cuda:0")
F64, F32, BFT, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(GC.WORST.items()):
        print("GEMMWORST %-24s err/tol %.3f" % (k, v))
    for k in sorted(GC.LAUNCHED):
        print("GEMMLAUNCH " + k)


def _scalar(v):
    return None if v is None else torch.tensor([v], dtype=F32, device=DEV)


def _counters_zero(name):
    torch.cuda.synchronize()
    for buf in G._counters.values():
        assert int(buf.abs().sum()) == 0, name + ": split-K counters not left at zero"


def launch(d, ops, spec):
    """one launch of `spec` on the stored operands `ops`, into a fresh guard-banded output"""
    M, N, K, a_col, b_col, batch, Ml, Kl, fp8 = d["sh"]
    pa, pb, bias = ops
    out = GC.output(d, spec, DEV)
    al, a1, a2 = GC.scalars(d, spec)
    bv = bias.vec() if spec.get("bias") else None
    lay = ("c" if a_col else "r") + ("c" if b_col else "r")
    if spec["kern"] == "gemm":
        G.gemm(pa.t, pb.t, out.t, M, N, K, a_col, b_col, spec["epi"], al, bv, cfg=spec["cfg"], alpha_dev=_scalar(a1),
               Ml=Ml, Kl=Kl)
        GC.LAUNCHED.add("gemm cfg%d %s epi%d" % (spec["cfg"], lay, spec["epi"]))
    else:
        kw = dict(splits=1) if spec.get("req", 1) == 1 else dict(plan=(spec["req"], bool(spec.get("ext"))))
        G.gemm8(pa.t, pb.t, out.t, spec["epi"], al, bv, _scalar(a1), _scalar(a2), a_col=a_col, b_col=b_col,
                max_grid=spec.get("max_grid", 0), **kw)
        GC.LAUNCHED.add("gemm8 %s %s epi%d%s" % ("fp8" if fp8 else "bf16", lay, spec["epi"],
                                                 "" if spec.get("S", 1) == 1 else
                                                 " split + g8_reduce_kernel" if spec.get("ext") else " split"))
    return out


def run(sh, specs_of, kernel=None):
    for fam in "AB":
        d = GC.problem(fam, sh)
        ops = GC.stored(d, DEV)
        for spec in specs_of(sh):
            out = launch(d, ops, spec)
            name = GC.case_name(d, spec)
            out.verify(name)
            tag = kernel or "%s%s %s" % (spec["kern"], " fp8" if sh[8] else "", "bf16" if spec["epi"] == 0 else "fp32")
            GC.verify(d, spec, out.t, kernel=tag)
            if spec.get("S", 1) > 1:
                _counters_zero(name)


# ------------------------------------------------------------------------------ csrc/gemm.hip
def test_tile_table():
    C = _ext.ext()
    for cfg, t in GC.TILES.items():
        assert tuple(C.gemm_tile(cfg)) == t
    with pytest.raises(RuntimeError):
        C.gemm_tile(9)


@pytest.mark.parametrize("sh", GC.GEMM_SHAPES + GC.GEMM_BATCH + GC.GEMM_CTC, ids=GC.ident)
def test_gemm(sh):
    """all nine configurations, epi 0 (without / with bias and alpha_dev), 1, 2"""
    run(sh, GC.gemm_launches)


@pytest.mark.parametrize("cfgs,sh", GC.GEMM_NINE, ids=lambda v: GC.ident(v) if len(v) == 9 else "cfg" + "+".join(map(str, v)))
def test_gemm_nine_m_tiles(cfgs, sh):
    """ntm = 9: the last group of the grouped tile order holds one m-tile"""
    run(sh, lambda s: GC.gemm_launches(s, cfgs))


@pytest.mark.parametrize("cfg", GC.PERSISTENT)
def test_gemm_persistent_refuses_accumulate(cfg):
    d = GC.problem("A", GC.shape_of(136, 136, 64, True, True))
    pa, pb, _ = GC.stored(d, DEV)
    out = GC.output(d, dict(epi=2), DEV)
    with pytest.raises(RuntimeError, match=r"kernel launch failed in gemm \(code"):
        G.gemm(pa.t, pb.t, out.t, 136, 136, 64, True, True, 2, 1.0, None, cfg=cfg)
    torch.cuda.synchronize()
    out.verify("cfg %d epi 2" % cfg, written=False, initial=d["c0"])


@pytest.mark.parametrize("b_col", [False, True], ids=["rr", "rc"])
@pytest.mark.parametrize("K", [40, 136])
@pytest.mark.parametrize("cfg", GC.PERSISTENT)
def test_gemm_persistent_seam(cfg, K, b_col):
    """more tiles than workgroups: the next tile's prologue is issued under this tile's stores"""
    (sh,) = [s for c, s in GC.seam_shapes(_ext.num_cus(0)) if c == cfg and s[2] == K and s[4] == b_col]
    bias = dict(kern="gemm", cfg=cfg, epi=0, bias=True, adev=True)
    f32 = dict(kern="gemm", cfg=cfg, epi=1, bias=False, adev=False)
    for fam, spec in (("A", f32 if b_col else bias), ("B", bias if b_col else f32)):
        d = GC.problem(fam, sh)
        out = launch(d, GC.stored(d, DEV), spec)
        out.verify(GC.case_name(d, spec))
        GC.verify(d, spec, out.t, kernel="gemm seam %s" % ("bf16" if spec["epi"] == 0 else "fp32"))


# ------------------------------------------------------------------------------ csrc/gemm8.hip
@pytest.mark.parametrize("sh", GC.GEMM8_SHAPES + GC.GEMM8_BATCH + [GC.GEMM8_17], ids=GC.ident)
def test_gemm8(sh):
    run(sh, GC.gemm8_launches)


@pytest.mark.parametrize("sh,req", GC.GEMM8_SPLIT + GC.FP8_SPLIT, ids=lambda v: GC.ident(v) if isinstance(v, tuple) else "S%d" % v)
def test_gemm8_split(sh, req):
    """forced plans (S, in-launch reduce) and (S, g8_reduce_kernel): the slices actually run, the
    counters left at zero"""
    C = _ext.ext()
    assert int(C.gemm8_splits(sh[2], sh[8], req)) == GC.slices_of(sh[2], req, sh[8])[0]
    run(sh, lambda s: GC.split_launches(s, req))


@pytest.mark.parametrize("sh", GC.GEMM8_MAXGRID, ids=GC.ident)
def test_gemm8_max_grid(sh):
    """a grid capped at 8 workgroups: looping over 12 units, and idle beside 1"""
    run(sh, lambda s: [dict(spec, max_grid=8) for spec in GC.gemm8_launches(s)])


@pytest.mark.parametrize("sh", GC.FP8_SHAPES, ids=GC.ident)
def test_gemm8_fp8(sh):
    """e4m3 operands created here, the oracle from the stored values, the scales as device scalars"""
    run(sh, GC.fp8_launches)


def _group(fam, members):
    ds = [GC.problem(fam, GC.shape_of(M, N, K, True, True)) for M, N, K, _, _ in members]
    ops = [GC.stored(d, DEV, 8 + 8 * (i % 7), 64 - 8 * (i % 7)) for i, d in enumerate(ds)]
    specs = [dict(kern="gemm8_group", epi=epi, alpha=1.0, S=GC.slices_of(K, req)[0], req=req) for _, _, K, req, epi in members]
    outs = [GC.output(d, s, DEV) for d, s in zip(ds, specs)]
    return ds, ops, specs, outs


def _group_verify(ds, specs, outs):
    for d, spec, out in zip(ds, specs, outs):
        out.verify(GC.case_name(d, spec))
        GC.verify(d, spec, out.t, kernel="gemm8_group fp32")
    GC.LAUNCHED.add("gemm8 bf16 cc group")


def test_gemm8_group_mixed():
    """members that differ in M, N, K, split count and epilogue, in one launch"""
    C = _ext.ext()
    for fam in "AB":
        ds, ops, specs, outs = _group(fam, GC.GROUP_MIXED)
        ws = torch.empty(sum(s["S"] * m[0] * m[1] for s, m in zip(specs, GC.GROUP_MIXED) if s["S"] > 1), device=DEV)
        cnt = G._tile_counters(DEV, sum(GC.cdiv(m[0], 256) * GC.cdiv(m[1], 256) for m in GC.GROUP_MIXED))
        C.gemm8_group([o[0].t for o in ops], [o[1].t for o in ops], [o.t for o in outs], [s["epi"] for s in specs],
                      [s["req"] for s in specs], True, True, ws, cnt, _ext.num_cus(0))
        _group_verify(ds, specs, outs)
        _counters_zero("gemm8_group")


def test_gemm8_group_many():
    """25 members: two launches"""
    for fam in "AB":
        ds, ops, specs, outs = _group(fam, GC.GROUP_MANY)
        G.gemm8_group([(o[0].t, o[1].t, out.t) for o, out in zip(ops, outs)])
        _group_verify(ds, specs, outs)


# ------------------------------------------------------------------------------ ops/gemm.py matmul
@pytest.mark.parametrize("c", GC.ROUTING, ids=lambda c: "-".join(str(int(v)) if v is not None else "x" for v in c))
def test_matmul_routing(c, monkeypatch):
    ta, tb, M, N, K, f32o, acc, bias, splits, max_grid = c
    a_col, b_col = ta, not tb
    epi = (2 if acc else 1) if f32o else 0
    calls = []
    for fn in ("gemm", "gemm8"):
        real = getattr(G, fn)
        monkeypatch.setattr(G, fn, lambda *a, _r=real, _n=fn, **k: (calls.append(_n), _r(*a, **k))[1])
    for fam in "AB":
        d = GC.problem(fam, GC.shape_of(M, N, K, a_col, b_col))
        pa, pb, pbias = GC.stored(d, DEV)
        a = pa.t.t() if ta else pa.t                # a [M, K]
        b = pb.t.t() if tb else pb.t                # b [K, N]
        if G._small_rowrow(M, N, K, a_col, b_col, 1, epi, a):
            want = "gemm"
        elif G.gemm8_supported(M, N, K, False, a_col, b_col):
            want = "gemm8"
        else:
            want = "gemm" if G.supported(M, N, K, a_col, b_col) else None
        S = GC.slices_of(K, splits)[0] if (want == "gemm8" and splits) else 1
        spec = dict(kern="matmul", epi=epi, bias=bias, S=S)
        out = GC.output(d, spec, DEV)
        del calls[:]
        ok = G.matmul(a, b, out.t, accumulate=acc, alpha=GC.SCAL[fam][0], bias=pbias.vec() if bias else None,
                      max_grid=max_grid, splits=splits)
        assert ok == (want is not None) and calls == ([want] if want else []), (calls, want)
        out.verify(GC.case_name(d, spec))
        GC.verify(d, spec, out.t, kernel="matmul -> %s %s" % (want, "bf16" if epi == 0 else "fp32"))


def test_matmul_declines():
    """False, and the output untouched"""
    M, N, K = 64, 64, 64
    d = GC.problem("A", GC.shape_of(M, N, K, False, True))
    pa, pb, pbias = GC.stored(d, DEV)
    a, b = pa.t, pb.t
    wide = torch.ones(M + 8, 2 * K + 16, device=DEV, dtype=BFT)
    odd = torch.ones(M, K + 4, device=DEV, dtype=BFT)
    cases = [("an fp32 operand", a.float(), b, F32, {}),
             ("a pointer offset by 4 elements", wide[:M, 4:4 + K], b, F32, {}),
             ("a row stride that is no multiple of 8", odd[:, :K], b, F32, {}),
             ("bf16 out with accumulate", a, b, BFT, dict(accumulate=True)),
             ("fp32 out with a bias", a, b, F32, dict(bias=pbias.vec())),
             ("a view with no unit stride", wide[:M, 0:2 * K:2], b, F32, {})]
    for name, aa, bb, odt, kw in cases:
        out = GC.Plane(1, M, N, odt, DEV, 16)
        assert G.matmul(aa, bb, out.t, **kw) is False, name
        torch.cuda.synchronize()
        out.verify(name, written=False)


# ------------------------------------------------------------------------------ refusals
# Every case is stopped by a host check before anything is launched; every tensor handed in is
# allocated to the extent its arguments name.
def _bf(rows, cols, ld=None):
    return torch.ones(rows, ld or cols, device=DEV, dtype=BFT)[:, :cols]


def test_gemm_refusals():
    cases = [("K % 8 with a row operand", dict(A=_bf(16, 12, 16), B=_bf(8, 12, 16), M=16, N=8, K=12)),
             ("N % 4", dict(A=_bf(16, 16), B=_bf(6, 16), M=16, N=6, K=16)),
             ("column-mode M % 8", dict(A=_bf(16, 12, 16), B=_bf(16, 8), M=12, N=8, K=16, a_col=True, b_col=True)),
             ("configuration 9", dict(A=_bf(16, 16), B=_bf(8, 16), M=16, N=8, K=16, cfg=9)),
             ("Kl with row-row", dict(A=_bf(16, 16), B=_bf(8, 16), M=16, N=8, K=16, Kl=8)),
             ("Ml < M", dict(A=_bf(16, 8), B=_bf(16, 8), M=16, N=8, K=16, a_col=True, b_col=True, Ml=8))]
    for name, c in cases:
        out = GC.Plane(1, c["M"], c["N"], F32, DEV, 16)
        with pytest.raises(RuntimeError, match=r"kernel launch failed in gemm \(code"):
            G.gemm(c["A"], c["B"], out.t, c["M"], c["N"], c["K"], c.get("a_col", False), c.get("b_col", False), 1, 1.0,
                   None, cfg=c.get("cfg", 3), Ml=c.get("Ml", 0), Kl=c.get("Kl", 0))
        torch.cuda.synchronize()
        out.verify("gemm refuses " + name, written=False)


def test_gemm8_refusals():
    f8 = lambda r, c: torch.ones(r, c, device=DEV, dtype=BFT).to(F8)
    b3 = lambda n: torch.ones(n, 16, 64, device=DEV, dtype=BFT)
    ragged_ldc = torch.full((16, 14), float("nan"), device=DEV)
    cases = [("K % 32 with a row operand", _bf(16, 48), _bf(8, 48), (16, 8), F32, {}, None),
             ("fp8 in column mode", f8(128, 16), f8(128, 16), (16, 16), F32, dict(a_col=True, b_col=True), None),
             ("fp8 with K % 128", f8(16, 64), f8(8, 64), (16, 8), F32, {}, None),
             ("a bias with epi 1", _bf(16, 64), _bf(8, 64), (16, 8), F32, dict(bias=torch.ones(8, device=DEV, dtype=BFT)), None),
             ("batch 25", b3(25), b3(25), (25, 16, 16), F32, {}, None),
             ("ext_red with a batch", torch.ones(2, 16, 128, device=DEV, dtype=BFT), torch.ones(2, 16, 128, device=DEV, dtype=BFT),
              (2, 16, 16), F32, dict(plan=(2, True)), None),
             ("ldc % 4", _bf(16, 64), _bf(12, 64), (16, 12), F32, {}, ragged_ldc[:, :12])]
    for name, A, B, oshape, odt, kw, view in cases:
        out = GC.Plane(oshape[0] if len(oshape) == 3 else 1, oshape[-2], oshape[-1], odt, DEV, 16)
        kw = dict(dict(splits=1) if "plan" not in kw else {}, **kw)
        with pytest.raises(RuntimeError, match=r"gemm8"):
            G.gemm8(A, B, out.t if view is None else view, 1, 1.0, **kw)
        torch.cuda.synchronize()
        out.verify("gemm8 refuses " + name, written=False)
        if view is not None:
            assert bool(torch.isnan(ragged_ldc).all()), name
        _counters_zero(name)
