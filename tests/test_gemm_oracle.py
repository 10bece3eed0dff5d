"""The GEMM oracle of tests/gemm_cases.py, checked on the CPU:

  * preconditions() and coverage() hold for every table, so a table cannot lose an edge unnoticed;
  * correctly rounded emulations of a right kernel (bf16 / e4m3 operands, fp32 accumulation
    sequential in k, in blocks of 32 then across blocks as an MFMA would, and in S slices summed in
    slice order; the fp32 epilogue fused and unfused; one RNE bf16 store) pass every family B
    entry within the tolerance and reproduce family A bit for bit;
  * twelve planted errors in a passing emulated output fail in both families, at their
    coordinates; the whole-matrix ratio of tests/test_gemm_gpu.py is printed beside each (run
    with -s), here and scaled to that file's 7712 x 800 output;
  * the guard-band checker flags a touched band and a payload element left at the sentinel.
"""
import pytest
import torch

import gemm_cases as GC

F64, F32, BFT = torch.float64, torch.float32, torch.bfloat16
EMU_WORST = {}
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(EMU_WORST.items()):
        print("GEMMEMU %-24s worst err/tol %.3f" % (k, v))
    for k, (here, there) in RATIOS.items():
        print("GEMMPLANT %-44s whole-matrix ratio %.2e here, %.2e at 7712 x 800" % (k, here, there))


# ------------------------------------------------------------------------------ emulation
def _seq(a, b, k0, k1):
    acc = torch.zeros(a.shape[0], a.shape[1], b.shape[1], dtype=F32)
    for k in range(k0, k1):
        acc.addcmul_(a[:, :, k:k + 1], b[:, :, k].unsqueeze(1))      # the product is exact in fp32
    return acc


def _blk(a, b, k0, k1):
    acc = torch.zeros(a.shape[0], a.shape[1], b.shape[1], dtype=F32)
    for q in range(k0, k1, 32):
        acc = acc + _seq(a, b, q, min(q + 32, k1))
    return acc


def accumulate(d, mode, S=1, first=0):
    """fp32 A B^T. mode seq / blk / slices (S slices of whole k-tiles, summed from slice `first`)"""
    K, fp8 = d["sh"][2], d["sh"][8]
    a, b = d["A"].to(F32), d["B"].to(F32)
    if mode == "seq":
        return _seq(a, b, 0, K)
    if mode == "blk":
        return _blk(a, b, 0, K)
    kt = 128 if fp8 else 64
    kps = GC.cdiv(GC.cdiv(K, kt), S)
    parts = [_blk(a, b, s * kps * kt, min((s + 1) * kps * kt, K)) for s in range(S)]
    v = parts[first]
    for p in parts[first + 1:]:
        v = v + p
    return v


def epilogue(d, spec, acc, fused=True, bias_shift=0, bias_after=False, drop_adev2=False, store_only=False):
    al, a1, a2 = GC.scalars(d, spec)
    alpha = torch.tensor(al, dtype=F32)
    if a1 is not None:
        alpha = alpha * torch.tensor(a1, dtype=F32)
    if a2 is not None and not drop_adev2:
        alpha = alpha * torch.tensor(a2, dtype=F32)
    add = None
    if spec.get("bias"):
        add = d["bias"].roll(bias_shift).to(F32)
    if spec["epi"] == 2 and not store_only:
        add = d["c0"].to(F32)
    if add is None or bias_after:
        v = alpha * acc
    elif fused:
        v = (alpha.to(F64) * acc.to(F64) + add.to(F64)).to(F32)        # one rounding: an fma
    else:
        v = alpha * acc + add
    if spec["epi"] != 0:
        return v
    if bias_after and add is not None:
        return (v.to(BFT).to(F32) + add).to(BFT)
    return v.to(BFT)


def _shapes():
    seen, out = set(), {}
    for sh, spec in GC.all_launches():
        key = (spec["epi"], bool(spec.get("bias")), bool(spec.get("adev")), bool(spec.get("adev2")), spec.get("S", 1))
        if (sh, key) not in seen:
            seen.add((sh, key))
            out.setdefault(sh, []).append(spec)
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("sh", list(SHAPES), ids=GC.ident)
def test_emulations_pass_every_case(sh):
    for fam in "AB":
        d = GC.problem(fam, sh)
        GC.preconditions(d)
        accs = {}
        for spec in SHAPES[sh]:
            S = spec.get("S", 1)
            for mode, fused in (("slices", True),) if S > 1 else (("seq", True), ("blk", False)):
                if (mode, S) not in accs:
                    accs[mode, S] = accumulate(d, mode, S)
                w = GC.verify(d, spec, epilogue(d, spec, accs[mode, S], fused), kernel="emu")
                k = "%s %s" % (mode, "bf16" if spec["epi"] == 0 else "fp32")
                EMU_WORST[k] = max(EMU_WORST.get(k, 0.0), w)


def test_family_a_exercises_the_bf16_rounding():
    """bf16 outputs of family A that bf16 cannot hold: in every case with a bias, ties included"""
    ties = 0
    for sh, specs in SHAPES.items():
        d = GC.problem("A", sh)
        for spec in specs:
            if spec["epi"] == 0 and spec.get("bias") and sh[0] * sh[1] >= 64:
                r, _ = GC.expected(d, spec)
                inexact = r.to(F32).to(BFT).to(F64) != r
                assert bool(inexact.any()), GC.case_name(d, spec)
                ties += int((inexact & (r == r.round()) & (r.abs() < 512)).sum())
    assert ties > 0


def test_tables_cover_the_edges():
    c = GC.coverage()
    for cfg, (bm, bn) in GC.TILES.items():
        e = c["gemm"][cfg]
        assert {1, 15, 16, 17, bm - 1} <= e["mrem"] and e["small_m"], (cfg, e["mrem"])
        assert {4, 12, 20, bn - 4} <= e["nrem"] and e["n4"], (cfg, e["nrem"])
        assert {8, bm - 8} <= e["mrem_col"] and {8, bn - 8} <= e["nrem_col"], (cfg, e)
        assert e["two_by_two"] and e["layouts"] == set(GC.LAYOUTS)
        want = {(0, False), (0, True), (1, False)} | (set() if cfg in GC.PERSISTENT else {(2, False)})
        assert e["epis"] == want, (cfg, e["epis"])
    # 1..4 k-tiles, every kvalid class of the last one, the K - 8 clamp (K % 64 not in {0, 56})
    assert {(n, "64") for n in (1, 2, 3)} <= c["gemm_k_row"] and {(n, "32") for n in (1, 2)} <= c["gemm_k_row"]
    assert {(n, "<32") for n in (1, 2, 3, 4)} <= c["gemm_k_row"] and {(n, "32..64") for n in (1, 2)} <= c["gemm_k_row"]
    assert {n for n, _ in c["gemm_k_row"]} == {1, 2, 3, 4}
    assert set(GC.G_K) | {5, 63, 65} == c["gemm_k_cc"]
    assert {n for _, n in c["gemm_nine"]} == {9} and {cfg for cfg, _ in c["gemm_nine"]} >= {0, 3}
    assert (False, True, 0, 29, 0, True) in c["gemm_ctc"]
    assert {(True, True, 32, 0, 1, True), (True, True, 32, 0, 2, True)} <= c["gemm_ctc"]
    assert c["gemm_batch"] == {(a, b, 3) for a, b in GC.LAYOUTS}
    g8 = c["gemm8"]
    assert g8["m_row"] == set(GC.G8_M) and g8["n_row"] == set(GC.G8_N)
    assert g8["m_col"] == set(GC.G8_MC) and g8["n_col"] == set(GC.G8_NC)
    assert g8["k_row"] == set(GC.G8_K) and g8["k_cc"] == set(GC.G8_KCC) and g8["layouts"] == set(GC.LAYOUTS)
    sp = g8["splits"]
    assert (96, 5, (1, 1)) in sp                                    # the request exceeds the k-tile count
    assert (160, 2, (2, 1)) in sp                                   # the ragged k-tile alone in the last slice
    assert (288, 2, (3, 2)) in sp and (288, 3, (2, 2, 1)) in sp     # shorter last slice; odd and even counts
    assert g8["maxgrid_units"][0] < 8 < g8["maxgrid_units"][-1]
    assert {3, 24} <= g8["batches"] and g8["m_tiles_17"] == (17, 1, 32)
    gr = g8["group"]
    assert min(len(gr[k]) for k in ("Ms", "Ns", "Ks")) >= 4 and gr["S"] >= {1, 2, 3} and gr["epis"] == {1, 2}
    assert gr["many"] == 25
    assert g8["fp8_k"] == {128, 256, 384} and g8["fp8_splits"] == {(1, 1), (2, 1)}
    assert {(1, 4), (127, 124), (129, 132), (257, 260)} <= g8["fp8_mn"]
    for cus in (256, 304, 64):
        for cfg, sh in GC.seam_shapes(cus):
            bm, bn = GC.TILES[cfg]
            assert GC.cdiv(sh[0], bm) * GC.cdiv(sh[1], bn) > cus and sh[0] % bm and sh[1] % bn and sh[1] > bn


# ------------------------------------------------------------------------------ planted errors
G8 = dict(kern="gemm8", epi=0, bias=True, adev=True, adev2=True, S=3, req=3)
BASE = GC.shape_of(272, 260, 288)
TAIL = GC.shape_of(272, 260, 40)
SQUARE = GC.shape_of(264, 264, 96)


def _caught(d, spec, got, region=None):
    """the checker fails on `got`, at the planted coordinates"""
    with pytest.raises(GC.Mismatch) as ei:
        GC.verify(d, spec, got, kernel="planted")
    c = ei.value.coords
    if region is not None:
        (m0, m1), (n0, n1) = region
        assert m0 <= c["m"] < m1 and n0 <= c["n"] < n1, (c, region)
    return ei.value


def _ratio(tag, d, spec, got, local=True):
    r, _ = GC.expected(d, spec)
    here = GC.old_ratio(torch.nan_to_num(got.to(F64)), r)
    mn = d["sh"][0] * d["sh"][1]
    RATIOS["%s %s" % (tag, d["fam"])] = (here, here * (mn / (7712.0 * 800)) ** 0.5 if local else here)


@pytest.mark.parametrize("fam", "AB")
def test_planted_errors_are_caught(fam):
    d = GC.problem(fam, BASE)
    a, b = d["A"].to(F32), d["B"].to(F32)
    acc = accumulate(d, "slices", 3)
    good = epilogue(d, G8, acc)
    GC.verify(d, G8, good, kernel="emu")

    # the last k-substep dropped in one tile row (rows 256..271 of the second m-tile)
    bad = acc.clone()
    bad[:, 256:272] -= _seq(a[:, 256:272], b, 256, 288)
    got = epilogue(d, G8, bad)
    _caught(d, G8, got, ((256, 272), (0, 260)))
    _ratio("last k-substep dropped in a tile row", d, G8, got)
    # one term doubled
    bad = acc.clone()
    bad[0, 130, 77] += a[0, 130, 200] * b[0, 77, 200]
    got = epilogue(d, G8, bad)
    _caught(d, G8, got, ((130, 131), (77, 78)))
    _ratio("one term doubled", d, G8, got)
    # a poisoned gap value multiplied: a NaN in one fragment row
    bad = acc.clone()
    bad[0, 271, 256:260] = float("nan")
    _caught(d, G8, epilogue(d, G8, bad), ((271, 272), (256, 260)))
    # the bias shifted by one 4-column group
    got = epilogue(d, G8, acc, bias_shift=4)
    _caught(d, G8, got)
    _ratio("bias shifted by 4 columns", d, G8, got, local=False)
    # the bias added after the bf16 rounding
    got = epilogue(d, G8, acc, bias_after=True)
    assert not torch.equal(got, good)
    _caught(d, G8, got)
    _ratio("bias added after the bf16 rounding", d, G8, got, local=False)
    # alpha_dev2 ignored
    got = epilogue(d, G8, acc, drop_adev2=True)
    _caught(d, G8, got)
    # the first slab skipped in the slice sum, in one 256 x 256 tile
    bad = acc.clone()
    bad[:, 256:, 256:] = accumulate(d, "slices", 3, first=1)[:, 256:, 256:]
    got = epilogue(d, G8, bad)
    _caught(d, G8, got, ((256, 272), (256, 260)))
    _ratio("first slab skipped in a corner tile", d, G8, got)
    # accumulate applied as store
    acc2 = dict(G8, epi=2, bias=False)
    GC.verify(d, acc2, epilogue(d, acc2, acc), kernel="emu")
    _caught(d, acc2, epilogue(d, acc2, acc, store_only=True))
    # a 16 x 4 fragment left unwritten, one row written past M: the buffer checks
    p = GC.output(d, G8, "cpu")
    p.t.copy_(good[0])
    p.verify("clean")
    p.t[32:48, 128:132].view(torch.int16).fill_(GC.SENT16)
    with pytest.raises(GC.Mismatch, match="64 of 70720 payload elements were never written") as ei:
        p.verify("fragment")
    assert ei.value.coords == dict(b=0, m=32, n=128)
    _caught(d, G8, p.t.unsqueeze(0), ((32, 48), (128, 132)))
    p.t[32:48, 128:132] = good[0, 32:48, 128:132]
    p.buf[0, p.before + 272, p.left:p.left + 260] = good[0, 271]
    with pytest.raises(GC.Mismatch, match="past the last row") as ei:
        p.verify("row past M")
    assert ei.value.coords["m"] == 272

    # the clamped tail chunk multiplied (K = 40: chunks 5..7 of the k-tile re-read k = 32..39)
    t = GC.problem(fam, TAIL)
    g = dict(kern="gemm", cfg=3, epi=0, bias=True, adev=True)
    at, bt = t["A"].to(F32), t["B"].to(F32)
    acct = accumulate(t, "blk")
    GC.verify(t, g, epilogue(t, g, acct, fused=False), kernel="emu")
    bad = acct.clone()
    bad[:, 128:144] += 3 * _seq(at[:, 128:144], bt, 32, 40)
    got = epilogue(t, g, bad, fused=False)
    _caught(t, g, got, ((128, 144), (0, 260)))
    _ratio("clamped tail chunk multiplied (K = 40)", t, g, got)

    # the A / B roles swapped (a square output)
    s = GC.problem(fam, SQUARE)
    g1 = dict(kern="gemm", cfg=0, epi=1)
    accs = accumulate(s, "blk")
    GC.verify(s, g1, epilogue(s, g1, accs), kernel="emu")
    _caught(s, g1, epilogue(s, g1, accs.transpose(1, 2).contiguous()))


def test_guard_band_checker():
    for dt, ity, sent in ((BFT, torch.int16, GC.SENT16), (F32, torch.int32, GC.SENT32)):
        p = GC.Plane(2, 5, 12, dt, "cpu", 16)
        assert p.ld % 8 == 0 and p.ld > 12 and p.t.shape == (2, 5, 12)
        p.verify("fresh", written=False)
        with pytest.raises(GC.Mismatch, match="never written"):
            p.verify("fresh")
        p.t.fill_(1.0)
        p.verify("written")
        init = torch.ones(2, 5, 12)
        p.verify("kept", written=False, initial=init)
        p.t[1, 4, 11] = 2.0
        with pytest.raises(AssertionError, match="payload changed"):
            p.verify("kept", written=False, initial=init)
        p.t[1, 2, 3].view(ity).fill_(sent)
        with pytest.raises(GC.Mismatch, match="never written; first at b=1, m=2, n=3"):
            p.verify("left")
        p.t.fill_(1.0)
        for (r, c), where in (((p.before - 1, p.left), "above row 0"), ((p.before + 5, p.left + 3), "past the last row"),
                              ((p.before, p.left - 1), "left of column 0"), ((p.before + 4, p.left + 12), "right of the last")):
            keep = p.buf[1, r, c].clone()
            p.buf[1, r, c] = 0.0
            with pytest.raises(GC.Mismatch, match=where):
                p.verify("band")
            p.buf[1, r, c] = keep
        p.verify("restored")
    q = GC.Plane(1, 3, 128, GC.F8, "cpu", 24)
    assert q.ld % 16 == 0 and bool(q.buf.to(F32).isnan().all())
