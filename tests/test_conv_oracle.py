"""The conv front-end oracle of tests/conv_cases.py, checked on the CPU:

  * the fp64 oracle equals F.conv2d / F.batch_norm(...).clamp(0, 20) and their autograd;
  * a plain-torch emulation of each kernel's arithmetic (bf16 operands, fp32 accumulation, one
    RNE store) passes the checker on every entry of the case tables, and reproduces family A
    exactly, so the tolerances are not tighter than honest fp32 arithmetic;
  * six planted local errors in a passing emulated output fail at their coordinates, while the
    whole-tensor ratio of tests/test_conv_gpu.py stays under its 1e-2 for the first four.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as CO

F64 = torch.float64
f32 = lambda t: t.to(torch.float32)
bf = lambda t: t.to(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------ emulation
def emu_fwd(which, d):
    if which == 1:
        y = F.conv2d(f32(d["x"]).unsqueeze(1), f32(d["w1"]), None, stride=(2, 2)).permute(0, 2, 3, 1)
        y = bf(y + f32(d["b1"]))
    else:
        y = F.conv2d(f32(d["z1"]).permute(0, 3, 1, 2), f32(d["w2"]), None, stride=(2, 1)).permute(0, 2, 3, 1)
        y = bf(y + f32(d["b2"]))
    v = y.float().reshape(-1, 32)
    return y.contiguous(), torch.stack([v.sum(0), (v * v).sum(0)], 1)


def emu_dgrad(d):
    return bf(CO.conv2_dgrad(f32(d["dy2"]), f32(d["w2"]), d["T1"]))


def emu_apply(y, p, tmaj):
    sc = f32(p["inv"]) * f32(p["gamma"])
    sh = f32(p["beta"]) - f32(p["mean"]) * sc
    z = bf((f32(y) * sc + sh).clamp(0, 20))
    return CO.to_tmaj(z) if tmaj else z


def emu_bwd(dz, y, p, upper_mask_off=None):
    mu, is_, g, bt = (f32(p[k]) for k in ("mean", "inv", "gamma", "beta"))
    xh = (f32(y) - mu) * is_
    zz = xh * g + bt
    m = (zz > 0) & (zz < 20)
    if upper_mask_off is not None:
        m[..., upper_mask_off] = (zz > 0)[..., upper_mask_off]
    dd = f32(dz) * m
    M = y.numel() // 32
    db, dg = dd.reshape(-1, 32).sum(0), (dd * xh).reshape(-1, 32).sum(0)
    dy = bf(g * is_ * (dd - db / M - xh * (dg / M)))
    return dg, db, dy


def _case(fam, c):
    d = CO.make(fam, *c[:3])
    CO.preconditions(d)
    return d


# ------------------------------------------------------------------------------ oracle == torch
def _close(a, b, rel):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize("c", [g for g in CO.geometries() if g[1] <= 44 or g in ((1, 61, 131), (2, 100, 133))],
                         ids=CO.ident)
def test_oracle_matches_torch_autograd(c):
    d = CO.make("B", *c)
    x = d["x"].clone().requires_grad_(True)
    w1 = d["w1"].clone().requires_grad_(True)
    y1 = F.conv2d(x.unsqueeze(1), w1, d["b1"], stride=(2, 2))
    _close(CO.conv1_fwd(d["x"], d["w1"], d["b1"]), y1.detach().permute(0, 2, 3, 1), 1e-12)
    y1.backward(d["dy1"].permute(0, 3, 1, 2))
    _close(CO.conv1_wgrad(d["dy1"], d["x"]), w1.grad, 1e-10)
    z = d["z1"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    w2 = d["w2"].clone().requires_grad_(True)
    y2 = F.conv2d(z, w2, d["b2"], stride=(2, 1))
    _close(CO.conv2_fwd(d["z1"], d["w2"], d["b2"]), y2.detach().permute(0, 2, 3, 1), 1e-12)
    y2.backward(d["dy2"].permute(0, 3, 1, 2))
    _close(CO.conv2_dgrad(d["dy2"], d["w2"], d["T1"]), z.grad.permute(0, 2, 3, 1), 1e-10)
    _close(CO.conv2_wgrad(d["dy2"], d["z1"]), w2.grad, 1e-10)
    # BatchNorm + clip, both layouts, with the exact (unrounded) batch statistics
    for tag, dz in (("1", d["dy1"]), ("2", d["dy2"])):
        y = d["y" + tag]
        mean, var, inv, M = CO.stats(y)
        p = dict(mean=mean, inv=inv, gamma=d["bn" + tag]["gamma"], beta=d["bn" + tag]["beta"])
        yr = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
        g_r, b_r = p["gamma"].clone().requires_grad_(True), p["beta"].clone().requires_grad_(True)
        rm, rv = torch.zeros(32, dtype=F64), torch.ones(32, dtype=F64)
        zr = F.batch_norm(yr, rm, rv, g_r, b_r, training=True, momentum=CO.BN_MOM, eps=CO.BN_EPS).clamp(0, 20)
        zo, _ = CO.bn_apply(y, p)
        _close(zo, zr.detach().permute(0, 2, 3, 1), 1e-12)
        _close(CO.to_tmaj(zo), zr.detach().permute(2, 0, 1, 3).reshape(y.shape[1], y.shape[0], -1), 1e-12)
        wm, wv = CO.running(torch.zeros(32), torch.ones(32), mean, var, M)
        _close(wm, rm, 1e-12)
        _close(wv, rv, 1e-12)
        zr.backward(dz.permute(0, 3, 1, 2))
        o = CO.bn_bwd(dz, y, p)
        _close(o["dbeta"], b_r.grad, 1e-10)
        _close(o["dgamma"], g_r.grad, 1e-10)
        _close(o["dy"], yr.grad.permute(0, 2, 3, 1), 1e-10)
        # the time-major gradient layout is the inverse of the time-major store
        assert torch.equal(CO.from_tmaj(CO.to_tmaj(dz), dz.shape[2]), dz)


# ------------------------------------------------------------------------------ emulation passes
def _cases(table):
    return [pytest.param(fam, c, id=fam + "-" + CO.ident(c)) for c in CO.TABLES[table] for fam in "AB"]


@pytest.mark.parametrize("which,table", [(1, "conv1_fwd"), (2, "conv2_fwd")])
def test_emulated_forward(which, table):
    for fam in "AB":
        for c in CO.TABLES[table]:
            d = _case(fam, c)
            y, ps = emu_fwd(which, d)
            CO.verify_fwd(which, d, y, ps)
            mean, var, inv, M = CO.stats(y)
            CO.verify_finalize(table, y, f32(mean), f32(inv))


@pytest.mark.parametrize("fam,c", _cases("conv2_dgrad"))
def test_emulated_dgrad(fam, c):
    d = _case(fam, c)
    dx = emu_dgrad(d)
    CO.verify_dgrad(d, dx)
    dg, db, _ = emu_bwd(dx, d["y1"], d["bn1"])
    CO.verify_sums("fused sums", fam, dx, d["y1"], d["bn1"], torch.stack([db, dg], 1), "conv2_dgrad sums")


@pytest.mark.parametrize("which,table", [(1, "conv1_wgrad"), (2, "conv2_wgrad")])
def test_emulated_wgrad(which, table):
    for fam in "AB":
        for c in CO.TABLES[table]:
            d = _case(fam, c)
            dw = (CO.conv1_wgrad(f32(d["dy1"]), f32(d["xd"])) if which == 1 else
                  CO.conv2_wgrad(f32(d["dy2d"]), f32(d["z1d"])))
            CO.verify_wgrad(which, d, dw)


def test_emulated_bn():
    for fam in "AB":
        for (n, t, f0, tmaj) in CO.BN_APPLY:
            d = _case(fam, (n, t, f0))
            tag = "2" if tmaj else "1"
            CO.verify_apply("apply", fam, d["y" + tag], d["bn" + tag], emu_apply(d["y" + tag], d["bn" + tag], tmaj),
                            tmaj, "emu")
        for (n, t, f0, tmaj, nb) in CO.BN_BWD:
            d = _case(fam, (n, t, f0))
            tag, dz = ("2", d["dy2d"]) if tmaj else ("1", d["dy1"])
            dg, db, dy = emu_bwd(dz, d["y" + tag], d["bn" + tag])
            CO.verify_bwd("bwd", fam, dz, d["y" + tag], d["bn" + tag], dg, db, dy, "emu")


def test_conditioned_inputs_have_their_ratio():
    for r in CO.STAT_RATIOS:
        x, w, b = CO.conditioned(r)
        mean, var, _, M = CO.stats(bf(CO.conv1_fwd(x, w, b)))
        got = mean.abs() / var.sqrt()
        assert M == 6478 and float((got - r).abs().max()) <= 0.05 * r + 0.05, (r, got)   # bf16 storage adds to the std
        assert float((var.sqrt() - 1).abs().max()) < 0.25


# ------------------------------------------------------------------------------ planted errors
def _fails_at(fn, **where):
    with pytest.raises(CO.Mismatch) as e:
        fn()
    for k, v in where.items():
        assert e.value.coords[k] == v, (k, v, e.value.coords, str(e.value))
    return str(e.value)


def _ulps(y, idx, k):
    """move one bf16 element by k units in the last place"""
    iv = y.view(torch.int16)
    iv[idx] += k


@pytest.mark.parametrize("fam", "AB")
def test_plant_last_position_4_ulps(fam):
    d = CO.make(fam, 3, 100, 163)
    y, ps = emu_fwd(2, d)
    CO.verify_fwd(2, d, y, ps)
    ref = y.clone()
    n, t, c = 1, 7, 13
    _ulps(y, (n, t, d["F2"] - 1, c), 4)
    assert CO.old_ratio(y, ref) < 1e-2
    _fails_at(lambda: CO.verify_fwd(2, d, y, ps), n=n, t=t, f=d["F2"] - 1, c=c)


@pytest.mark.parametrize("fam", "AB")
def test_plant_dropped_tap_in_last_mtile(fam):
    """(kt, kf) = (9, 4) missing for the positions f2 >= 64 of one tile (one output row)"""
    d = CO.make(fam, 3, 100, 163)
    y, ps = emu_fwd(2, d)
    ref = y.clone()
    n, t = 2, 11
    tap = torch.einsum("fi,oi->fo", f32(d["z1"])[n, 2 * t + 9, 64 + 4:d["F2"] + 4], f32(d["w2"])[:, :, 9, 4])
    y[n, t, 64:] = bf(y[n, t, 64:].float() - tap)
    assert bool((y != ref).any())
    assert CO.old_ratio(y, ref) < 1e-2, CO.old_ratio(y, ref)
    msg = _fails_at(lambda: CO.verify_fwd(2, d, y, ps), n=n, t=t)
    with pytest.raises(CO.Mismatch) as e:
        CO.verify_fwd(2, d, y, ps)
    assert e.value.coords["f"] >= 64, msg


@pytest.mark.parametrize("fam", "AB")
def test_plant_nonzero_in_zero_row(fam):
    d = CO.make(fam, 2, 40, 163)          # T1 = 11, T2 = 1: row 10 is read by no output
    dx = emu_dgrad(d)
    CO.verify_dgrad(d, dx)
    ref = dx.clone()
    dx[1, 10, 79, 5] = 2.0 ** -6
    assert CO.old_ratio(dx, ref) < 1e-2
    _fails_at(lambda: CO.verify_dgrad(d, dx), n=1, t=10, f=79, c=5)


@pytest.mark.parametrize("fam", "AB")
def test_plant_upper_mask_ignored_for_one_octet(fam):
    d = CO.make(fam, 2, 100, 163)
    y, p, dz = d["y1"], d["bn1"], d["dy1"]
    dg, db, dy = emu_bwd(dz, y, p)
    CO.verify_bwd("bwd", fam, dz, y, p, dg, db, dy, "emu")
    octet = slice(8, 16)
    dg2, db2, dy2 = emu_bwd(dz, y, p, upper_mask_off=octet)
    # the apply pass alone is wrong (sums as the kernel under test received them)
    with pytest.raises(CO.Mismatch) as e:
        CO.verify_bwd("bwd", fam, dz, y, p, dg, db, emu_bwd_apply_only(dz, y, p, dg, db, octet), "emu")
    assert 8 <= e.value.coords["c"] < 16
    _, zz = CO.bn_zz(y, p)
    co = e.value.coords
    assert float(zz[co["n"], co["t"], co["f"], co["c"]]) >= 20.0
    # the reduce pass wrong: dbeta / dgamma of that octet
    with pytest.raises(CO.Mismatch) as e:
        CO.verify_bwd("bwd", fam, dz, y, p, dg2, db2, None, "emu")
    assert 8 <= e.value.coords["c"] < 16
    # on the inputs tests/test_conv_gpu.py uses (gamma in 0.5..1.5, beta ~ 0.3 randn, y = 3 randn + 1)
    # zz never reaches 20, so the same error changes nothing there: ratio 0 < 2e-2
    g = torch.Generator().manual_seed(3)
    yo = bf(torch.randn(3, 17, 79, 32, generator=g) * 3 + 1).to(F64)
    mean, _, inv, _ = CO.stats(yo)
    po = dict(mean=mean, inv=inv, gamma=(torch.rand(32, generator=g) + 0.5).to(F64),
              beta=(torch.randn(32, generator=g) * 0.3).to(F64))
    dzo = bf(torch.randn(3, 17, 79, 32, generator=g)).to(F64)
    a, b = emu_bwd(dzo, yo, po), emu_bwd(dzo, yo, po, upper_mask_off=octet)
    assert float(CO.bn_zz(yo, po)[1].max()) < 20
    for u, v in zip(a, b):
        assert CO.old_ratio(v, u) < 1e-2


def emu_bwd_apply_only(dz, y, p, dg, db, octet):
    mu, is_, g, bt = (f32(p[k]) for k in ("mean", "inv", "gamma", "beta"))
    xh = (f32(y) - mu) * is_
    zz = xh * g + bt
    m = (zz > 0) & (zz < 20)
    m[..., octet] = (zz > 0)[..., octet]
    M = y.numel() // 32
    return bf(g * is_ * (f32(dz) * m - db / M - xh * (dg / M)))


@pytest.mark.parametrize("fam", "AB")
def test_plant_partial_counted_twice(fam):
    d = CO.make(fam, 2, 61, 161)
    y, ps = emu_fwd(2, d)
    one_wg = CO.part_sums(y[0, 2]).float()         # what the workgroup of one tile contributes
    with pytest.raises(CO.Mismatch) as e:
        CO.verify_fwd(2, d, y, ps + one_wg)
    assert "partials" in str(e.value)


@pytest.mark.parametrize("fam", "AB")
def test_plant_time_major_index_swapped(fam):
    d = CO.make(fam, 2, 100, 163)
    y, p = d["y2"], d["bn2"]
    out = emu_apply(y, p, True)
    CO.verify_apply("apply", fam, y, p, out, True, "emu")
    t, n = 5, 1
    z = emu_apply(y, p, False)
    out[t, n] = z[n, t].reshape(-1)                # feature index f*C + c
    _fails_at(lambda: CO.verify_apply("apply", fam, y, p, out, True, "emu"), t=t, n=n)
