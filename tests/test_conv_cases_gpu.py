"""Conv front-end kernels (csrc/conv1.hip, conv2.hip, bn_cl.hip) and the NCHW BatchNorm kernels (csrc/bn_act.hip)
per element against the step-local fp64 oracle of tests/conv_cases.py, whose docstring holds the
method, the two input families and every tolerance. Each kernel is called through its binding on
the case tables there; every output and partials buffer sits between guard bands.

Printed (run with -s): CONVSTAT lines, the invstd error of both BatchNorm implementations at the
five conditioning ratios, and the worst err/tol per kernel. profiles/conv_oracle_coverage.md
records them.
"""
import pytest
import torch

import conv_cases as CO

pytestmark = pytest.mark.gpu
F64 = torch.float64
BFT, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(CO.WORST.items()):
        print("CONVWORST %-32s err/tol %.3f" % (k, v))


def _ext():
    from deepspeech_amd.ops import _ext
    return _ext.ext()


def bfd(t, dev):
    return t.to(F32).to(BFT).to(dev).contiguous()


def f32d(t, dev):
    return t.to(F32).to(dev).contiguous()


def bnp(p, dev):
    return [f32d(p[k], dev) for k in ("mean", "inv", "gamma", "beta")]


def G(shape, dtype, dev):
    return CO.Guarded(shape, dtype, dev)


def psum(part, nb):
    """fp64 sum of the workgroup partials [nb][32][2]"""
    return part.t.to(F64).view(nb, 32, 2).sum(0).cpu()


def _finalize(C_, name, y, part, nb, dev, seed):
    g = torch.Generator().manual_seed(seed)
    rm0, rv0 = torch.randn(32, generator=g), torch.rand(32, generator=g) + 0.5
    mean, inv, rm, rv = (G((32,), F32, dev) for _ in range(4))
    rm.t.copy_(rm0)
    rv.t.copy_(rv0)
    M = y.t.numel() // 32
    C_.bn_cl_finalize(part.t, nb, float(M), CO.BN_EPS, mean.t, inv.t, rm.t, rv.t, CO.BN_MOM)
    for b in (mean, inv, rm, rv):
        b.verify(name + " finalize")
    CO.verify_finalize(name, y.t, mean.t, inv.t, rm0, rv0, rm.t, rv.t)


@pytest.mark.parametrize("c", CO.CONV1_FWD, ids=CO.ident)
def test_conv1_fwd(cuda, c):
    C_ = _ext()
    N, T, F0 = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        y = G((N, d["T1"], d["F1"], 32), BFT, cuda)
        nb = int(C_.conv1_fwd_grid(N, d["T1"]))
        part = G((nb * 64,), F32, cuda)
        C_.conv1_fwd(bfd(d["x"], cuda), bfd(d["w1"], cuda), f32d(d["b1"], cuda), y.t, part.t)
        y.verify("conv1_fwd y")
        part.verify("conv1_fwd part")
        CO.verify_fwd(1, d, y.t, psum(part, nb))
        _finalize(C_, "conv1_fwd %s %s" % (fam, CO.ident(c)), y, part, nb, cuda, T)


@pytest.mark.parametrize("c", CO.CONV2_FWD, ids=CO.ident)
def test_conv2_fwd(cuda, c):
    C_ = _ext()
    N, T, F0, grid = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        y = G((N, d["T2"], d["F2"], 32), BFT, cuda)
        part = G((grid * 64,), F32, cuda)
        C_.conv2_fwd(bfd(d["z1"], cuda), bfd(d["w2"], cuda), f32d(d["b2"], cuda), y.t, part.t, grid)
        y.verify("conv2_fwd y")
        part.verify("conv2_fwd part")
        CO.verify_fwd(2, d, y.t, psum(part, grid))
        _finalize(C_, "conv2_fwd %s %s" % (fam, CO.ident(c)), y, part, grid, cuda, T)


@pytest.mark.parametrize("c", CO.CONV2_DGRAD, ids=CO.ident)
def test_conv2_dgrad(cuda, c):
    C_ = _ext()
    N, T, F0, grid = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        name = "conv2_dgrad %s %s" % (fam, CO.ident(c))
        dy, w = bfd(d["dy2"], cuda), bfd(d["w2"], cuda)
        dx = G((N, d["T1"], d["F1"], 32), BFT, cuda)
        C_.conv2_dgrad(dy, w, dx.t, grid)
        dx.verify(name)
        CO.verify_dgrad(d, dx.t)
        # with conv1's BatchNorm-backward sums in the epilogue: the same dx, and partials of every
        # workgroup (idle ones: zeros) over the dx just stored
        p = bnp(d["bn1"], cuda)
        dx2 = G((N, d["T1"], d["F1"], 32), BFT, cuda)
        part = G((grid * 64,), F32, cuda)
        C_.conv2_dgrad(dy, w, dx2.t, grid, bfd(d["y1"], cuda), p[0], p[1], p[2], p[3], part.t)
        dx2.verify(name + " (bn)")
        part.verify(name + " fused partials")
        assert torch.equal(dx2.t, dx.t), name + ": the BatchNorm epilogue changed dx"
        CO.verify_sums(name + " fused sums", fam, dx.t, d["y1"], d["bn1"], psum(part, grid), "conv2_dgrad fused sums")
        # and bn_cl_bwd's finalize over exactly these partials (part_ready = 2: no apply pass)
        dg, db = G((32,), F32, cuda), G((32,), F32, cuda)
        keep = G((N, d["T1"], d["F1"], 32), BFT, cuda)
        C_.bn_cl_bwd(dx.t, bfd(d["y1"], cuda), p[0], p[1], p[2], p[3], part.t, grid, dg.t, db.t, keep.t, False,
                     part_ready=2)
        keep.verify(name + " part_ready=2 dy", written=False)
        CO.verify_bwd(name + " part_ready=2", fam, dx.t.cpu().to(F64), d["y1"], d["bn1"], dg.t, db.t, None,
                      "bn_cl_bwd(part_ready)")


def test_conv2_dgrad_refuses_narrow_rows(cuda):
    """F1 = 64: the host gate answers -42 and launches nothing"""
    C_ = _ext()
    dy = torch.zeros(1, 1, 60, 32, device=cuda, dtype=BFT)
    w = torch.zeros(32, 32, 10, 5, device=cuda, dtype=BFT)
    dx = G((1, 10, 64, 32), BFT, cuda)
    with pytest.raises(RuntimeError, match=r"kernel launch failed in conv2_dgrad \(code -42\)"):
        C_.conv2_dgrad(dy, w, dx.t, 4)
    torch.cuda.synchronize()
    dx.verify("refused conv2_dgrad", written=False)


def test_refusals_name_their_condition(cuda):
    """Three host gates at their smallest shapes: conv1_fwd with an F1 = 97 output against F0 = 161
    (F1 must be (161 - 5) // 2 + 1 = 79), bn_cl_apply on F = 97 > 96, conv2_dgrad at F1 = 64. Each
    raises a RuntimeError that names its own condition, and no buffer, input or output, changes."""
    C_ = _ext()
    vec = [G((32,), F32, cuda) for _ in range(4)]
    x, w1, y1 = G((1, 20, 161), BFT, cuda), G((32, 1, 20, 5), BFT, cuda), G((1, 1, 97, 32), BFT, cuda)
    part = G((int(C_.conv1_fwd_grid(1, 1)) * 64,), F32, cuda)
    ya, za = G((1, 1, 97, 32), BFT, cuda), G((1, 1, 97, 32), BFT, cuda)
    dy, w2, dx = G((1, 1, 60, 32), BFT, cuda), G((32, 32, 10, 5), BFT, cuda), G((1, 10, 64, 32), BFT, cuda)
    calls = {
        "conv1_fwd": (lambda: C_.conv1_fwd(x.t, w1.t, None, y1.t, part.t), r"F1 = \(F0 - 5\) / 2 \+ 1"),
        "bn_cl_apply": (lambda: C_.bn_cl_apply(ya.t, *(v.t for v in vec), za.t, False), r"F <= 96"),
        "conv2_dgrad": (lambda: C_.conv2_dgrad(dy.t, w2.t, dx.t, 4), r"F1 > 64"),
    }
    said = {}
    for name, (call, condition) in calls.items():
        pattern = r"kernel launch failed in %s \(code -\d+\): .*%s" % (name, condition)
        with pytest.raises(RuntimeError, match=pattern) as e:
            call()
        said[name] = str(e.value).split("\n")[0].split("kernel launch failed in ")[1]
    torch.cuda.synchronize()
    texts = [s.split(": ", 1)[1] for s in said.values()]
    codes = [s.split("(code ")[1].split(")")[0] for s in said.values()]
    assert len(set(texts)) == 3 and len(set(codes)) == 3, said
    for b in vec + [x, w1, y1, part, ya, za, dy, w2, dx]:
        b.verify("refused call", written=False)


@pytest.mark.parametrize("c", CO.CONV2_WGRAD, ids=CO.ident)
def test_conv2_wgrad(cuda, c):
    C_ = _ext()
    N, T, F0, grid = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        part = G((int(C_.conv2_wgrad_part_floats(grid)),), F32, cuda)
        dw = G((32, 32, 10, 5), F32, cuda)
        C_.conv2_wgrad(bfd(d["dy2d"], cuda), bfd(d["z1d"], cuda), part.t, dw.t, grid)
        part.verify("conv2_wgrad part")
        dw.verify("conv2_wgrad dw")
        CO.verify_wgrad(2, d, dw.t)


@pytest.mark.parametrize("c", CO.CONV1_WGRAD, ids=CO.ident)
def test_conv1_wgrad(cuda, c):
    C_ = _ext()
    N, T, F0, grid = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        part = G((int(C_.conv1_wgrad_part_floats(grid)),), F32, cuda)
        dw = G((32, 1, 20, 5), F32, cuda)
        C_.conv1_wgrad(bfd(d["dy1"], cuda), bfd(d["xd"], cuda), part.t, dw.t, grid)
        part.verify("conv1_wgrad part")
        dw.verify("conv1_wgrad dw")
        CO.verify_wgrad(1, d, dw.t)


@pytest.mark.parametrize("c", CO.CONV1_WGRAD_BN, ids=CO.ident)
def test_conv1_wgrad_fused_bn_backward(cuda, c):
    """The BatchNorm backward applied in the staging: dw against the oracle's weight gradient of the
    dy that bn_cl_bwd's apply pass stores from the same sums (itself checked here), and bitwise
    the unfused kernel's on that dy."""
    C_ = _ext()
    N, T, F0, grid = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        name = "conv1_wgrad(bn) %s %s" % (fam, CO.ident(c))
        p = bnp(d["bn1"], cuda)
        dz, y1, x = bfd(d["dy1"], cuda), bfd(d["y1"], cuda), bfd(d["xd"], cuda)
        bpart = G((64 * 64,), F32, cuda)
        dg, db = G((32,), F32, cuda), G((32,), F32, cuda)
        dyb = G(tuple(dz.shape), BFT, cuda)
        C_.bn_cl_bwd(dz, y1, p[0], p[1], p[2], p[3], bpart.t, 64, dg.t, db.t, dyb.t, False)
        dyb.verify(name + " dy")
        CO.verify_bwd(name, fam, d["dy1"], d["y1"], d["bn1"], dg.t, db.t, dyb.t, "bn_cl_bwd")
        part = G((int(C_.conv1_wgrad_part_floats(grid)),), F32, cuda)
        dw_a, dw_b = G((32, 1, 20, 5), F32, cuda), G((32, 1, 20, 5), F32, cuda)
        C_.conv1_wgrad(dyb.t, x, part.t, dw_a.t, grid)
        C_.conv1_wgrad(dz, x, part.t, dw_b.t, grid, y1, p[0], p[1], p[2], p[3], db.t, dg.t)
        dw_b.verify(name + " dw")
        assert torch.equal(dw_a.t, dw_b.t), (name, float((dw_a.t - dw_b.t).abs().max()))
        CO.verify_wgrad(1, d, dw_b.t, dy=dyb.t.cpu().to(F64), kernel="conv1_wgrad(bn)")


def test_conv1_unread_samples(cuda):
    """T = 39 leaves frame 38 unread and F0 = 162 leaves bin 161 unread: an input that is nonzero
    only there gives y = bias exactly and a weight gradient of exact zeros (fused and unfused)."""
    C_ = _ext()
    N, T, F0 = 2, 39, 162
    d = CO.make("B", N, T, F0)
    x = torch.zeros(N, T, F0, dtype=F64)
    x[:, 38, :] = 3.0
    x[:, :, 161] = -5.0
    y = G((N, d["T1"], d["F1"], 32), BFT, cuda)
    nb = int(C_.conv1_fwd_grid(N, d["T1"]))
    part = G((nb * 64,), F32, cuda)
    C_.conv1_fwd(bfd(x, cuda), bfd(d["w1"], cuda), f32d(d["b1"], cuda), y.t, part.t)
    y.verify("conv1_fwd")
    want = d["b1"].to(F32).to(BFT).to(F64).expand(N, d["T1"], d["F1"], 32)
    CO.check_equal("conv1_fwd on unread samples", y.t, want, CO.NTFC)
    p = bnp(d["bn1"], cuda)
    dz, y1 = bfd(d["dy1"], cuda), bfd(d["y1"], cuda)
    for grid in (1, 3):
        wp = G((int(C_.conv1_wgrad_part_floats(grid)),), F32, cuda)
        dw = G((32, 1, 20, 5), F32, cuda)
        C_.conv1_wgrad(dz, bfd(x, cuda), wp.t, dw.t, grid)
        dw.verify("conv1_wgrad")
        CO.check_equal("conv1_wgrad on unread samples", dw.t, torch.zeros(32, 1, 20, 5, dtype=F64),
                       ("co", "ci", "kt", "kf"))
        dg, db = f32d(torch.randn(32), cuda), f32d(torch.randn(32), cuda)
        dw2 = G((32, 1, 20, 5), F32, cuda)
        C_.conv1_wgrad(dz, bfd(x, cuda), wp.t, dw2.t, grid, y1, p[0], p[1], p[2], p[3], db, dg)
        CO.check_equal("conv1_wgrad(bn) on unread samples", dw2.t, torch.zeros(32, 1, 20, 5, dtype=F64),
                       ("co", "ci", "kt", "kf"))


@pytest.mark.parametrize("c", CO.BN_APPLY, ids=CO.ident)
def test_bn_cl_apply(cuda, c):
    C_ = _ext()
    N, T, F0, tmaj = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        tag = "2" if tmaj else "1"
        yv, pv = d["y" + tag], d["bn" + tag]
        n, t, f, _ = yv.shape
        out = G((t, n, 32 * f) if tmaj else (n, t, f, 32), BFT, cuda)
        p = bnp(pv, cuda)
        C_.bn_cl_apply(bfd(yv, cuda), p[0], p[1], p[2], p[3], out.t, tmaj)
        name = "bn_cl_apply %s %s" % (fam, CO.ident(c))
        out.verify(name)
        CO.verify_apply(name, fam, yv, pv, out.t, tmaj, "bn_cl_apply_tmaj" if tmaj else "bn_cl_apply")


@pytest.mark.parametrize("c", CO.BN_BWD, ids=CO.ident)
def test_bn_cl_bwd(cuda, c):
    C_ = _ext()
    N, T, F0, tmaj, nb = c
    for fam in "AB":
        d = CO.make(fam, N, T, F0)
        tag, dzv = ("2", d["dy2d"]) if tmaj else ("1", d["dy1"])
        yv, pv = d["y" + tag], d["bn" + tag]
        name = "bn_cl_bwd %s %s" % (fam, CO.ident(c))
        p = bnp(pv, cuda)
        y = bfd(yv, cuda)
        dz = bfd(CO.to_tmaj(dzv) if tmaj else dzv, cuda)
        part = G((nb * 64,), F32, cuda)
        dg, db, dy = G((32,), F32, cuda), G((32,), F32, cuda), G(tuple(yv.shape), BFT, cuda)
        C_.bn_cl_bwd(dz, y, p[0], p[1], p[2], p[3], part.t, nb, dg.t, db.t, dy.t, tmaj)
        for b in (part, dg, db, dy):
            b.verify(name)
        kern = "bn_cl_bwd(tmaj)" if tmaj else "bn_cl_bwd"
        CO.verify_sums(name + " partials", fam, dzv, yv, pv, psum(part, nb), kern + " partials")
        CO.verify_bwd(name, fam, dzv, yv, pv, dg.t, db.t, dy.t, kern)
        if tmaj:
            continue
        # the same partials handed in: no reduce pass (1), no apply pass either (2)
        for ready in (1, 2):
            p2 = part.t.clone()
            dg2, db2, dy2 = G((32,), F32, cuda), G((32,), F32, cuda), G(tuple(yv.shape), BFT, cuda)
            C_.bn_cl_bwd(dz, y, p[0], p[1], p[2], p[3], p2, nb, dg2.t, db2.t, dy2.t, False, part_ready=ready)
            assert torch.equal(p2, part.t), name + ": part_ready rewrote the partials"
            assert torch.equal(dg2.t, dg.t) and torch.equal(db2.t, db.t), (name, ready)
            dy2.verify(name + " part_ready=%d" % ready, written=ready == 1)
            if ready == 1:
                assert torch.equal(dy2.t, dy.t), (name, ready)


@pytest.mark.parametrize("ratio", CO.STAT_RATIOS)
def test_statistics_conditioning(cuda, ratio):
    """One-pass fp32 sums (sum v, sum v^2) of the conv epilogue at |mean|/std = ratio, std ~ 1,
    M = 6478: invstd within 2^-11 relative for ratios <= 8 (asserted; the running statistics
    too). At 32 and 128 the error is printed, beside that of bn_stats (csrc/bn_act.hip, sums
    about a per-channel shift) on the same values in NCHW."""
    C_ = _ext()
    x, w, b = CO.conditioned(ratio)
    N, T, F0 = x.shape
    T1, F1, _, _ = CO.geom(T, F0)
    y = G((N, T1, F1, 32), BFT, cuda)
    nb = int(C_.conv1_fwd_grid(N, T1))
    part = G((nb * 64,), F32, cuda)
    C_.conv1_fwd(bfd(x, cuda), bfd(w, cuda), f32d(b, cuda), y.t, part.t)
    y.verify("conv1_fwd")
    g = torch.Generator().manual_seed(ratio)
    rm0, rv0 = torch.randn(32, generator=g), torch.rand(32, generator=g) + 0.5
    mean, inv, rm, rv = (G((32,), F32, cuda) for _ in range(4))
    rm.t.copy_(rm0)
    rv.t.copy_(rv0)
    C_.bn_cl_finalize(part.t, nb, float(N * T1 * F1), CO.BN_EPS, mean.t, inv.t, rm.t, rv.t, CO.BN_MOM)
    # the NCHW implementation on the same stored values
    yn = y.t.permute(0, 3, 1, 2).contiguous()
    cnb = int(C_.bn_chunks(N, T1, F1))
    mean2, inv2 = G((32,), F32, cuda), G((32,), F32, cuda)
    C_.bn_stats(yn, torch.empty(32 * cnb * 2, device=cuda), CO.BN_EPS, mean2.t, inv2.t, None, None, CO.BN_MOM)
    m64, var, i64, _ = CO.stats(y.t.cpu())
    rel = lambda t: float(((t.cpu().to(F64) - i64).abs() / i64).max())
    print("CONVSTAT ratio %3d (stored %.1f)  bn_cl_finalize invstd rel err %.3e  bn_stats %.3e  mean err %.3e / %.3e" % (
        ratio, float((m64.abs() / var.sqrt()).mean()), rel(inv.t), rel(inv2.t),
        float((mean.t.cpu().to(F64) - m64).abs().max()), float((mean2.t.cpu().to(F64) - m64).abs().max())))
    name = "statistics at |mean|/std = %d" % ratio
    if ratio <= 8:
        CO.verify_finalize(name, y.t, mean.t, inv.t, rm0, rv0, rm.t, rv.t)
        CO.verify_finalize(name + " (bn_stats)", y.t, mean2.t, inv2.t)
    else:
        CO.verify_finalize(name, y.t, mean.t, inv.t, inv_rel=None)


# ------------------------------------------------------------------------------ NCHW BNClip
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BFT], ids=["fp32", "bf16"])
def test_bnclip_nchw(cuda, layout, dtype):
    """ops/frontend.py BNClip (csrc/bn_act.hip) on a clip-saturating input, from the mean / invstd
    its statistics kernel produced."""
    from deepspeech_amd.ops.frontend import BNClip
    N, C, T, Fd = 3, 8, 37, 11
    g = torch.Generator().manual_seed(11 + layout)
    store = "bf16" if dtype == BFT else "f32"
    yv = (2 * torch.randn(N, C, T, Fd, generator=g) + 0.5 * torch.randn(1, C, 1, 1, generator=g)).to(dtype)
    gamma = (8 + 0.5 * torch.randn(C, generator=g)).to(cuda).requires_grad_(True)
    beta = (10 + torch.randn(C, generator=g)).to(cuda).requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.to(cuda), rv0.to(cuda)
    y = yv.to(cuda).requires_grad_(True)
    out = BNClip.apply(y, gamma, beta, rm, rv, True, layout, dtype)
    _, mean, inv, _, _ = out.grad_fn.saved_tensors
    ycl = yv.to(F64).permute(0, 2, 3, 1)
    name = "BNClip layout %d %s" % (layout, store)
    CO.verify_finalize(name, ycl, mean, inv, rm0, rv0, rm, rv)
    p = dict(mean=mean.cpu().to(F64), inv=inv.cpu().to(F64), gamma=gamma.detach().cpu().to(F64),
             beta=beta.detach().cpu().to(F64))
    _, zz = CO.bn_zz(ycl, p)
    assert (zz <= 0).double().mean() >= 0.05 and (zz >= 20).double().mean() >= 0.05
    got = out.detach() if layout == 0 else out.detach().reshape(T, N, C * Fd)
    if layout == 0:
        got = got.permute(0, 2, 3, 1)
    CO.verify_apply(name + " out", "B", ycl, p, got, layout == 1, "bn_apply(nchw)", store=store)
    dzv = torch.randn(N, T, Fd, C, generator=g).to(dtype)
    dout = (CO.to_tmaj(dzv) if layout == 1 else dzv.permute(0, 3, 1, 2)).contiguous().to(cuda)
    out.backward(dout)
    CO.verify_bwd(name, "B", dzv.to(F64), ycl, p, gamma.grad, beta.grad, y.grad.permute(0, 2, 3, 1), "bn_bwd(nchw)",
                  store=store)


# ------------------------------------------------------------------------------ FrontendCL
def _saturate(model):
    """gamma ~ 8, beta ~ 10: both clip regions populated, as in the cases"""
    with torch.no_grad():
        for blk in (model.conv1, model.conv2):
            blk.bn_gamma.fill_(8.0).add_(0.5 * torch.randn(32, device=blk.bn_gamma.device))
            blk.bn_beta.fill_(10.0).add_(torch.randn(32, device=blk.bn_beta.device))


def _models(cuda, bins):
    """fp32 reference model, HIP-engine model, HIP-engine model for the library-conv path"""
    from deepspeech_amd.models import DeepSpeech2
    torch.manual_seed(0)
    kw = dict(num_filters=32, num_hidden=64, num_rnn_layers=1, freq_bins=bins)
    ref = DeepSpeech2(**kw).to(cuda)
    with torch.no_grad():
        for blk in (ref.conv1, ref.conv2):
            blk.bias.normal_(0, 0.1)
            blk.running_mean.normal_(0, 0.2)
            blk.running_var.uniform_(0.5, 1.5)
    out = [ref]
    for _ in range(2):
        m = DeepSpeech2(**kw).to(cuda)
        m.load_state_dict(ref.state_dict())
        m.set_engine("hip", BFT)
        out.append(m)
    return out


def _block(model, name):
    blk = getattr(model, name)
    return {k: getattr(blk, k).detach().cpu().to(F64) for k in ("weight", "bias", "bn_gamma", "bn_beta",
                                                                "running_mean", "running_var")}


def _check_chain(name, feats, z1, out, b1, b2, training):
    """z1 [N,T1,F1,32] from the features; out [T2,N,32*F2] from the tapped z1. b1 / b2: the blocks'
    tensors BEFORE the step. Training: batch statistics (bounded by CO.chained_stats, the
    kernels' own are not exposed); eval: the running statistics."""
    x = feats.detach().cpu().to(F32).to(BFT).to(F64)
    bfv = lambda t: t.to(F32).to(BFT).to(F64)
    for tag, inp, blk, got, conv, K in (("conv1", x, b1, z1, CO.conv1_fwd, 100),
                                        ("conv2", z1.detach().cpu().to(F64), b2, out, CO.conv2_fwd, 1600)):
        w, b = bfv(blk["weight"]), blk["bias"].to(F32).to(F64)
        r = conv(inp, w, b)
        tol_y = CO.tol_bf16(r, conv(inp.abs(), w.abs(), b.abs()), K)
        g, bt = blk["bn_gamma"].to(F32).to(F64), blk["bn_beta"].to(F32).to(F64)
        if training:
            mean, inv, dmean, dinv = CO.chained_stats(r, tol_y)
        else:
            mean = blk["running_mean"].to(F32).to(F64)
            inv = (blk["running_var"].to(F32).to(F64) + CO.BN_EPS).rsqrt().to(F32).to(F64)
            # torch's fp32 rsqrt on the device against the correctly rounded one: 2 ulp
            dmean, dinv = torch.zeros(32, dtype=F64), torch.full((32,), 2.0 ** -22, dtype=F64)
        p = dict(mean=mean, inv=inv, gamma=g, beta=bt)
        # |d(y - mean)| <= tol_y + dmean, then the relative error of invstd on |xh g|
        z, tol = CO.bn_apply(r, p, dy_in=tol_y + dmean)
        tol = tol + ((r - mean) * inv * g).abs() * dinv
        if tag == "conv2":
            z, tol, dims = CO.to_tmaj(z), CO.to_tmaj(tol), ("t", "n", "cf")
        else:
            dims = CO.NTFC
        CO.check("%s %s" % (name, tag), got, z, tol, dims, kernel="FrontendCL " + tag)


def _grads_match_reference(ref, hip, lib, feats, monkeypatch):
    """the tolerances of tests/test_conv_gpu.py::test_frontend_cl_matches_reference"""
    xr = ref.frontend(feats)
    xh = hip.frontend(feats.bfloat16())
    monkeypatch.setenv("DS2_CONV", "lib")
    xl = lib.frontend(feats.bfloat16())
    monkeypatch.delenv("DS2_CONV")
    assert xh.shape == xr.shape and xh.dtype == BFT
    assert CO.old_ratio(xh, xr) < 3e-2, CO.old_ratio(xh, xr)
    g = torch.randn_like(xr).bfloat16().float()      # exact in bf16: the engines read the same gradient
    xr.backward(g)
    xh.backward(g.bfloat16())
    xl.backward(g.bfloat16())
    for name in ("conv1.weight", "conv1.bn_gamma", "conv1.bn_beta", "conv2.weight", "conv2.bn_gamma",
                 "conv2.bn_beta"):
        pr = dict(ref.named_parameters())[name].grad
        ph = dict(hip.named_parameters())[name].grad
        pl = dict(lib.named_parameters())[name].grad
        assert ph is not None, name
        floor = CO.old_ratio(pl, pr)
        assert CO.old_ratio(ph, pr) < max(5e-2, 1.5 * floor), (name, CO.old_ratio(ph, pr), floor)
    assert float(dict(hip.named_parameters())["conv2.bias"].grad.abs().max()) == 0.0
    for blk in ("conv1", "conv2"):
        assert torch.allclose(getattr(hip, blk).running_mean, getattr(ref, blk).running_mean, atol=2e-3, rtol=2e-2), blk


def test_frontend_cl_wiring(cuda):
    """FrontendCL end to end at N = 2, T = 40, 163 bins (F1 = 80, an odd T1, one output row) with
    both clip regions populated: the tapped activations per element, and the parameter gradients
    within the tolerances of tests/test_engine_gpu.py::test_frontend_backward_headline_same_upstream,
    against its float64 reference that stores bf16 where the kernels do. (Against the fp32 engine,
    as tests/test_conv_gpu.py compares, a clip mask that flips under bf16 rounding is a full-size
    gradient error whose relative weight, ~ sqrt(2 P(flip)), does not shrink with the size:
    measured here 5.1 - 5.3 % for conv1.bn_gamma against a library-path floor of 3.2 %, and
    conv1's BN beta gradient cancels far below its terms, as that test's docstring works out.)"""
    from test_engine_gpu import _frontend_emulated
    _, hip, _ = _models(cuda, 163)
    _saturate(hip)
    hip.train()
    hip.capture = True
    feats = torch.randn(2, 40, 163, device=cuda).bfloat16().float()      # exact in bf16
    b1, b2 = _block(hip, "conv1"), _block(hip, "conv2")
    xh = hip.frontend(feats.bfloat16())
    z1, out = hip.act_taps["conv1"], hip.act_taps["conv2"]
    assert tuple(z1.shape) == (2, 11, 80, 32) and tuple(out.shape) == (1, 2, 32 * 76)
    assert torch.equal(out, xh.detach())
    _check_chain("FrontendCL train", feats, z1, out, b1, b2, True)
    dout = ((torch.randn(xh.shape, device=cuda) + 0.3) * 1e-3).to(BFT)
    xh.backward(dout)
    torch.cuda.synchronize()
    mass = {}
    want = _frontend_emulated(hip, feats, dout, mass)
    got = dict(hip.named_parameters())
    errs = {n: CO.old_ratio(got[n].grad.double(), g) for n, g in want.items() if n != "conv1.bn_beta"}
    assert max(errs.values()) < 2e-2, errs
    d = (got["conv1.bn_beta"].grad.double() - want["conv1.bn_beta"]).abs()
    assert bool((d <= 1e-2 * mass["conv1"]).all()), (d / mass["conv1"]).max().item()
    for blk in ("conv1", "conv2"):
        assert float(got[blk + ".bias"].grad.abs().max()) == 0.0      # train-mode BN cancels the bias


def test_frontend_cl_eval(cuda):
    """eval mode: the running statistics, per element"""
    _, hip, _ = _models(cuda, 161)
    _saturate(hip)
    hip.eval()
    hip.capture = True
    feats = torch.randn(2, 61, 161, device=cuda).bfloat16().float()      # exact in bf16
    b1, b2 = _block(hip, "conv1"), _block(hip, "conv2")
    with torch.no_grad():
        out = hip.frontend(feats.bfloat16())
    z1 = hip.act_taps["conv1"]
    assert tuple(z1.shape) == (2, 21, 79, 32) and tuple(out.shape) == (6, 2, 32 * 75)
    _check_chain("FrontendCL eval", feats, z1, out, b1, b2, False)
    for k, v in _block(hip, "conv1").items():
        assert torch.equal(v, b1[k]), "eval changed conv1." + k


def test_129_bins_train_on_the_library_path_and_eval_on_frontend_cl(cuda, monkeypatch):
    """F1 = 63: ds2_conv2_dgrad refuses the width, so a training step must not enter FrontendCL
    (it raised 'kernel launch failed in conv2_dgrad (code -42)' in backward); eval, which runs
    the forward kernels only, still does."""
    from deepspeech_amd.ops import frontend as FE
    ref, hip, lib = _models(cuda, 129)
    feats = torch.randn(2, 61, 129, device=cuda).bfloat16().float()      # exact in bf16
    assert not FE.cl_supported(hip, feats)
    hip.capture = True
    _grads_match_reference(ref, hip, lib, feats, monkeypatch)
    assert tuple(hip.act_taps["conv1"].shape) == (2, 32, 21, 63)          # NCHW: the library path
    _saturate(hip)
    hip.eval()
    assert FE.cl_supported(hip, feats)
    b1, b2 = _block(hip, "conv1"), _block(hip, "conv2")
    with torch.no_grad():
        out = hip.frontend(feats.bfloat16())
    z1 = hip.act_taps["conv1"]
    assert tuple(z1.shape) == (2, 21, 63, 32)                              # channels-last: FrontendCL
    _check_chain("FrontendCL eval 129 bins", feats, z1, out, b1, b2, False)
