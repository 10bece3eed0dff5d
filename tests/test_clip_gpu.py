"""Gradient-norm clipping on the GPU: grad_sumsq, clip_finalize and the CLIP variants of the three
Adam + EMA kernels (csrc/optim.hip) on raw guard-banded buffers, then the Trainer schedules.
Definition: ops/reference.py (clip_from_sumsq, clipped_adam_ref); buffers, Adam oracle and bounds:
tests/stream_cases.py.

grad_sumsq bound. A segment's partial is, per lane, a chain of 16 fmas (4 float4 groups x 4
elements; fma(t, t, acc) rounds once, t = fl32(g gscale) is the oracle's own operand), then the
6 levels of the wave butterfly and 2 levels across the four waves: 24 correctly rounded
operations on non-negative terms, so |part - S_seg| <= ((1 + u)^24 - 1) S_seg < 25 u S_seg with
u = 2^-24, per segment; their fp64 sum against the fp64 total carries the same factor.
clip_finalize sums the partials in fp64 (error ~ nseg 2^-53, far below half an fp32 ulp) and
rounds once: |S - sum| <= u (1 + 2^-20) sum. norm and coef are then exact functions of that S.
"""
import copy

import pytest
import torch

import stream_cases as SC
from stream_cases import BFT, EPS, F32, F64, I32, TINY, Band

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from deepspeech_amd.ops import _ext  # noqa: E402
from deepspeech_amd.ops import reference as R  # noqa: E402

DEV = torch.device("cuda:0")
INF = float("inf")
# words of the clipping state
S_, NORM_, COEF_, BAD_, STEPS_, CLIPPED_, SKIPPED_ = range(7)


@pytest.fixture(scope="module")
def C():
    return _ext.ext()


@pytest.fixture(scope="module")
def SEG(C):
    seg = int(C.grad_sumsq_segment())
    assert seg == 4096                                   # 4 float4 groups per lane of 256
    return seg


def _sizes(seg):
    return (1, 3, 4, 5, seg - 1, seg, seg + 1, 2 * seg + 5, (1 << 20) + 3)


def _grad(n, seed=None):
    return torch.randn(n, generator=SC._g(n if seed is None else seed), dtype=F32)


def _state(vals=None):
    st = Band(8, F32, DEV).put(torch.zeros(8))
    if vals is not None:
        st.t.copy_(vals)
    return st


def _read(st):
    f = st.values()
    i = f.view(I32)
    return dict(S=float(f[S_]), norm=float(f[NORM_]), coef=float(f[COEF_]), bad=int(i[BAD_]), steps=int(i[STEPS_]),
                clipped=int(i[CLIPPED_]), skipped=int(i[SKIPPED_]), spare=int(i[7]))


def _sumsq(C, g, gscale, seg, max_grid=0, nontemporal=False):
    """partials of one launch on guard-banded buffers (g checked read-only, guards intact)"""
    n = g.numel()
    G, part = Band(n, F32, DEV).put(g), Band(SC.cdiv(n, seg), F32, DEV)
    snap = G.payload()
    C.grad_sumsq(G.t, gscale, part.t, max_grid, nontemporal)
    torch.cuda.synchronize()
    G.verify("grad_sumsq n=%d: g" % n)
    part.verify("grad_sumsq n=%d: part" % n)
    G.same("grad_sumsq n=%d: g (read-only)" % n, snap)
    part.written("grad_sumsq n=%d: part" % n)
    return part


# ------------------------------------------------------------------------------ grad_sumsq
@pytest.mark.parametrize("k", range(9))
@pytest.mark.parametrize("gscale", [1.0, SC.GSCALES[2]])
def test_sumsq_partials(C, SEG, k, gscale):
    """every segment's partial against its fp64 sum, the total likewise, and the partials bitwise
    the same whatever the grid (1 block, 7 blocks, the default cap) and the load flavour"""
    n = _sizes(SEG)[k]
    g = _grad(n)
    parts = {mg: _sumsq(C, g, gscale, SEG, mg).values() for mg in (1, 7, 0)}
    parts["nt"] = _sumsq(C, g, gscale, SEG, 0, True).values()
    for key, p in parts.items():
        assert torch.equal(p, parts[0]), "n=%d: partials differ between grid cap %s and the default" % (n, key)
    x = (g * torch.tensor(gscale, dtype=F32)).to(F64)
    nseg = SC.cdiv(n, SEG)
    sq = torch.zeros(nseg * SEG, dtype=F64)
    sq[:n] = x * x
    want = sq.view(nseg, SEG).sum(1)
    SC.check_vals("grad_sumsq n=%d gscale=%g: partials" % (n, gscale), parts[0], want, 25 * EPS * want + TINY, "grad_sumsq")
    S = want.sum().reshape(1)
    SC.check_vals("grad_sumsq n=%d gscale=%g: sum" % (n, gscale), parts[0].to(F64).sum().reshape(1), S, 25 * EPS * S + TINY)


def test_sumsq_does_not_depend_on_neighbours(C, SEG):
    """a segment's partial is a function of its own elements: the same values at another segment
    index, beside other data and under another grid give the same bits"""
    g = _grad(3 * SEG + 7)
    a = _sumsq(C, g, 0.5, SEG).values()
    h = g.clone()
    h[:SEG] = g[SEG:2 * SEG]
    h[SEG:2 * SEG] = g[:SEG]
    b = _sumsq(C, h, 0.5, SEG, 2).values()
    assert torch.equal(a[[1, 0, 2, 3]], b)


# ------------------------------------------------------------------------------ clip_finalize
def _measure(C, g, gscale, max_norm, seg, st=None):
    part = _sumsq(C, g, gscale, seg)
    st = st or _state()
    ps = part.payload()
    C.clip_finalize(part.t, max_norm, st.t)
    torch.cuda.synchronize()
    st.verify("clip_finalize: state")
    part.verify("clip_finalize: part")
    part.same("clip_finalize: part (read-only)", ps)
    return st, part.values()


@pytest.mark.parametrize("k", range(9))
def test_finalize_is_the_definition_applied_to_its_own_sum(C, SEG, k):
    n = _sizes(SEG)[k]
    g = _grad(n)
    gscale = SC.GSCALES[1]
    norm64 = float(((g * torch.tensor(gscale, dtype=F32)).to(F64) ** 2).sum().sqrt())
    st = _state()
    steps = clipped = 0
    for max_norm in (norm64 / 2, norm64 * 2, INF, 400.0, SC.f32r(norm64 / 3)):
        st, part = _measure(C, g, gscale, max_norm, SEG, st)
        r = _read(st)
        tot = float(part.to(F64).sum())
        print("CLIP n=%d C=%g: S=%.9g norm=%.9g coef=%.9g" % (n, max_norm, r["S"], r["norm"], r["coef"]))
        assert abs(r["S"] - tot) <= EPS * (1 + 2.0 ** -20) * tot, (r["S"], tot)
        norm, coef, bad = R.clip_from_sumsq(r["S"], max_norm)
        assert (r["norm"], r["coef"], r["bad"]) == (norm, coef, 0) and not bad
        steps += 1
        clipped += int(norm > SC.f32r(max_norm))
        assert (coef < 1.0) == (norm > SC.f32r(max_norm))
        assert (r["steps"], r["clipped"], r["skipped"], r["spare"]) == (steps, clipped, 0, 0)
    assert clipped >= 2


def test_finalize_selects_one_at_the_threshold_and_for_a_zero_gradient(C, SEG):
    g = torch.zeros(SEG + 9)
    g[0], g[SEG + 8] = 3.0, 4.0                           # S = 25 exactly, in two segments (one in the scalar tail)
    st, _ = _measure(C, g, 1.0, 5.0, SEG)
    r = _read(st)
    assert (r["S"], r["norm"], r["coef"], r["bad"], r["clipped"]) == (25.0, 5.0, 1.0, 0, 0)
    below = float(torch.nextafter(torch.tensor(5.0), torch.tensor(0.0)))
    st, _ = _measure(C, g, 1.0, below, SEG, st)
    r = _read(st)
    assert r["coef"] == R.clip_from_sumsq(25.0, below)[1] < 1.0 and r["clipped"] == 1
    st, _ = _measure(C, torch.zeros(5), 1.0, 1e-30, SEG, st)
    r = _read(st)
    assert (r["S"], r["norm"], r["coef"], r["bad"], r["steps"], r["clipped"]) == (0.0, 0.0, 1.0, 0, 3, 1)
    for bad_c in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError):
            C.clip_finalize(torch.zeros(1, device=DEV), bad_c, st.t)


def test_overflowing_sum_is_a_bad_step(C, SEG):
    """finite gradients whose squares pass the fp32 range: 1e20 in one element, and partials that
    only overflow when summed"""
    g = _grad(SEG + 1)
    g[17] = 1e20
    assert _read(_measure(C, g, 1.0, INF, SEG)[0])["bad"] == 1
    # x = 2^57: every partial is 4096 * 2^114 = 2^126 exactly; two of them sum to 2^127 (finite,
    # norm = fl32(2^63.5)), four to 2^128, past the fp32 range although every partial is finite
    g = torch.full((2 * SEG,), 2.0 ** 57, dtype=F32)
    st, part = _measure(C, g, 1.0, 1.0, SEG)
    r = _read(st)
    assert part.tolist() == [2.0 ** 126] * 2 and (r["S"], r["bad"]) == (2.0 ** 127, 0)
    assert r["norm"] == SC.f32r(2.0 ** 63.5) and r["coef"] == R.clip_from_sumsq(2.0 ** 127, 1.0)[1] > 0
    g = torch.full((4 * SEG,), 2.0 ** 57, dtype=F32)
    st, part = _measure(C, g, 1.0, 1.0, SEG, st)
    r = _read(st)
    assert part.tolist() == [2.0 ** 126] * 4
    assert (r["bad"], r["coef"], r["steps"], r["skipped"]) == (1, 0.0, 2, 1) and r["S"] == INF


# ------------------------------------------------------------------------------ clipped Adam + EMA
FORMS = (("strided", dict(max_grid=3)), ("chunk", dict(max_grid=-7)), ("ranges", dict(ranges="sixty-four")))
OPTS = (dict(), dict(ema=False), dict(p16=False), dict(ema=False, p16=False), dict(hyper=True),
        dict(hyper=True, ema=False, gscale=SC.GSCALES[2]))
N_ADAM = SC.ARENA + 3                                    # the ranges lie inside [0, ARENA); 3 tail elements


def _run_adam(C, form, opt, clip, zero_m=False, n=N_ADAM, g=None):
    """One launch of a form on guard-banded arrays with the state `clip` (a Band, or None for the
    unclipped kernel). Returns (bands, snapshots, inputs, element mask)."""
    inp = dict(SC.adam_inputs(n))
    if zero_m:
        inp["m"] = torch.zeros(n)
    if g is not None:
        inp["g"] = g
    use_e, use_16 = opt.get("ema", True), opt.get("p16", True)
    B = {k: Band(n, F32, DEV).put(inp[k]) for k in ("pgmve" if use_e else "pgmv")}
    if use_16:
        B["h"] = Band(n, BFT, DEV)
    snap = {k: b.payload() for k, b in B.items()}
    lr, keep, hyper = SC.HYP["lr_t"], SC.HYP["keep"], None
    if opt.get("hyper"):
        hyper = torch.tensor([lr, keep], dtype=F32, device=DEV)
        lr = keep = float("nan")
    args = (B["p"].t, B["g"].t, B["m"].t, B["v"].t, B["e"].t if use_e else None, B["h"].t if use_16 else None)
    hy = (SC.HYP["b1"], SC.HYP["b2"], SC.HYP["eps"], opt.get("gscale", SC.GSCALES[1]), keep)
    mask = torch.ones(n, dtype=torch.bool)
    cs = clip.payload() if clip is not None else None
    if "ranges" in form:
        mask[:] = False
        for lo, hi in SC.ADAM_RANGES[form["ranges"]]:
            mask[lo:hi] = True
        C.adam_ema_ranges(*args, [x for r in SC.ADAM_RANGES[form["ranges"]] for x in r], lr, *hy, hyper,
                          None if clip is None else clip.t)
    else:
        skip = None if form.get("skip") is None else torch.tensor([form["skip"]], dtype=I32, device=DEV)
        C.adam_ema(*args, lr, *hy, skip, form["max_grid"], hyper, form.get("lds", 0), None if clip is None else clip.t)
    torch.cuda.synchronize()
    for k, b in B.items():
        b.verify("clipped adam %s: %s" % (form, k))
    B["g"].same("clipped adam: g (read-only)", snap["g"])
    if clip is not None:
        clip.verify("clipped adam: state")
        clip.same("clipped adam: state (read-only)", cs)
    for k, b in B.items():
        b.same("clipped adam %s: %s outside the ranges" % (form, k), snap[k], ~mask)
    return B, snap, inp, mask


def _clip_state(coef, bad=0):
    v = torch.zeros(8, dtype=F32)
    v[S_], v[NORM_], v[COEF_] = 1.0, 1.0, coef
    v.view(I32)[BAD_] = bad
    v.view(I32)[STEPS_] = 5
    return _state(v)


@pytest.mark.parametrize("opt", OPTS, ids=lambda o: "-".join(sorted(o)) or "all")
@pytest.mark.parametrize("fname,form", FORMS)
def test_clipped_adam_per_element(C, fname, form, opt):
    coef = SC.f32r(0.37)
    gscale = opt.get("gscale", SC.GSCALES[1])
    name = "clipped adam %s %s" % (fname, opt)
    B, snap, inp, mask = _run_adam(C, form, opt, _clip_state(coef))
    # the kernel's operand g' = fl32(fl32(g gscale) coef), by torch fp32 ops; the unclipped oracle on it
    gp = (inp["g"] * torch.tensor(gscale, dtype=F32)) * torch.tensor(coef, dtype=F32)
    want, tol = SC.adam_oracle(dict(inp, g=gp), 1.0)
    got = {k: B[k].values() for k in B}
    for k in "mvp":
        SC.check_vals("%s: %s" % (name, k), got[k], want[k], tol[k], "clipped adam " + k, mask)
    if "e" in B:
        we, te = SC.ema_oracle(inp["e"], got["p"])
        SC.check_vals(name + ": ema", got["e"], we, te, "clipped adam ema", mask)
    if "h" in B:
        B["h"].written(name + ": p16", mask)
        SC.check_bf16(name + ": p16 against RNE of the stored p", got["h"], got["p"], mask)
    # m after one step from zero: exactly fl32((1 - b1) g')
    B0, _, _, _ = _run_adam(C, form, opt, _clip_state(coef), zero_m=True)
    one_minus = torch.tensor(1.0, dtype=F32) - torch.tensor(SC.HYP["b1"], dtype=F32)
    m_want = one_minus * gp
    m_got = B0["m"].values()
    nan = torch.isnan(m_want)
    assert bool((torch.isnan(m_got) == nan)[mask].all())
    assert torch.equal(torch.where(nan | ~mask, torch.zeros(()), m_got), torch.where(nan | ~mask, torch.zeros(()), m_want)), name
    # coef == 1: every array bitwise the unclipped kernel's
    B1, _, _, _ = _run_adam(C, form, opt, _clip_state(1.0))
    Bu, _, _, _ = _run_adam(C, form, opt, None)
    SC.same_forms(name + " coef = 1 against unclipped", {k: b.payload() for k, b in Bu.items()}, {k: b.payload() for k, b in B1.items()})
    # and the three forms agree bitwise on the clipped update where both write
    if fname != "strided":
        Bs, _, _, _ = _run_adam(C, FORMS[0][1], opt, _clip_state(coef))
        for k in B:
            a, b = Bs[k].payload(), B[k].payload()
            assert torch.equal(a[mask], b[mask]), "%s: %s differs from the strided form" % (name, k)


def test_clipped_adam_with_lds_reserve_and_skip_word(C):
    """lds_reserve and the skip word keep working with the state: the reserving launch is bitwise
    the plain clipped one (capped or not), skip = 1 writes nothing, skip = 0 changes nothing"""
    st = _clip_state(SC.f32r(0.37))
    a = {k: b.payload() for k, b in _run_adam(C, dict(max_grid=0), {}, st)[0].items()}
    for form in (dict(max_grid=0, lds=32768), dict(max_grid=3, lds=32768), dict(max_grid=3, skip=0)):
        b = {k: x.payload() for k, x in _run_adam(C, form, {}, st)[0].items()}
        SC.same_forms("clipped adam %s" % form, a, b)
    B, snap, _, _ = _run_adam(C, dict(max_grid=3, skip=1), {}, st)
    for k, b in B.items():
        b.same("clipped adam under skip = 1: %s" % k, snap[k])


@pytest.mark.parametrize("poison", [float("nan"), INF, -INF])
@pytest.mark.parametrize("where", ["first", "last float4", "scalar tail"])
def test_poisoned_gradient_skips_every_update(C, SEG, poison, where):
    n = N_ADAM
    at = {"first": 0, "last float4": 4 * (n // 4 - 1) + 2, "scalar tail": n - 1}[where]
    g = _grad(n, 77)
    st, _ = _measure(C, g, 0.5, 1.0, SEG)
    g[at] = poison
    st, _ = _measure(C, g, 0.5, 1.0, SEG, st)
    r = _read(st)
    assert (r["bad"], r["coef"], r["steps"], r["clipped"], r["skipped"]) == (1, 0.0, 2, 1, 1), r
    assert not torch.isfinite(torch.tensor(r["norm"]))
    for fname, form in FORMS:
        B, snap, _, _ = _run_adam(C, form, dict(gscale=0.5), st, g=g)
        for k, b in B.items():
            b.same("bad step, %s: %s" % (fname, k), snap[k])
    g[at] = 0.0                                            # recovery: the flag is rewritten, not sticky
    r = _read(_measure(C, g, 0.5, 1.0, SEG, st)[0])
    assert (r["bad"], r["steps"], r["clipped"], r["skipped"]) == (0, 3, 2, 1) and 0 < r["coef"] < 1


def test_bindings_refuse_bad_arguments(C, SEG):
    g = Band(SEG + 5, F32, DEV).put(_grad(SEG + 5))
    st = _state()
    for what, thunk in (("a short part", lambda: C.grad_sumsq(g.t, 1.0, torch.zeros(1, device=DEV))),
                        ("a misaligned g", lambda: C.grad_sumsq(g.t[1:], 1.0, torch.zeros(2, device=DEV))),
                        ("a host part", lambda: C.grad_sumsq(g.t, 1.0, torch.zeros(2))),
                        ("a short state", lambda: C.clip_finalize(torch.zeros(2, device=DEV), 1.0, st.t[:4])),
                        ("an int state", lambda: C.clip_finalize(torch.zeros(2, device=DEV), 1.0, st.t.view(I32))),
                        ("a host clip", lambda: _run_adam(C, FORMS[0][1], {}, Band(8, F32, "cpu").put(torch.zeros(8))))):
        with pytest.raises(RuntimeError):
            thunk()
    torch.cuda.synchronize()
    g.verify("refusals: g")
    st.verify("refusals: state")


# ------------------------------------------------------------------------------ Trainer schedules
MODES = {"eager": dict(), "defer_update": dict(defer_update=True), "step_graphs": dict(step_graphs=True, graph_warmup=1),
         "force_buckets": dict(force_buckets=True)}
STEPS = 8


@pytest.fixture(scope="module")
def world():
    """the 3 x BiGRU-256 model and its batches (tests/test_defer_update_gpu.py), and a process group
    of one rank for force_buckets"""
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.parallel.dist import init_distributed, shutdown
    ctx = init_distributed("cuda", force_group=True)
    torch.manual_seed(1)
    base = DeepSpeech2(num_filters=32, num_hidden=256, num_rnn_layers=3, cell="gru").to(DEV)
    feed = FixedShapeBatches(8, max_frames=300, seed=300, pool=2)
    batches = [to_device(feed.next(), DEV) for _ in range(2)]
    yield base, batches
    shutdown(ctx)               # later GPU tests must not run with a live RCCL group


_RUNS = {}


def _run(world, mode, max_grad_norm, steps=STEPS, cache=True):
    """losses, the six state tensors, the clip statistics and m after step 0 of one trajectory"""
    from deepspeech_amd.trainer import LRSchedule, Trainer
    key = (mode, max_grad_norm, steps)
    if cache and key in _RUNS:
        return _RUNS[key]
    base, batches = world
    tr = Trainer(copy.deepcopy(base).set_engine("hip", torch.bfloat16), LRSchedule(1e-3, 3, 0.5),
                 max_grad_norm=max_grad_norm, **MODES[mode])
    out = dict(losses=[], pending=None, first=None)
    for i in range(steps):
        out["losses"].append(float(tr.step(batches[i % 2])))
        if i == 0:
            out["pending"] = tr.arena.has_pending_update()
            if max_grad_norm:
                tr.flush()
                torch.cuda.synchronize()
                out["first"] = dict(m=tr.opt.m.clone(), g=tr.arena.grad.clone(), stats=tr.opt.clip_stats())
    tr.flush()
    torch.cuda.synchronize()
    out["state"] = [t.clone() for t in (tr.arena.flat, tr.arena.grad, tr.opt.m, tr.opt.v, tr.opt.ema, tr.arena.p16)]
    out["stats"] = tr.opt.clip_stats() if max_grad_norm else None
    out["graphs"] = len(tr._graphs)
    if cache:
        _RUNS[key] = out
    return out


def _same(a, b, what):
    assert a["losses"] == b["losses"], (what, a["losses"], b["losses"])
    for name, x, y in zip(("flat", "grad", "m", "v", "ema", "p16"), a["state"], b["state"]):
        assert torch.equal(x, y), "%s: %s differs, max %g" % (what, name, float((x.float() - y.float()).abs().max()))


@pytest.mark.parametrize("mode", list(MODES))
def test_huge_threshold_is_bitwise_the_flag_off(world, mode):
    off, on = _run(world, mode, 0.0), _run(world, mode, 1e30)
    _same(off, on, mode + ": max_grad_norm=1e30 against off")
    st = on["stats"]
    assert (st["steps"], st["clipped_steps"], st["skipped_steps"], st["clip_coef"], st["bad"]) == (STEPS, 0, 0, 1.0, 0)
    assert (on["graphs"] >= 1) == (mode == "step_graphs")
    if mode == "defer_update":
        assert on["pending"]


@pytest.fixture(scope="module")
def half_norm(world):
    """half the first step's measured norm: every step of these trajectories clips"""
    n0 = _run(world, "eager", INF, steps=1)["stats"]["grad_norm"]
    assert n0 > 0
    return SC.f32r(n0 / 2)


@pytest.mark.parametrize("mode", list(MODES))
def test_clipping_schedules_agree_bitwise(world, half_norm, mode):
    ref, run = _run(world, "eager", half_norm), _run(world, mode, half_norm)
    print("CLIPRUN %s: C=%g losses %s stats %s" % (mode, half_norm, run["losses"], run["stats"]))
    st = run["stats"]
    assert st["clipped_steps"] == st["steps"] == STEPS and st["skipped_steps"] == 0 and 0 < st["clip_coef"] < 1
    assert run["pending"] == (mode == "defer_update")      # the carried update survives clipping
    assert (run["graphs"] >= 1) == (mode == "step_graphs")     # replayed, not only captured: see _run
    # after step 0 from fresh moments: m = (1 - b1) (g coef), from the arena's gradient and the device's coef
    f = run["first"]
    coef = torch.tensor(f["stats"]["clip_coef"], dtype=F32, device=DEV)
    one_minus = torch.tensor(1.0, dtype=F32, device=DEV) - torch.tensor(0.9, dtype=F32, device=DEV)
    assert 0 < float(coef) < 1 and abs(f["stats"]["grad_norm"] * float(coef) - half_norm) <= 4 * EPS * half_norm
    assert torch.equal(f["m"], one_minus * (f["g"] * coef)), mode
    _same(ref, run, mode + " against eager, clipping every step")
    assert ref["losses"] != _run(world, "eager", 0.0)["losses"]


def test_clipped_run_repeats_bitwise(world, half_norm):
    _same(_run(world, "defer_update", half_norm), _run(world, "defer_update", half_norm, cache=False), "second run")
