"""Every recurrence kernel family (csrc/rnn_xcd.hip, rnn_fp8.hip forward, rnn_persistent.hip) per
element against the step-local fp64 oracle of tests/rnn_cases.py, whose docstring derives the
bounds: |kernel - oracle| <= max(8 e_ref, floor) for every (direction, step, row, unit) of the saved
state, the gates, dgh, dgx, the bias partials and dU, and the bitwise properties (hx = bf16(hs),
outputs = bf16 of the state, frozen rows, zero padding, dgx / dgh shared columns).

Launches go through ops/rnn.py _run_fwd / _run_bwd / _run_fwd_fp8 on buffers pre-filled with NaN
wherever the launch contract does not ask for an initial value (gates, hs[:, 1:], y2, dgh, dgx), so
an element a kernel leaves unwritten shows. Every case asserts the kernel family its plan launches
through the extension's own dispatch report (kernel_families / fp8_recurrence_ok).

Not covered here: the fp8 BPTT per element. rnnf8_bwd_kernel quantises its fp32 gate gradients to
e4m3 and the observable dgh is their bf16 rounding; re-quantising the bf16 value double-rounds and
rare elements differ by a whole e4m3 ulp, so test_kernels_gpu.py test_fp8_bptt_matches_emulation
stays the check of that kernel. The fp8 forward takes no h0 and no preallocated buffers and serves
only batches its 8-group tiling shares with the bf16 plan, hence its shorter edge list.

Measured on an MI355X: per family and quantity the element that used most of its bound, as kernel
error / e_ref at that element, then the share of max(8 e_ref, floor) it used (each test prints its own
lines with the floor and the coordinates; "edges" rows are the (b) sweeps of that representative; the
whole file, 222 tests, takes 10 s):
  family                        hs              gates           dgh             dgx             bias partials   dU
  rnnq GRU, LDS k-steps         6e-8/1e-10 0.11 2e-7/7e-9 0.16  2e-3/2e-5 0.42  2e-5/1e-6 0.40  1e-3/8e-8 0.03  8e-8/8e-8 0.01
    edges rnnq-gru-1152         7e-8/7e-11 0.10 2e-7/4e-9 0.16  2e-4/3e-5 0.45  2e-4/3e-5 0.45  4e-4/5e-8 0.12  4e-8/7e-9 0.28
    edges rnnq-relu-160         7e-7/2e-7 0.01  -               2e-2/7e-5 0.71  2e-2/7e-5 0.71  5e-3/0 0.52     4e-8/2e-8 0.18
  rnnq ReLU                     4e-7/2e-7 0.06  -               2e-2/3e-3 0.85  2e-2/3e-3 0.85  6e-3/3e-8 0.38  4e-6/2e-7 0.02
    edges rnne-64               6e-8/3e-10 0.11 2e-7/4e-8 0.15  4e-4/6e-5 0.87  4e-4/6e-5 0.87  3e-4/3e-8 0.47  1e-9/6e-10 0.17
  rnne GRU                      6e-8/2e-9 0.11  2e-7/2e-8 0.16  2e-5/2e-6 0.88  2e-5/2e-6 0.88  1e-3/8e-9 0.22  1e-7/8e-8 0.03
  gen 2 small tiles, knob 256   6e-8/2e-9 0.11  2e-7/4e-8 0.15  2e-5/2e-6 0.88  2e-5/2e-6 0.88  6e-3/3e-8 0.38  4e-8/4e-8 0.03
    edges gen2-928              5e-8/1e-10 0.10 2e-7/2e-8 0.16  2e-3/4e-4 0.50  2e-4/4e-5 0.46  3e-4/2e-8 0.16  2e-8/6e-9 0.34
  gen 2 GRU                     6e-8/1e-11 0.12 2e-7/2e-8 0.17  2e-3/4e-4 0.45  3e-3/8e-4 0.43  1e-3/2e-8 0.03  5e-7/2e-7 0.01
    edges rnnw-1056             0/0 0.00        -               3e-2/3e-3 0.59  3e-2/3e-3 0.59  1e-2/1e-7 0.36  1e-7/1e-7 0.06
  rnnw fwd + BPTT (ReLU)        1e-6/2e-7 0.00  -               3e-2/5e-4 0.53  3e-2/5e-4 0.53  1e-2/1e-7 0.26  6e-6/6e-6 0.02
  rnnrs R<=8, bf16 partials     4e-8/3e-11 0.10 2e-7/6e-9 0.15  3e-4/1e-5 0.62  3e-4/1e-5 0.62  1e-2/5e-8 0.24  3e-8/2e-8 0.03
  rnnrs R 9..16, bf16 partials  6e-8/9e-10 0.12 2e-7/1e-8 0.17  2e-2/2e-3 0.62  4e-3/3e-5 0.65  3e-2/5e-8 0.21  9e-7/4e-7 0.02
  rnnrs knob 64, fp32 partials  4e-8/3e-11 0.10 2e-7/6e-9 0.15  1e-4/1e-4 0.13  2e-5/2e-5 0.13  1e-7/3e-8 0.00  3e-8/3e-8 0.03
  rnne / rnnrs, N < R           9e-8/2e-9 0.10  1e-7/1e-8 0.14  2e-5/1e-7 0.70  2e-5/1e-7 0.70  8e-3/1e-7 0.33  8e-9/8e-9 0.03
  gen 1, batch 96 two tiles     6e-8/5e-11 0.12 2e-7/6e-9 0.16  6e-5/6e-5 0.13  5e-4/5e-4 0.13  2e-7/4e-8 0.00  2e-7/6e-8 0.01
    edges gen1-step-64          6e-8/3e-10 0.11 2e-7/4e-8 0.15  9e-6/9e-6 0.12  9e-6/9e-6 0.12  3e-7/7e-8 0.04  1e-8/1e-8 0.05
    edges gen1-64               6e-8/3e-10 0.11 2e-7/4e-8 0.15  9e-6/9e-6 0.12  9e-6/9e-6 0.12  3e-7/7e-8 0.04  1e-8/1e-8 0.05
  gen 1 step launches           7e-8/1e-8 0.10  2e-7/3e-9 0.14  2e-3/2e-3 0.13  2e-3/2e-3 0.13  7e-7/2e-7 0.01  3e-8/1e-10 0.02
  gen 1 persistent              7e-8/9e-10 0.11 2e-7/9e-9 0.15  2e-3/2e-3 0.13  2e-3/2e-3 0.13  7e-7/2e-7 0.01  3e-8/2e-8 0.03
    edges fp8-256 forward       8e-6/8e-9 0.33  6e-6/1e-8 0.59  -               -               -               -
  fp8 forward                   9e-6/2e-8 0.38  2e-5/0 0.46     -               -               -               -
The forward sits at the fp32 evaluation's own error scale, an order under its floor. The bf16-partial
BPTT families (rnnrs, rnnw) sit at 0.4 - 0.9 of a floor that the exchanged partials' rounding decides:
with one producer (H = 32) the kernel's 1.7e-5 against 2.0e-5 shows the tag's extra bf16 ulp
(bf16x2_tagged) is real, the plain-rounding term alone (2^-8) would not hold it. With fp32 partials
(knob 64) and in generation 1 the BPTT is at e_ref. The fp8 forward's scaled MFMA accumulates less
exactly than fp32 FMA chains (8e-6 against an e_ref of 1e-8) and still keeps to the dot-product floor.
"""
import pytest
import torch

import rnn_cases as RC

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _rnn():
    from deepspeech_amd.ops import rnn as RNN
    return RNN


def _exchange(bwd_family, knobs):
    """(producer columns per gate, relative error of one exchanged partial) of a BPTT family
    (tests/rnn_cases.py docstring), None for generation 1."""
    if bwd_family.startswith("rnnrs"):
        return (32, 2 * RC.EPS if knobs & 64 else 3 * RC.BF)
    if bwd_family.startswith("rnnw"):
        return (64, 3 * RC.BF)
    return None


def _dev(c, cuda):
    pad = [None] * (2 - c["ndir"])
    return dict(gx=c["gx"].to(cuda), lens=c["lens"].to(cuda), dy=c["dy"].to(cuda),
                U=[u.to(cuda) for u in c["U"]] + pad,
                bh=[b.to(cuda) if b is not None else None for b in c["bh"]] + pad,
                h0=c["h0"].to(cuda) if c["h0"] is not None else None)


def _report(*reps):
    fails = []
    for r in reps:
        for line in r.lines():
            print(line)
        fails += r.failures
    assert not fails, "\n".join(fails[:6])


def _run_case(cuda, monkeypatch, tag, cell, H, N, T, ndir, mode="auto", knobs=0, min_rows=0, nw=0, lens="edge",
              h0=False, scale=1.0, fwd=None, bwd=None, r_range=None, seed=1):
    """One forward + BPTT launch pair of the plan (cell, H, N, ndir, mode) chooses, checked per
    element. fwd / bwd: the kernel families the plan must launch."""
    RNN = _rnn()
    monkeypatch.setattr(RNN, "RNNX_KNOBS", knobs)
    monkeypatch.setattr(RNN, "_MIN_ROWS", min_rows)
    monkeypatch.setattr(RNN, "_FORCE_NW", nw)
    plan = RNN.make_plan(N, H, cell, ndir, RNN._ext.num_cus(cuda.index or 0), mode)
    fam = RNN.kernel_families(plan)
    assert fam[0].startswith(fwd) and fam[1].startswith(bwd), (tag, fam, plan)
    if nw:
        assert plan.nw == nw, plan
    if r_range is not None:
        assert r_range[0] <= plan.R <= r_range[1], plan
    c = RC.make_case(cell, H, N, T, ndir, seed, lens, h0)
    d = _dev(c, cuda)
    GH = RNN.GATES[cell] * H
    b = RNN._alloc_fwd(T, N, plan, cuda)
    if plan.kind == "xcd":
        RNN._fill_fwd(b, plan)              # the launch contract's regions
    else:
        b.hx[:, 1:] = NAN
    b.hs[:, 1:] = NAN
    if b.gates is not None:
        b.gates.fill_(NAN)
    if b.y2 is not None:
        b.y2.fill_(NAN)
    y, (hx, hs, gates) = RNN._run_fwd(d["gx"], d["lens"], d["U"], d["bh"], plan, h0=d["h0"], bufs=b)
    torch.cuda.synchronize()
    RNN.check_errors()
    dgh = torch.full((ndir, T, plan.NP, GH), NAN, device=cuda, dtype=torch.bfloat16)
    dgx = torch.full((T, N, ndir * GH), NAN, device=cuda, dtype=torch.bfloat16)
    dgx, dgh, parts = RNN._run_bwd(d["dy"], d["lens"], d["U"], hx, hs, gates, plan, ndir * GH, dgx_scale=scale,
                                   dgh=dgh, dgx=dgx)
    torch.cuda.synchronize()
    RNN.check_errors()
    dU = [RNN._dU(dgh, hx, i, plan, None) for i in range(ndir)]
    torch.cuda.synchronize()
    g = gates if cell == "gru" else None
    fw = RC.check_forward(cell, d["gx"], d["lens"], d["U"], d["bh"], hx, hs, g, N, y=y, y2=b.y2, tag=tag)
    bw = RC.check_bptt(cell, d["dy"], d["lens"], d["U"], hs, g, dgh, dgx, parts, N, scale=scale,
                       exchange=_exchange(fam[1], knobs), tag=tag)
    _report(fw, bw, *[RC.check_dU(dU[i], dgh, hx, i, N, tag=tag) for i in range(ndir)])


def _run_fp8(cuda, tag, H, N, T, ndir, lens="edge", seed=2):
    """The fp8 GRU forward: operand e4m3(hs[d, s]), U e4m3 with its power-of-two scale (the
    kernel's own quantisation, read back), the rest as the bf16 forward."""
    RNN = _rnn()
    plan = RNN.make_plan(N, H, "gru", ndir, RNN._ext.num_cus(cuda.index or 0), "auto")
    assert RNN.fp8_recurrence_ok(plan, N), (tag, plan)
    c = RC.make_case("gru", H, N, T, ndir, seed, lens)
    d = _dev(c, cuda)
    keep = {}
    y, (hx, hs, gates) = RNN._run_fwd_fp8(d["gx"], d["lens"], d["U"], d["bh"], plan, keep)
    torch.cuda.synchronize()
    RNN.check_errors()
    U8T, words = keep["quant"]
    Uq = [U8T[i].view(torch.float8_e4m3fn).double().t().contiguous() * 2.0 ** (int(words[i]) - 127) for i in range(ndir)]
    h_op = hs[:, :T, :N].to(torch.float8_e4m3fn).double()
    _report(RC.check_forward("gru", d["gx"], d["lens"], Uq, d["bh"], hx, hs, gates, N, y=y, h_operand=h_op, tag=tag))


# ------------------------------------------------------------------------------------ (a) families
# T = 7, both directions, zero h0, scale 1, the edge batch (lengths T, 0, 1, 2, T-1, T, ...).
# N = 13 gives groups of R = 4 rows with a partial last group (R <= 8: two producers per load in
# rnnrs); N = 33 gives R = 9 (H <= 1024) or 16 (wider), again with a partial last group.
def _sweep():
    S = []

    def add(tag, cell, H, N, fwd, bwd, **kw):
        S.append(pytest.param(dict(tag="%s-%s-%d-N%d" % (tag, cell, H, N), cell=cell, H=H, N=N, fwd=fwd, bwd=bwd, **kw),
                              id="%s-%s-%d-N%d" % (tag, cell, H, N)))

    for H in RC.FWD_RNNE:
        add("rnne", "gru", H, 13, "rnne", "rnnrs")
    for H in RC.FWD_RNNQ_RELU:
        add("rnnq", "rnn_relu", H, 13, "rnnq", "rnnrs")
    for H in RC.FWD_RNNQ_GRU_LDS:
        add("rnnq-lds", "gru", H, 33, "rnnq", "rnnrs")
    for H in RC.FWD_GEN2_GRU:
        add("gen2", "gru", H, 33, "rnnx", "rnnrs")
    for H in RC.FWD_GEN2_SMALL:
        for cell in ("gru", "rnn_relu"):
            add("gen2-knob256", cell, H, 13, "rnnx", "rnnrs", knobs=256)
    for H in RC.WIDE_RELU:
        add("rnnw", "rnn_relu", H, 13, "rnnw", "rnnw")
    for H in RC.BWD_RNNRS:
        for cell in ("gru", "rnn_relu"):
            if cell == "rnn_relu" and H > 1024:
                continue                                    # one-gate layers that wide run rnnw (above)
            f = ("rnne" if H <= 1024 else "rnnx") if cell == "gru" else "rnnq"
            f = "rnnx" if (cell == "gru" and H == 928) else f
            add("rnnrs-R8", cell, H, 13, f, "rnnrs", r_range=(1, 8), min_rows=4 if H > 1024 else 0)
            add("rnnrs-R16", cell, H, 33, f, "rnnrs", r_range=(9, 16))
            # knob 64: fp32 partials, the third exchange form of every unit-tile arm
            add("rnnrs-fp32-partials", cell, H, 13, f, "rnnrs", knobs=64, min_rows=4 if H > 1024 else 0)
    add("rnnrs-fp32-partials-R16", "rnn_relu", 448, 33, "rnnq", "rnnrs", knobs=64)
    add("gen2-knob256", "rnn_relu", 928, 13, "rnnx", "rnnrs", knobs=256)      # the widest one-gate generation-2 tile
    add("rows-below-R", "gru", 64, 5, "rnne", "rnnrs", min_rows=8, r_range=(8, 8))
    for mode, name in (("v1", "rnn_fwd (gen 1, persistent"), ("step", "rnn_fwd (gen 1, step")):
        for cell, H in (("gru", 64), ("rnn_relu", 64), ("rnn_relu", 2048)):
            for nw in (8, 4):
                add("gen1-%s-nw%d" % (mode, nw), cell, H, 13, name, name.replace("fwd", "bwd"), mode=mode, nw=nw)
    # more k-steps-per-wave tiles of the generation-1 template (persistent; both wave counts)
    g1 = "rnn_fwd (gen 1, persistent"
    for cell, H, nw in (("gru", 512, 8), ("gru", 1024, 8), ("gru", 1344, 8), ("gru", 512, 4), ("gru", 1024, 4),
                        ("gru", 1344, 4), ("rnn_relu", 1536, 8), ("rnn_relu", 1024, 4), ("rnn_relu", 1536, 4)):
        add("gen1-v1-nw%d" % nw, cell, H, 13, g1, g1.replace("fwd", "bwd"), mode="v1", nw=nw)
    add("gen1-two-tiles", "gru", 1280, 96, "rnn_fwd (gen 1", "rnn_bwd (gen 1", T=5)
    add("gen1-two-tiles", "rnn_relu", 2048, 96, "rnn_fwd (gen 1", "rnn_bwd (gen 1", T=5)
    return S


@pytest.mark.parametrize("p", _sweep())
def test_family(cuda, monkeypatch, p):
    p = dict(p)
    _run_case(cuda, monkeypatch, p.pop("tag"), p.pop("cell"), p.pop("H"), p.pop("N"), p.pop("T", 7), 2, **p)


def test_two_tile_plan_is_two_tiles(cuda):
    RNN = _rnn()
    for cell, H in (("gru", 1280), ("rnn_relu", 2048)):
        assert RNN.make_plan(96, H, cell, 2, RNN._ext.num_cus(cuda.index or 0), "auto").mt == 2


# every forward instantiation a plan can reach: rnnf8_fwd_kernel at H = 256, 512, 768, rnnf8h_fwd_kernel
# at 1024 and 1280 (1280: N = 16, the batch its one-group bf16 plan and the 8-group fp8 tiling share)
@pytest.mark.parametrize("H,N,ndir", [(H, 16 if H == 1280 else 13, 2) for H in RC.FP8_FWD] +
                         [(256, 15, 1), (1024, 15, 1), (1280, 16, 1)])
def test_family_fp8_forward(cuda, H, N, ndir):
    _run_fp8(cuda, "fp8-%d-d%d" % (H, ndir), H, N, 7, ndir)


# ------------------------------------------------------------------------------------ (b) edges
# one representative per kernel source; N = 19 for the wide GRU (R = 16, a 3-row last group)
REPS = {
    "rnne-64": dict(cell="gru", H=64, N=13, fwd="rnne", bwd="rnnrs"),
    "rnnq-relu-160": dict(cell="rnn_relu", H=160, N=13, fwd="rnnq", bwd="rnnrs"),
    "rnnq-gru-1152": dict(cell="gru", H=1152, N=19, fwd="rnnq", bwd="rnnrs"),
    "gen2-928": dict(cell="gru", H=928, N=13, fwd="rnnx", bwd="rnnrs"),
    "rnnw-1056": dict(cell="rnn_relu", H=1056, N=13, fwd="rnnw", bwd="rnnw"),
    "gen1-64": dict(cell="gru", H=64, N=13, fwd="rnn_fwd (gen 1, persistent", bwd="rnn_bwd (gen 1, persistent", mode="v1"),
    "gen1-step-64": dict(cell="gru", H=64, N=13, fwd="rnn_fwd (gen 1, step", bwd="rnn_bwd (gen 1, step", mode="step"),
}
# T = 1..6: every residue of the BPTT's 3-slot ring and every depth of the forward memory wave's
# prologue and drain; the rest at T = 7
EDGES = {"T%d" % t: dict(T=t) for t in range(1, 7)}
EDGES.update({
    "N1": dict(N=1), "one-direction": dict(ndir=1),
    "all-full": dict(lens="full"), "all-length-1": dict(lens="one"), "all-length-0": dict(lens="zero"),
    "length-minus-2": dict(lens="negative"), "h0": dict(h0=True),
    "scale-0.5": dict(scale=0.5), "scale-sbn": dict(scale="sbn"),
})


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("rep", list(REPS))
def test_edges(cuda, monkeypatch, rep, edge):
    kw = dict(T=7, ndir=2)
    kw.update(REPS[rep])
    kw.update(EDGES[edge])
    if kw.get("scale") == "sbn":
        kw["scale"] = _rnn().sbn_scale()
    _run_case(cuda, monkeypatch, "%s/%s" % (rep, edge), kw.pop("cell"), kw.pop("H"), kw.pop("N"), kw.pop("T"),
              kw.pop("ndir"), seed=3, **kw)


FP8_EDGES = {k: v for k, v in EDGES.items() if k[0] == "T" or k.startswith(("all-", "length-"))}


@pytest.mark.parametrize("edge", list(FP8_EDGES) + ["one-direction"])
def test_edges_fp8_forward(cuda, edge):
    kw = dict(T=7, lens="edge")
    kw.update(FP8_EDGES.get(edge, {}))
    ndir, N = (1, 15) if edge == "one-direction" else (2, 13)
    _run_fp8(cuda, "fp8-256/%s" % edge, 256, N, kw["T"], ndir, lens=kw["lens"], seed=4)
