"""The recurrence oracle of tests/rnn_cases.py checked on the CPU: it is the reference recurrence
(ops/reference.py) in float64, its BPTT is torch autograd of that scan, and its per-element checker
sees the localised errors a whole-tensor norm ratio hides."""
import math

import pytest
import torch

import rnn_cases as RC

from deepspeech_amd.ops import reference as R

F64 = torch.float64
CASE_IDS = ["%s-H%d-N%d-T%d-d%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "-h0" if c[6] else "") for c in RC.CPU_CASES]


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _case(p, seed=1):
    cell, H, N, T, ndir, lens, h0 = p
    return RC.make_case(cell, H, N, T, ndir, seed, lens, h0)


@pytest.mark.parametrize("p", RC.CPU_CASES, ids=CASE_IDS)
def test_forward_oracle_is_the_reference_scan(p):
    """cell_step chained from its own output in float64, without operand rounding, against
    ops/reference.py: recurrent_scan per direction (nonzero h0 included: outputs and final state)
    and birnn_ref for the direction sum from zero state, to 1e-12."""
    c = _case(p)
    cell, H, T, ndir, lens = c["cell"], c["H"], c["T"], c["ndir"], c["lens"]
    GH = RC.GATES[cell] * H
    gx = c["gx"].to(F64)
    U = [u.to(F64) for u in c["U"]]
    bh = [b.to(F64) if b is not None else None for b in c["bh"]]
    h0 = c["h0"].to(F64) if c["h0"] is not None else None
    _, hs, _, y2 = RC.forward_chain(cell, gx, lens, U, bh, h0, F64, False)
    for d in range(ndir):
        gxd = gx[..., d * GH:(d + 1) * GH]
        if d == 1:
            gxd = R.reverse_sequence(gxd, lens)
        out, hfin = R.recurrent_scan(cell, gxd, U[d], bh[d], lens, h0[d] if h0 is not None else None)
        if d == 1:
            out = R.reverse_sequence(out, lens)
        assert float((y2[d] - out).abs().max()) <= 1e-12
        assert float((hs[d, T] - hfin).abs().max()) <= 1e-12
    if h0 is None:
        want = R.birnn_ref(cell, gx[..., :GH], gx[..., GH:] if ndir == 2 else None, U[0], U[1] if ndir == 2 else None,
                           bh[0], bh[1] if ndir == 2 else None, lens, mm_dtype=None)
        assert float((y2.sum(0) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("p", RC.CPU_CASES, ids=CASE_IDS)
def test_bptt_oracle_is_autograd_of_the_scan(p):
    """The BPTT oracle fed its own unrounded dgh against torch autograd of the float64 scan:
    dgx, dU, dbh and dh0 to 1e-10."""
    c = _case(p, seed=2)
    cell, H, N, T, ndir, lens = c["cell"], c["H"], c["N"], c["T"], c["ndir"], c["lens"]
    GH = RC.GATES[cell] * H
    gx = c["gx"].to(F64).requires_grad_(True)
    U = [u.to(F64).requires_grad_(True) for u in c["U"]]
    bh = [b.to(F64).requires_grad_(True) if b is not None else None for b in c["bh"]]
    h0 = (c["h0"] if c["h0"] is not None else torch.zeros(ndir, N, H)).to(F64).requires_grad_(True)
    dy = c["dy"].to(F64)
    y = 0
    for d in range(ndir):
        gxd = gx[..., d * GH:(d + 1) * GH]
        if d == 1:
            gxd = R.reverse_sequence(gxd, lens)
        out, _ = R.recurrent_scan(cell, gxd, U[d], bh[d], lens, h0[d])
        y = y + (R.reverse_sequence(out, lens) if d == 1 else out)
    (y * dy).sum().backward()
    with torch.no_grad():
        _, hs, gates, _ = RC.forward_chain(cell, gx, lens, U, bh, h0, F64, False)
        got = RC.bptt(cell, dy, lens, U, hs, gates, N, F64, feed="own")
        ar = torch.arange(N)
        for d in range(ndir):
            t_idx, act = RC.time_index(lens, T, d)
            dgx = torch.zeros(T, N, GH, dtype=F64)
            dgx[t_idx[act], ar.expand(T, N)[act]] = got[d]["gxs"][act]
            assert float((dgx - gx.grad[..., d * GH:(d + 1) * GH]).abs().max()) <= 1e-10
            dU = torch.einsum("snj,snk->jk", got[d]["ghv"], hs[d, :T, :N])
            assert float((dU - U[d].grad).abs().max()) <= 1e-10
            if cell == "gru":
                assert float((got[d]["ghv"].sum((0, 1)) - bh[d].grad).abs().max()) <= 1e-10
            assert float((got[d]["dh0"] - h0.grad[d]).abs().max()) <= 1e-10


def _check_all(c, k, scale=1.0, exchange=None):
    fw = RC.check_forward(c["cell"], c["gx"], c["lens"], c["U"], c["bh"], k["hx"], k["hs"], k["gates"], c["N"],
                          y=k["y"], y2=k["y2"], tag="fwd")
    bw = RC.check_bptt(c["cell"], c["dy"], c["lens"], c["U"], k["hs"], k["gates"], k["dgh"], k["dgx"], k["parts"],
                       c["N"], scale=scale, exchange=exchange, tag="bwd")
    return fw, bw


@pytest.mark.parametrize("p", RC.CPU_CASES, ids=CASE_IDS)
def test_e_ref_condition(p):
    """On every case table entry the fp32 emulation passes the checker, and e_ref is finite and
    nonzero wherever there is anything to round: on the state of every entry with a running row,
    on the gradients of every entry with a row of two steps or more (a row's last step has no
    recurrent term: its ReLU gradient is dy times a 0/1 mask, exact in any precision, e_ref = 0 and
    the kernel has to be exact too). Prints the share of elements where 8 e_ref is below the
    floor, so that the floor decides."""
    c = _case(p, seed=3)
    k = RC.emulate(c["cell"], c["gx"], c["lens"], c["U"], c["bh"], c["h0"], c["dy"], NP=c["N"] + 3)
    fw, bw = _check_all(c, k)
    for line in fw.lines() + bw.lines():
        print(line)
    assert not fw.failures and not bw.failures, (fw.failures + bw.failures)[:4]
    running = int(c["lens"].clamp(min=0).max()) > 0
    for name, v in list(fw.worst.items()) + list(bw.worst.items()):
        assert math.isfinite(v["e_ref_max"]), name
        if (running and name.startswith("hs")) or (int(c["lens"].max()) >= 2 and name.startswith("dg")):
            assert v["e_ref_max"] > 0, name
    if running:
        assert any(n.startswith("hs") for n in fw.worst)


def test_checker_sees_what_the_norm_misses():
    """Localised errors planted into a passing synthetic kernel output (the fp32 emulation, at the
    flagship T = 61, N = 32): the checker fails at the planted coordinates, while the whole-tensor
    ratio the norm tests measure (tests/test_kernels_gpu.py _rnn_case: y 2e-2, gradients 3e-2)
    moves by less than their tolerance for the first four."""
    cell, H, N, T, ndir, scale = "gru", 64, 32, 61, 2, 0.5
    lens = torch.randint(T // 2, T + 1, (N,), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    lens[0], lens[1] = T, T - 9
    c = RC.make_case(cell, H, N, T, ndir, 4, lens)
    GH = 3 * H
    clean = RC.emulate(cell, c["gx"], lens, c["U"], c["bh"], None, c["dy"], scale=scale, NP=N + 2)
    fw, bw = _check_all(c, clean, scale)
    assert not fw.failures and not bw.failures, (fw.failures + bw.failures)[:4]
    f32 = torch.float32

    def dU_of(k, d):
        return k["dgh"][d].reshape(T * (N + 2), GH).float().t() @ k["hx"][d, :T].reshape(T * (N + 2), H).float()

    def restate(k, d, s, b, hnew):
        """row b's state after step s of direction d becomes hnew, consistently published"""
        k["hs"][d, s + 1:, b] = hnew
        k["hx"][d, s + 1:, b] = hnew.to(torch.bfloat16)

    def reoutput(k):
        k["y2"] = RC.expected_outputs(k["hs"], lens, N)
        k["y"] = k["y2"][0] + k["y2"][1]

    def step(d, s, b, t):
        h = clean["hs"][d, s, b]
        return RC.cell_step(cell, h.to(torch.bfloat16).float(), h, c["gx"][t, b, d * GH:(d + 1) * GH].float(),
                            c["U"][d].float(), c["bh"][d])[0]

    plants = []

    def plant(name, where, side, old, tol):
        def deco(fn):
            plants.append((name, where, side, old, tol, fn))
            return fn
        return deco

    @plant("state element +4 bf16 ulps at one step", "hs[d=0]: 1 of", "fwd", "y", 2e-2)
    def _(k):
        v = k["hs"][0, T, 0, 5]
        ulp = 2.0 ** (math.frexp(float(v))[1] - 8)            # bf16: 8 significant bits
        restate(k, 0, T - 1, 0, torch.cat([k["hs"][0, T, 0, :5], (v + 4 * ulp).view(1), k["hs"][0, T, 0, 6:]]))
        reoutput(k)
        return "s=%d b=0 u=5" % (T - 1)

    @plant("backward direction of one row reads time L-s", "hs[d=1]", "fwd", "y", 2e-2)
    def _(k):
        restate(k, 1, T - 1, 0, step(1, T - 1, 0, 1))          # step T-1 of a full row reads time 0
        reoutput(k)
        return "s=%d b=0" % (T - 1)

    @plant("frozen row updates for one more step", "frozen hs[d=0]", "fwd", "y", 2e-2)
    def _(k):
        L = int(lens[1])
        restate(k, 0, L, 1, step(0, L, 1, L))
        return "s=%d b=1" % L

    @plant("32-unit slice of one step's dgh without the carry", "dgh[d=0]", "bwd", "dU", 3e-2)
    def _(k):
        s, b = 20, 3
        r = RC.bptt(cell, c["dy"], lens, c["U"], k["hs"], k["gates"], N, f32, feed="rounded")[0]
        ratio = (r["dh"][s, b, :32] - r["carry"][s, b, :32]) / r["dh"][s, b, :32]
        for g in range(3):
            k["dgh"][0, s, b, g * H:g * H + 32] = (r["ghv"][s, b, g * H:g * H + 32] * ratio).to(torch.bfloat16)
        return "s=%d b=%d" % (s, b)

    @plant("padded dgh row nonzero", "padded dgh rows[d=1]", "bwd", "dU", 3e-2)
    def _(k):
        k["dgh"][1, 7, N + 1, 11] = 1.0
        return "s=7 row-N=1 col=11"

    @plant("hx != bf16(hs) in one element", "hx=bf16(hs)[d=1]", "fwd", "y", 2e-2)
    def _(k):
        k["hx"][1, 9, 4, 17] += 2.0 ** -6
        return "s=9 b=4 u=17"

    @plant("dgx_scale missing for one gate", "dgx[d=0]", "bwd", "dgx", 3e-2)
    def _(k):
        k["dgx"][:, :, H:2 * H] = (k["dgx"][:, :, H:2 * H].float() / scale).to(torch.bfloat16)
        return "col=%d" % H

    for i, (name, where, side, old, tol, fn) in enumerate(plants):
        k = {key: (v.clone() if v is not None else None) for key, v in clean.items()}
        coords = fn(k)
        fw, bw = _check_all(c, k, scale)
        fails = (fw if side == "fwd" else bw).failures
        ratio = {"y": lambda: _rel(k["y"], clean["y"]), "dgx": lambda: _rel(k["dgx"], clean["dgx"]),
                 "dU": lambda: max(_rel(dU_of(k, d), dU_of(clean, d)) for d in range(2))}[old]()
        hit = [m for m in fails if where in m]
        print("plant %-52s checker: %s | whole-tensor %s ratio %.2e (tolerance %.0e: %s)" % (
            name, hit[0][:150] if hit else "PASSED", old, ratio, tol, "passes" if ratio < tol else "fails"))
        assert hit, (name, fails[:3])
        if name.startswith("dgx_scale"):
            assert H <= int(hit[0].split("col=")[1].split(":")[0]) < 2 * H, hit[0]
        else:
            assert coords in hit[0], (name, coords, hit[0])
        if i < 4:
            assert ratio < tol, (name, ratio, tol)
