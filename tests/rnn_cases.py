"""Step-local fp64 oracle, per-element checker and case tables of the recurrence kernels
(csrc/rnn_xcd.hip, rnn_fp8.hip forward, rnn_persistent.hip). Pure torch, device-agnostic, does not
import the extension.

Buffer contract (header of csrc/rnn_persistent.hip, shared by every family):
  hx[d, s+1] / hs[d, s+1]   bf16 operand copy / fp32 state after step s; slot 0 = h0
  gates[d, s]               (r, z, n, U_n h + b_hn) of step s (GRU)
  gx, y, dy, dgx            time-indexed: direction 1 at step s uses time len-1-s while s < len,
                            time s otherwise; direction 0 always time s
  dgh[d, s]                 bf16 gradient of the recurrent pre-activation of step s
  the state is frozen, and outputs / gradients are zero, from step len on.

Method. Given the kernel's OWN state at step s (hx[d, s] as the operand it published, hs[d, s]),
step s+1 is a deterministic function of exact inputs, so every step is checked on its own, per
element: no chaos of a free-running comparison, no ReLU mask flips. The BPTT is linearised at the
kernel's own forward state and fed the kernel's own stored bf16 dgh[d, s+1] for the recurrent
term: every BPTT family multiplies exactly that stored value (rnnrs / rnnw: the bf16 tile dg_s
that is also staged for the dgh store; generation 1 reads dgh back), so nothing else is modelled.
The GRU carry z * dh is not observable and is chained by the oracle in fp64 (its error bound is
chained with it, E_carry below). ReLU mask, read off the kernels (rnn_xcd.hip rnnrs / rnnw
epilogues, rnn_persistent.hip): da = dh if 0 < hs[d, s+1] < 20 else 0, strict on both sides, so
a unit at exactly 0 or exactly the cap passes no gradient.

Bound (the rule of tests/test_ctc_gpu.py): per element |kernel - oracle| <= max(8 e_ref, floor).
e_ref is, per element, the error against the same oracle of the plain fp32 torch evaluation of
the same step from the same bf16 / fp32 inputs (never the kernel's output). The floors are
a-priori bounds, with eps = 2^-24 (fp32 unit roundoff) and b = 2^-8 (bf16: one rounding to
nearest moves x by at most 2^-8 |x|):

  pre-activation a_j = gx + sum_k U_jk h_k + bh_j, H products (exact in fp32: bf16 x bf16) and
      H + 2 additions in any order:  d_a = (H + 2) eps (sum_k |U_jk h_k| + |bh_j| + |gx|)
  ReLU state  h' = clamp(a, 0, 20), Lipschitz 1:  d_h = d_a
  sigmoidf_ (common.h) = v_rcp(1 + v_exp(-x)): argument scaling by log2 e (|x| sigma'(x) eps
      < 1 eps), v_exp 1 ulp (2 eps relative on e <= the result's 2 eps), the add (1 eps), v_rcp
      1 ulp (2 eps): 6 eps absolute on a value <= 1, taken as SIG_ABS = 8 eps. sigma' <= 1/4:
      d_r = d_a / 4 + SIG_ABS (same for z)
  ghn = (U_n h) + b_hn:  d_ghn = (H + 2) eps (sum |U h| + |b_hn|)
  a_n = gx_n + r ghn:  d_an = |ghn| d_r + r d_ghn + d_r d_ghn + 2 eps (|gx_n| + |r ghn|)
  tanhf_ = 1 - 2 v_rcp(v_exp(2x) + 1), q = 1 / (e + 1), e = exp(2x): the result is a difference of
      O(1) values, so its error is absolute, not relative (it cancels near 0). Argument scaling and
      v_exp leave (2 + 2|x|) eps relative on e, which reaches q with weight e / (1 + e):
      q e (1 + |x|) / (1 + e) <= 0.6 for every x, so 1.2 eps on q; the add 1 eps, v_rcp 2 eps (q <= 1);
      doubled, plus 1 eps for the final subtraction: < 10 eps, taken as TANH_ABS = 16 eps.
      tanh' <= 1:  d_n = d_an + TANH_ABS
  h' = (1 - z) n + z h:  d_h = |h - n| d_z + |1 - z| d_n + 4 eps (|(1 - z) n| + |z h|)
  the stored gates (r, z, n, ghn) carry d_r, d_z, d_n, d_ghn.
  fp8 forward: the operand is e4m3(hs[d, s]) and U is e4m3 with one power-of-two scale; products
      of two e4m3 values are exact in fp32 and the scale is exact, so the same floors hold with
      the quantised operands in the sums.

  BPTT recurrent term  dhrec_u = sum_j U[j, u] dgh[d, s+1, b, j], G H terms:
      generation 1 (fp32 partial sums through LDS):        E_rec = G H eps sum |terms|
      rnnrs (R <= 16) and rnnw exchange ROUNDED partials: producer p of the group's P workgroups
      multiplies its own gate columns (32 per gate in rnnrs, 64 in rnnw) and publishes
      P_p = sum_{j in cols_p} U[j, u] dgh[j] as bf16 (bf16x2_tagged, common.h: round to nearest,
      b |P_p|, then the mantissa LSB REPLACED by the ring tag, one more bf16 ulp, 2 b |P_p|), the
      consumer sums the P values in fp32:   E_rec = 3 b sum_p |P_p| + (G H + P) eps sum |terms|
      The oracle splits j into the producers itself. (b sum |P_p| alone, plain rounding, is not
      enough: the tag replacement is the kernel's own documented 1.5 ulp, and with one producer,
      H = 32, the measured error reaches 0.88 of this floor.)
      rnnrs with knob 64 exchanges fp32 partials whose LSB carries the tag: 2 eps sum_p |P_p|
      instead of the 3 b term. Generation 1 has no exchange of partials and no such term.
  dh = dy + carry + dhrec:  E_dh = E_rec + 3 eps (|dy| + |carry| + |dhrec|) + E_carry
  GRU carry into step s-1, c = z dh:  E_carry = z E_dh + eps |c|   (chained over the steps)
  every gate gradient is dh times a coefficient k of the saved gates (a few fp32 products):
      E_val = |k| E_dh + 8 eps |want|
  bf16 outputs dgh, dgx: one output rounding: floor = (1 + b) E_val + b |want| (dgx: both
      scaled by dgx_scale; the scaling itself is inside the 8 eps)
  bias partials: the kernels sum the UNROUNDED fp32 gate gradients (sbx / sbh registers, LDS row
      reduction, one add per group), so no b term: floor = sum_{s, b} E_val + (T N + 32) eps
      sum_{s, b} |want|; the input-bias partial is the sum before dgx_scale.
  dU (ops/rnn.py _dU, fp32 output of a bf16 GEMM over steps x NP rows) against
      sum_s dgh[d, s]^T hx[d, s] of the kernel's own buffers: T NP eps sum |terms|.
Exact (bitwise) properties: hx = bf16(hs) in every slot; per-direction output = bf16(hs[d, s+1])
at the step's time; summed output = bf16(bf16(fw) + bf16(bw)); frozen state, zero outputs and
zero gradients from step len on; dgh rows N..NP zero; where dgx_scale is a power of two, the
columns dgx and dgh share agree bitwise after the exact scaling.
"""
import math

import torch

EPS = 2.0 ** -24
BF = 2.0 ** -8
RELU_CAP = 20.0
SIG_ABS = 8 * EPS
TANH_ABS = 16 * EPS
GATES = {"rnn_relu": 1, "gru": 3}
F64 = torch.float64


# ------------------------------------------------------------------------------------ indexing
def time_index(lens, T, d):
    """(t [T, N] long, act [T, N] bool): the time step s of direction d uses for row b, and
    whether the row is still running at step s. The same map read the other way gives the step
    that produced time t."""
    s = torch.arange(T, device=lens.device).unsqueeze(1)
    L = lens.long().unsqueeze(0)
    act = s < L
    t = s.expand(T, L.shape[1]) if d == 0 else torch.where(act, L - 1 - s, s)
    return t.clamp(0, max(T - 1, 0)), act


def _coords(idx, shape, dims):
    out = []
    for n, name in zip(reversed(shape), reversed(dims)):
        out.append("%s=%d" % (name, idx % n))
        idx //= n
    return " ".join(reversed(out))


class Report:
    """What a checker found: failures (messages naming the worst element's coordinates) and,
    per compared quantity, the worst element's error / e_ref / floor."""

    def __init__(self, tag=""):
        self.tag, self.failures, self.worst = tag, [], {}

    def compare(self, name, got, want, ref, floor, mask, dims):
        got, ref = got.to(F64), ref.to(F64)
        err, eref = (got - want).abs(), (ref - want).abs()
        bound = torch.maximum(8 * eref, floor)
        mask = mask.expand_as(err)
        n = int(mask.sum())
        if n == 0:
            return
        score = (err / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf, posinf=math.inf)
        score = torch.where(mask, score, torch.full_like(score, -1.0))
        i = int(score.argmax())
        nbad = int((mask & ~(err <= bound)).sum())
        where = _coords(i, tuple(err.shape), dims)
        e = dict(err=float(err.flatten()[i]), e_ref=float(eref.flatten()[i]), floor=float(floor.expand_as(err).flatten()[i]),
                 use=float(score.flatten()[i]), where=where, n=n, bad=nbad,
                 e_ref_max=float(eref[mask].max()), err_max=float(err[mask].nan_to_num(nan=math.inf).max()),
                 floor_share=float(((8 * eref < floor) & mask).sum()) / n)
        old = self.worst.get(name)
        if old is None or e["use"] > old["use"]:
            if old is not None:
                e["e_ref_max"] = max(e["e_ref_max"], old["e_ref_max"])
            self.worst[name] = e
        if nbad:
            self.failures.append("%s %s: %d of %d elements out of bound, worst at %s: got %r want %r err %.3e e_ref %.3e "
                                 "floor %.3e" % (self.tag, name, nbad, n, where, float(got.flatten()[i]),
                                                 float(want.flatten()[i]), e["err"], e["e_ref"], e["floor"]))

    def exact(self, name, got, want, mask, dims):
        """got == want on mask (0.0 == -0.0; a NaN never matches)."""
        want = torch.as_tensor(want, device=got.device, dtype=got.dtype).expand_as(got)
        bad = ~(got == want) & mask.expand_as(got)
        nbad = int(bad.sum())
        if nbad:
            i = int(bad.flatten().to(torch.uint8).argmax())
            self.failures.append("%s %s: %d elements differ, first at %s: got %r want %r" % (
                self.tag, name, nbad, _coords(i, tuple(got.shape), dims), float(got.flatten()[i]), float(want.flatten()[i])))

    def lines(self):
        return ["rnn-err %s %-14s kernel %.3e e_ref %.3e floor %.3e (%.2f of bound) at %s; floor decides %.0f%%" % (
            self.tag, k, v["err"], v["e_ref"], v["floor"], v["use"], v["where"], 100 * v["floor_share"])
            for k, v in self.worst.items()]


# ------------------------------------------------------------------------------------ forward
def cell_step(cell, h_op, h_prev, gxt, U, bh):
    """One step of one direction in the dtype of its arguments: h_op [..., H] the operand of the
    recurrent product, h_prev [..., H] the state, gxt [..., G H], U [G H, H], bh [G H] or None.
    Returns (h_new, gates [..., H, 4] or None)."""
    H = h_prev.shape[-1]
    pre = h_op @ U.t()
    if cell == "rnn_relu":
        return torch.clamp(gxt + pre, 0.0, RELU_CAP), None
    gh = pre + bh
    r = torch.sigmoid(gxt[..., :H] + gh[..., :H])
    z = torch.sigmoid(gxt[..., H:2 * H] + gh[..., H:2 * H])
    ghn = gh[..., 2 * H:]
    n = torch.tanh(gxt[..., 2 * H:] + r * ghn)
    return (1.0 - z) * n + z * h_prev, torch.stack([r, z, n, ghn], -1)


def fwd_floors(cell, h_op, h_prev, gxt, U, bh, gates):
    """(floor of h_new, floor of the gates or None), fp64, from the module docstring."""
    H = h_prev.shape[-1]
    k = (H + 2) * EPS
    A = h_op.abs() @ U.abs().t()
    if cell == "rnn_relu":
        return k * (A + gxt.abs()), None
    B = bh.abs()
    r, z, n, ghn = gates.unbind(-1)
    d_a = k * (A + B + gxt.abs())
    d_r = d_a[..., :H] / 4 + SIG_ABS
    d_z = d_a[..., H:2 * H] / 4 + SIG_ABS
    d_ghn = k * (A[..., 2 * H:] + B[2 * H:])
    gxn = gxt[..., 2 * H:]
    d_an = ghn.abs() * d_r + r * d_ghn + d_r * d_ghn + 2 * EPS * (gxn.abs() + (r * ghn).abs())
    d_n = d_an + TANH_ABS
    d_h = (h_prev - n).abs() * d_z + (1 - z).abs() * d_n + 4 * EPS * (((1 - z) * n).abs() + (z * h_prev).abs())
    return d_h, torch.stack([d_r, d_z, d_n, d_ghn], -1)


def expected_outputs(hs, lens, N):
    """Per-direction outputs [ndir, T, N, H] bf16 implied by the saved state: bf16(hs[d, s+1]) at
    the time step s wrote, zero from the row's length on."""
    ndir, T1, _, H = hs.shape
    T = T1 - 1
    ar = torch.arange(N, device=hs.device)
    out = []
    for d in range(ndir):
        sidx, valid = time_index(lens, T, d)
        v = hs[d, 1:, :N][sidx, ar].to(torch.bfloat16)
        out.append(torch.where(valid.unsqueeze(-1), v, torch.zeros_like(v)))
    return torch.stack(out)


def check_forward(cell, gx, lens, U, bh, hx, hs, gates, N, y=None, y2=None, h_operand=None, tag=""):
    """Every (d, s, b, u) of a forward launch's saved buffers against the step-local oracle.
    gx [T, N, ndir G H] bf16, U / bh per-direction lists (the operands the kernel multiplied: the
    dequantised ones for the fp8 forward), hx / hs [ndir, T+1, NP, H], gates [ndir, T, NP, H, 4]
    or None, y [T, N, H] the summed output, y2 [ndir, T, N, H] the per-direction outputs where
    the launch has them, h_operand [ndir, T, N, H] where the operand is not hx (fp8)."""
    rep = Report(tag)
    ndir, T1, NP, H = hs.shape
    T, GH = T1 - 1, GATES[cell] * H
    lens = lens.to(hs.device)
    ar = torch.arange(N, device=hs.device)
    for d in range(ndir):
        t_idx, act = time_index(lens, T, d)
        gxt = gx[t_idx, ar, d * GH:(d + 1) * GH]
        h_op = hx[d, :T, :N] if h_operand is None else h_operand[d]
        hp, hn = hs[d, :T, :N], hs[d, 1:, :N]
        b64 = bh[d].to(F64) if cell == "gru" else None
        b32 = bh[d].float() if cell == "gru" else None
        want_h, want_g = cell_step(cell, h_op.to(F64), hp.to(F64), gxt.to(F64), U[d].to(F64), b64)
        ref_h, ref_g = cell_step(cell, h_op.float(), hp.float(), gxt.float(), U[d].float(), b32)
        fl_h, fl_g = fwd_floors(cell, h_op.to(F64), hp.to(F64), gxt.to(F64), U[d].to(F64), b64, want_g)
        a3 = act.unsqueeze(-1)
        dims = ("s", "b", "u")
        rep.compare("hs[d=%d]" % d, hn, want_h, ref_h, fl_h, a3, dims)
        if cell == "gru":
            rep.compare("gates[d=%d]" % d, gates[d, :, :N], want_g, ref_g, fl_g, a3.unsqueeze(-1), dims + ("gate",))
        rep.exact("frozen hs[d=%d]" % d, hn, hp, ~a3, dims)
        rep.exact("hx=bf16(hs)[d=%d]" % d, hx[d, :, :N], hs[d, :, :N].to(torch.bfloat16), torch.ones_like(a3[:1]), dims)
        if NP > N:
            fin = torch.isfinite(hx[d, :T, N:].float())
            rep.exact("finite padded hx[d=%d]" % d, fin.float(), 1.0, torch.ones_like(fin), dims)
        last = hs[d, lens.long().clamp(0, T)[:N], ar]
        rep.exact("h_last[d=%d]" % d, hs[d, T, :N], last, torch.ones_like(last, dtype=torch.bool), ("b", "u"))
    ydir = expected_outputs(hs, lens, N)
    allm = torch.ones(1, dtype=torch.bool, device=hs.device)
    if y2 is not None:
        rep.exact("y per direction", y2.float(), ydir.float(), allm, ("d", "t", "b", "u"))
    if y is not None:
        want = ydir[0] + ydir[1] if ndir == 2 else ydir[0]
        rep.exact("y", y.float(), want.float(), allm, ("t", "b", "u"))
    return rep


def forward_chain(cell, gx, lens, U, bh, h0, dtype, round_operand, NP=None):
    """Free-running scan built from cell_step in ``dtype``: the buffers a kernel would leave
    (hx bf16, hs, gates, y2 per direction in ``dtype``). round_operand: feed bf16(h) to the
    product as the kernels do. Padded rows N..NP stay zero."""
    T, N, _ = gx.shape
    ndir = len([u for u in U if u is not None])
    H = U[0].shape[1]
    G = GATES[cell]
    GH = G * H
    NP = NP or N
    dev = gx.device
    hs = torch.zeros(ndir, T + 1, NP, H, dtype=dtype, device=dev)
    gates = torch.zeros(ndir, T, NP, H, 4, dtype=dtype, device=dev) if cell == "gru" else None
    y2 = torch.zeros(ndir, T, N, H, dtype=dtype, device=dev)
    ar = torch.arange(N, device=dev)
    for d in range(ndir):
        t_idx, act = time_index(lens, T, d)
        if h0 is not None:
            hs[d, 0, :N] = h0[d].to(dtype)
        for s in range(T):
            h = hs[d, s, :N]
            h_op = h.to(torch.bfloat16).to(dtype) if round_operand else h
            gxt = gx[t_idx[s], ar, d * GH:(d + 1) * GH].to(dtype)
            hn, g = cell_step(cell, h_op, h, gxt, U[d].to(dtype), bh[d].to(dtype) if cell == "gru" else None)
            a = act[s].unsqueeze(-1)
            hs[d, s + 1, :N] = torch.where(a, hn, h)
            if g is not None:
                gates[d, s, :N] = torch.where(a.unsqueeze(-1), g, torch.zeros_like(g))
            y2[d, t_idx[s][act[s]], ar[act[s]]] = hn[act[s]]
    return hs.to(torch.bfloat16), hs, gates, y2


# ------------------------------------------------------------------------------------ BPTT
def _partial_abs(src, Ud, G, H, pw):
    """sum_p |P_p| [N, H]: P_p = sum over producer p's gate columns (pw per gate) of U[j, u] src[j]."""
    P = -(-H // pw)
    N = src.shape[0]
    s3 = src.new_zeros(N, G, P * pw)
    s3[:, :, :H] = src.view(N, G, H)
    u3 = Ud.new_zeros(G, P * pw, H)
    u3[:, :H] = Ud.view(G, H, H)
    part = torch.einsum("ngpj,gpju->npu", s3.view(N, G, P, pw), u3.view(G, P, pw, H))
    return part.abs().sum(1), P


def bptt(cell, dy, lens, U, hs, gates, N, dtype, dgh=None, feed="kernel", exchange=None, scale=1.0):
    """BPTT of every direction linearised at the saved forward state (hs, gates), in ``dtype``.
    feed: the recurrent term's operand: "kernel" the stored bf16 dgh[d, s+1] given in ``dgh``;
    "rounded" this function's own step s+1 rounded to bf16 (an emulated kernel); "own" its own
    unrounded values (the exact gradient). exchange: None (fp32 sums, generation 1) or (producer
    columns per gate, relative error of one exchanged partial) for the floors.
    Returns per direction a dict: ghv, gxs [T, N, G H] (step-indexed, unrounded, unscaled), dh and
    the carry that entered it [T, N, H], dh0 [N, H], and with dtype fp64 the floors f_dgh, f_dgx
    (of the bf16 outputs, dgx with scale), e_val_h, e_val_x (of the unrounded values)."""
    T = dy.shape[0]
    ndir, _, _, H = hs.shape
    G = GATES[cell]
    dev = hs.device
    ar = torch.arange(N, device=dev)
    want_floor = dtype == F64
    out = []
    for d in range(ndir):
        Ud = U[d].to(dtype)
        t_idx, act_all = time_index(lens, T, d)
        carry = torch.zeros(N, H, dtype=dtype, device=dev)
        e_carry = torch.zeros(N, H, dtype=F64, device=dev)
        ghv_all, gxs_all, dh_all, carry_all = [None] * T, [None] * T, [None] * T, [None] * T
        fl = dict(f_dgh=[None] * T, f_dgx=[None] * T, e_val_h=[None] * T, e_val_x=[None] * T)
        nxt = None
        dhrec = torch.zeros(N, H, dtype=dtype, device=dev)
        for s in range(T - 1, -1, -1):
            act = act_all[s].unsqueeze(-1)
            dyt = torch.where(act, dy[t_idx[s], ar].to(dtype), torch.zeros((), dtype=dtype, device=dev))
            e_rec = 0.0
            if s + 1 < T:
                src = dgh[d, s + 1, :N].to(dtype) if feed == "kernel" else \
                    (nxt.to(torch.bfloat16).to(dtype) if feed == "rounded" else nxt)
                dhrec = src @ Ud
                if want_floor:
                    absprod = src.abs() @ Ud.abs()
                    if exchange is None:
                        e_rec = G * H * EPS * absprod
                    else:
                        pabs, P = _partial_abs(src, Ud, G, H, exchange[0])
                        e_rec = exchange[1] * pabs + (G * H + P) * EPS * absprod
            else:
                dhrec = torch.zeros(N, H, dtype=dtype, device=dev)
            dh = dyt + carry + dhrec
            zero = torch.zeros_like(dh)
            if cell == "gru":
                g = torch.where(act.unsqueeze(-1), gates[d, s, :N].to(dtype), torch.zeros((), dtype=dtype, device=dev))
                r, z, n, ghn = g.unbind(-1)
                hp = torch.where(act, hs[d, s, :N].to(dtype), zero)
                kn = (1.0 - z) * (1.0 - n * n)
                coef_h = [kn * ghn * r * (1.0 - r), (hp - n) * z * (1.0 - z), kn * r]
                coef_x = coef_h[:2] + [kn]
                cnew = torch.where(act, dh * z, zero)
            else:
                h1 = hs[d, s + 1, :N]
                m = ((h1 > 0) & (h1 < RELU_CAP) & act).to(dtype)
                coef_h = coef_x = [m]
                z = zero
                cnew = zero
            ghv = torch.where(act, torch.cat([dh * c for c in coef_h], 1), zero.repeat(1, G))
            gxs = torch.where(act, torch.cat([dh * c for c in coef_x], 1), zero.repeat(1, G))
            if want_floor:
                e_dh = e_rec + 3 * EPS * (dyt.abs() + carry.abs() + dhrec.abs()) + e_carry
                e_dh = torch.where(act, e_dh, zero)
                for key, coef, val in (("h", coef_h, ghv), ("x", coef_x, gxs)):
                    ev = torch.cat([c.abs() * e_dh for c in coef], 1) + 8 * EPS * val.abs()
                    fl["e_val_" + key][s] = ev
                    sc = abs(scale) if key == "x" else 1.0
                    fl["f_dg" + key][s] = sc * ((1 + BF) * ev + BF * val.abs())
                e_carry = torch.where(act, z * e_dh + EPS * cnew.abs(), zero)
            dh_all[s], carry_all[s] = dh, carry
            carry = cnew
            ghv_all[s], gxs_all[s], nxt = ghv, gxs, ghv
        res = dict(ghv=torch.stack(ghv_all) if T else torch.zeros(0, N, G * H, dtype=dtype, device=dev),
                   gxs=torch.stack(gxs_all) if T else torch.zeros(0, N, G * H, dtype=dtype, device=dev),
                   dh0=carry + (ghv_all[0] @ Ud if T else 0.0))
        if T:
            res.update(dh=torch.stack(dh_all), carry=torch.stack(carry_all))
        if want_floor and T:
            res.update({k: torch.stack(v) for k, v in fl.items()})
        out.append(res)
    return out


def _pow2(x):
    m, _ = math.frexp(abs(x))
    return x != 0 and m == 0.5


def check_bptt(cell, dy, lens, U, hs, gates, dgh, dgx, parts, N, scale=1.0, exchange=None, tag=""):
    """Every element of a BPTT launch's outputs against the oracle linearised at the kernel's own
    forward state and fed the kernel's own dgh. dgh [ndir, T, NP, G H] bf16, dgx [T, N, ndir G H]
    bf16 (x scale), parts [k, ndir, BG, G H] fp32 or None."""
    rep = Report(tag)
    ndir, T, NP, GH = dgh.shape
    H = hs.shape[-1]
    G = GATES[cell]
    lens = lens.to(hs.device)
    ar = torch.arange(N, device=hs.device)
    want = bptt(cell, dy, lens, U, hs, gates, N, F64, dgh=dgh, feed="kernel", exchange=exchange, scale=scale)
    ref = bptt(cell, dy, lens, U, hs, gates, N, torch.float32, dgh=dgh, feed="kernel")
    dims = ("s", "b", "col")
    for d in range(ndir):
        w, r = want[d], ref[d]
        t_idx, act = time_index(lens, T, d)
        s_idx = torch.arange(T, device=hs.device).unsqueeze(1).expand(T, N)
        t_store = torch.where(act, t_idx, s_idx)
        allm = torch.ones(1, 1, 1, dtype=torch.bool, device=hs.device)
        got_h = dgh[d, :, :N]
        got_x = dgx[t_store, ar, d * GH:(d + 1) * GH]
        rep.compare("dgh[d=%d]" % d, got_h, w["ghv"], r["ghv"].to(torch.bfloat16), w["f_dgh"], allm, dims)
        rep.compare("dgx[d=%d]" % d, got_x, w["gxs"] * scale, (r["gxs"] * scale).to(torch.bfloat16), w["f_dgx"], allm, dims)
        a3 = act.unsqueeze(-1)
        rep.exact("dgh past len[d=%d]" % d, got_h.float(), 0.0, ~a3, dims)
        rep.exact("dgx past len[d=%d]" % d, got_x.float(), 0.0, ~a3, dims)
        if NP > N:
            rep.exact("padded dgh rows[d=%d]" % d, dgh[d, :, N:].float(), 0.0, allm, ("s", "row-N", "col"))
        if _pow2(scale):
            shared = GH if cell == "rnn_relu" else 2 * H
            rep.exact("dgx/scale == dgh[d=%d]" % d, got_x[..., :shared].float() / scale, got_h[..., :shared].float(), allm, dims)
        if parts is not None:
            terms = T * N + 32
            cases = [("dbx", 0, "gxs", "e_val_x")] + ([("dbh", 1, "ghv", "e_val_h")] if cell == "gru" else [])
            for name, k, key, ek in cases:
                got = parts[k, d].to(F64).sum(0)
                fl = w[ek].sum((0, 1)) + terms * EPS * w[key].abs().sum((0, 1))
                rep.compare("%s[d=%d]" % (name, d), got, w[key].sum((0, 1)), r[key].sum((0, 1)), fl,
                            torch.ones(1, dtype=torch.bool, device=hs.device), ("col",))
    return rep


def check_dU(dU, dgh, hx, d, N, tag=""):
    """dU[d] [G H, H] fp32 against sum_s dgh[d, s]^T hx[d, s] over the REAL rows of the kernel's own
    buffers: a nonzero padded dgh row, or a NaN in a padded hx row, shows as an error here."""
    rep = Report(tag)
    T, NP = dgh.shape[1], dgh.shape[2]
    a = dgh[d, :, :N].reshape(T * N, -1)
    b = hx[d, :T, :N].reshape(T * N, -1)
    want = a.to(F64).t() @ b.to(F64)
    ref = a.float().t() @ b.float()
    fl = T * NP * EPS * (a.to(F64).abs().t() @ b.to(F64).abs())
    rep.compare("dU[d=%d]" % d, dU, want, ref, fl, torch.ones(1, 1, dtype=torch.bool, device=dU.device), ("col", "k"))
    return rep


def emulate(cell, gx, lens, U, bh, h0, dy, scale=1.0, NP=None):
    """A synthetic kernel: the fp32 evaluation of the whole launch pair with the kernels' operand
    roundings (bf16 h into the product, bf16 dgh into the recurrent term), in the kernels' buffer
    layout. Returns a dict of hx, hs, gates, y2, y, dgh, dgx, parts."""
    T, N, _ = gx.shape
    f32 = torch.float32
    hx, hs, gates, y2 = forward_chain(cell, gx, lens, U, bh, h0, f32, True, NP)
    ndir, _, NPp, H = hs.shape
    GH = GATES[cell] * H
    y2 = y2.to(torch.bfloat16)
    y = y2[0] + y2[1] if ndir == 2 else y2[0].clone()
    res = bptt(cell, dy, lens, U, hs, gates, N, f32, feed="rounded")
    dgh = torch.zeros(ndir, T, NPp, GH, dtype=torch.bfloat16, device=gx.device)
    dgx = torch.zeros(T, N, ndir * GH, dtype=torch.bfloat16, device=gx.device)
    parts = torch.zeros(2 if cell == "gru" else 1, ndir, 1, GH, dtype=f32, device=gx.device)
    ar = torch.arange(N, device=gx.device)
    for d in range(ndir):
        t_idx, act = time_index(lens, T, d)
        t_store = torch.where(act, t_idx, torch.arange(T, device=gx.device).unsqueeze(1).expand(T, N))
        dgh[d, :, :N] = res[d]["ghv"].to(torch.bfloat16)
        dgx[t_store, ar, d * GH:(d + 1) * GH] = (res[d]["gxs"] * scale).to(torch.bfloat16)
        parts[0, d, 0] = res[d]["gxs"].sum((0, 1))
        if cell == "gru":
            parts[1, d, 0] = res[d]["ghv"].sum((0, 1))
    return dict(hx=hx, hs=hs, gates=gates, y2=y2, y=y, dgh=dgh, dgx=dgx, parts=parts)


# ------------------------------------------------------------------------------------ cases
def edge_lens(T, N):
    """One edge batch: full, empty, 1, 2, T-1 and a duplicate of T, cycled over N rows."""
    pat = [T, 0, 1, 2, T - 1, T]
    return torch.tensor([max(0, min(T, pat[i % len(pat)])) for i in range(N)], dtype=torch.int32)


def length_pattern(name, T, N):
    if name == "edge":
        return edge_lens(T, N)
    if name == "full":
        return torch.full((N,), T, dtype=torch.int32)
    if name == "one":
        return torch.full((N,), min(1, T), dtype=torch.int32)
    if name == "zero":
        return torch.zeros(N, dtype=torch.int32)
    if name == "negative":          # a 26-frame clip: floor((26 - 34) / 4) = -2
        v = edge_lens(T, N)
        v[0] = -2
        return v
    raise ValueError(name)


LENGTH_PATTERNS = ("edge", "full", "one", "zero", "negative")


def make_case(cell, H, N, T, ndir, seed, lens="edge", h0=False):
    """Inputs of one launch pair, already rounded to what the kernels read (bf16 gx / U / dy, a
    bf16-representable fp32 bias), random also past the lengths (the kernels must ignore it).
    ReLU: a few inputs of +30 drive units to exactly the cap."""
    g = torch.Generator().manual_seed(1000 * seed + H + 7 * N + T)
    G = GATES[cell]
    gx = (torch.randn(T, N, ndir * G * H, generator=g) * (0.5 if cell == "gru" else 0.3)).to(torch.bfloat16)
    if cell == "rnn_relu":
        gx[:, :, 3::37] = 30.0
    U = [(torch.randn(G * H, H, generator=g) / math.sqrt(H)).to(torch.bfloat16) for _ in range(ndir)]
    bh = [(torch.randn(G * H, generator=g) * 0.1).to(torch.bfloat16).float() if cell == "gru" else None for _ in range(ndir)]
    dy = torch.randn(T, N, H, generator=g).to(torch.bfloat16)
    h0v = torch.randn(ndir, N, H, generator=g) if h0 else None
    if h0v is not None and cell == "rnn_relu":
        h0v = h0v.abs()
    return dict(cell=cell, H=H, N=N, T=T, ndir=ndir, gx=gx, U=U, bh=bh, dy=dy, h0=h0v,
                lens=length_pattern(lens, T, N) if isinstance(lens, str) else lens)


# (id, cell, H): the geometry sweep of tests/test_rnn_gpu.py; the expected kernel family is
# asserted there through the extension's own dispatch report, not mirrored here
FWD_RNNE = [32, 64, 288, 544, 800, 896, 1024]
FWD_RNNQ_RELU = [32, 160, 288, 416, 544, 672, 800, 928, 1024]
FWD_RNNQ_GRU_LDS = [1152, 1280]
FWD_GEN2_GRU = [928, 1056, 1184, 1344]
FWD_GEN2_SMALL = [32, 256, 480, 704]
WIDE_RELU = [1056, 1312, 1088, 1152, 1376, 1568, 1600, 1792]
BWD_RNNRS = [224, 448, 672, 896, 928, 1344]
FP8_FWD = [256, 512, 768, 1024, 1280]
# CPU case table (small widths: the oracle itself is width-independent)
CPU_CASES = [(cell, H, N, T, ndir, lens, h0)
             for cell in ("gru", "rnn_relu")
             for (H, N, T, ndir, lens, h0) in ((32, 7, 7, 2, "edge", False), (64, 5, 5, 1, "edge", True),
                                               (32, 3, 1, 2, "full", True), (32, 6, 3, 2, "negative", False),
                                               (32, 2, 4, 2, "zero", False), (32, 2, 6, 2, "one", True))]
