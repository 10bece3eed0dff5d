"""Lookahead convolution kernels (csrc/lookahead.hip) per element against the fp64 oracle of
tests/lookahead_cases.py (definition, the two input families, every tolerance and the case grid
are in its docstring), then the wiring: autograd op and arena, Trainer steps with and without
step graphs, the whole model against the fp32 reference engine, and the streaming recogniser.

Printed (run with -s): LOOKWORST lines, the worst err/tol per kernel over family B, and LOOKGRAD
lines, the relative gradient error of the new parameter against the reference engine.
profiles/lookahead.md records them.
"""
import copy

import pytest
import torch

import conv_cases as CO
import lookahead_cases as LC
from deepspeech_amd.models import DeepSpeech2

pytestmark = pytest.mark.gpu
F64 = torch.float64
BFT, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(LC.WORST.items()):
        print("LOOKWORST %-24s err/tol %.3f" % (k, v))


def _ext():
    from deepspeech_amd.ops import _ext
    return _ext.ext()


def bfd(t, dev):
    return t.to(F32).to(BFT).to(dev).contiguous()


def G(shape, dtype, dev):
    return CO.Guarded(shape, dtype, dev)


def _wgrad(C, dr, h, lens, tau, dev, name):
    T, B, H = h.shape
    P = int(C.lookahead_wgrad_parts(T, B, H))
    part, dw = G((P, H * (tau + 1)), F32, dev), G((H, tau + 1), F32, dev)
    C.lookahead_wgrad(dr, h, lens, part.t, tau)
    C.col_sum([part.t.view(1, P, H * (tau + 1))], [dw.t], [False])
    part.verify(name + " partials")
    dw.verify(name + " dw")
    return dw.t


# ------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("c", LC.GRID + LC.EXTRA, ids=LC.ident)
def test_kernels_per_element(cuda, c):
    C = _ext()
    tau, T, B, H = c
    for fam in ("A", "B"):
        d = LC.make(fam, *c)
        if T * B * H > 130 * 9 * 40:          # the CPU suite asserts the smaller ones once
            LC.preconditions(d)
        h, dr, w = bfd(d["h"], cuda), bfd(d["dr"], cuda), bfd(d["w"], cuda)
        lens = d["lens"].to(cuda)
        r, dh = G((T, B, H), BFT, cuda), G((T, B, H), BFT, cuda)
        C.lookahead(h, w, lens, r.t, False)
        C.lookahead(dr, w, lens, dh.t, True)
        r.verify("lookahead_fwd %s" % LC.ident(c))
        dh.verify("lookahead_bwd_data %s" % LC.ident(c))
        LC.verify_fwd(d, r.t)
        LC.verify_bwd_data(d, dh.t)
        dw1 = _wgrad(C, dr, h, lens, tau, cuda, "lookahead_bwd_weight %s" % LC.ident(c))
        LC.verify_bwd_weight(d, dw1)
        dw2 = _wgrad(C, dr, h, lens, tau, cuda, "lookahead_bwd_weight %s (again)" % LC.ident(c))
        assert torch.equal(dw1, dw2), "the weight gradient is not reproducible from run to run"


def test_weight_gradient_accumulates_and_ops_pick_the_kernels(cuda):
    """ops/lookahead.py on operands inside the contract: the kernels' results, bit for bit; the
    accumulate flag adds to what is there."""
    from deepspeech_amd.ops import lookahead as LA
    C = _ext()
    d = LC.make("B", 7, 67, 9, 40)
    h, dr, w = bfd(d["h"], cuda), bfd(d["dr"], cuda), bfd(d["w"], cuda)
    lens = d["lens"].to(cuda)
    assert LA.kernels_cover(h, w)
    r = torch.empty_like(h)
    C.lookahead(h, w, lens, r, False)
    assert torch.equal(LA.lookahead_fwd(h, w, lens), r)
    assert torch.equal(LA.lookahead_fwd(h, w, d["lens"].to(torch.int64)), r)          # lens of any int type / device
    dw = torch.empty(40, 8, device=cuda)
    LA.lookahead_bwd_weight(dr, h, lens, 7, dw)
    LC.verify_bwd_weight(d, dw)
    twice = torch.full((40, 8), 3.0, device=cuda)
    LA.lookahead_bwd_weight(dr, h, lens, 7, twice, accumulate=True)
    assert torch.equal(twice, dw + 3.0)


@pytest.mark.parametrize("c", [(1, 20, 1, 8), (2, 29, 3, 40), (7, 67, 3, 800), (20, 67, 9, 40), (31, 130, 2, 800),
                               (31, 20, 3, 8)], ids=LC.ident)
def test_stream_equals_whole_sequence(cuda, c):
    """Chunks of 1, 3 and 13 frames, then the zero flush: the streaming kernel's outputs, delayed
    by tau frames, are bitwise the whole-sequence forward (every stream has length T here)."""
    C = _ext()
    tau, T, B, H = c
    d = LC.make("B", *c)
    h, w = bfd(d["h"], cuda), bfd(d["w"], cuda)
    full = torch.empty_like(h)
    C.lookahead(h, w, torch.full((B,), T, dtype=torch.int32, device=cuda), full, False)
    hist = G((tau, B, H), BFT, cuda)
    hist.t.zero_()
    outs, t, sizes = [], 0, (1, 3, 13)
    while t < T:
        n = min(sizes[len(outs) % 3], T - t)
        o = G((n, B, H), BFT, cuda)
        C.lookahead_stream(hist.t, h[t:t + n], w, o.t)
        o.verify("lookahead_stream out")
        outs.append(o.t)
        t += n
    assert torch.equal(hist.t, h[T - tau:] if T >= tau else torch.cat([torch.zeros_like(h[:tau - T]), h], 0))
    o = G((tau, B, H), BFT, cuda)
    C.lookahead_stream(hist.t, torch.zeros(tau, B, H, dtype=BFT, device=cuda), w, o.t)
    outs.append(o.t)
    hist.verify("lookahead_stream hist")
    got = torch.cat(outs, 0)
    assert got.shape[0] == T + tau
    assert torch.equal(got[tau:], full)


def test_outside_the_contract_takes_the_composite(cuda):
    """H % 8 != 0, fp32, a non-contiguous tensor, tau > 31: the torch composite on the same
    device, checked against the oracle (fp32 arithmetic: tolerance K eps S with K = 2 (tau + 1)
    for the products' own rounding, plus the bf16 store where the output is bf16)."""
    from deepspeech_amd.ops import lookahead as LA
    g = torch.Generator().manual_seed(5)
    lens = torch.tensor([11, 1, 7], dtype=torch.int32)

    def run(h, dr, w, cover_expected=False):
        assert LA.kernels_cover(h, w) == cover_expected
        tau = w.shape[1] - 1
        h64, dr64, w64 = h.detach().cpu().to(F64), dr.detach().cpu().to(F64), w.detach().cpu().to(F64)
        r, dh, dw = LC.oracle(h64, dr64, w64, lens)
        Sr, Sd, Sw = LC.oracle(h64.abs(), dr64.abs(), w64.abs(), lens)
        store = (lambda v, dd: CO.hulp(v.abs() + dd)) if h.dtype == BFT else (lambda v, dd: 0)
        k = 2 * (tau + 1) * LC.EPS
        got_r = LA.lookahead_fwd(h, w, lens.to(h.device))
        got_dh = LA.lookahead_bwd_data(dr, w, lens.to(h.device))
        got_dw = torch.empty(w.shape, device=h.device, dtype=F32)
        LA.lookahead_bwd_weight(dr, h, lens.to(h.device), tau, got_dw)
        assert got_r.device == h.device and got_r.dtype == h.dtype and got_r.shape == h.shape
        CO.check("composite r", got_r, r, k * Sr + store(r, k * Sr), LC.DIMS)
        CO.check("composite dh", got_dh, dh, k * Sd + store(dh, k * Sd), LC.DIMS)
        CO.check("composite dw", got_dw, dw, 2 * h.shape[0] * h.shape[1] * LC.EPS * Sw, ("i", "j"))

    rn = lambda *s: torch.randn(*s, generator=g).to(BFT)
    run(rn(11, 3, 12).to(cuda), rn(11, 3, 12).to(cuda), rn(12, 4).to(cuda))                      # H % 8 != 0
    run(rn(11, 3, 16).float().to(cuda), rn(11, 3, 16).float().to(cuda), rn(16, 4).to(cuda))      # fp32
    wide = rn(11, 3, 32).to(cuda)
    run(wide[:, :, ::2], rn(11, 3, 16).to(cuda), rn(16, 4).to(cuda))                              # non-contiguous
    run(rn(11, 3, 16).to(cuda), rn(11, 3, 16).to(cuda), rn(16, 33).to(cuda))                      # tau = 32
    run(rn(11, 3, 16).to(cuda), rn(11, 3, 16).to(cuda), rn(16, 4).to(cuda), cover_expected=True)  # the control


# ------------------------------------------------------------------------------ engine wiring
TAU = 5


def _identity(H, tau, dev):
    w = torch.zeros(H, tau + 1, device=dev)
    w[:, 0] = 1
    return w


def _uni_pair(cuda, tau=TAU):
    """(model without the layer, the same weights with an identity lookahead layer), HIP engine"""
    torch.manual_seed(21)
    kw = dict(num_filters=32, num_hidden=128, num_rnn_layers=2, cell="gru", bidirectional=False)
    m0 = DeepSpeech2(**kw).to(cuda)
    m1 = DeepSpeech2(lookahead=tau, **kw).to(cuda)
    m1.load_state_dict(m0.state_dict(), strict=False)
    assert torch.equal(m1.lookahead_weight.detach(), _identity(128, tau, cuda))
    return m0.set_engine("hip", BFT), m1.set_engine("hip", BFT)


def _batches(cuda, n=3):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    feed = FixedShapeBatches(6, max_frames=260, seed=3, pool=n)
    return [to_device(feed.next(), cuda) for _ in range(n)]


def test_identity_layer_changes_no_loss_and_no_gradient(cuda):
    """Fused head + CTC path with an arena: r == h and dh == dr bitwise under identity weights, so
    the loss and every other parameter's gradient are those of the model without the layer."""
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.ops.optim import ParamArena
    m0, m1 = _uni_pair(cuda)
    b = _batches(cuda, 1)[0]
    out = []
    for m in (m0, m1):
        arena = ParamArena(m, bf16_shadow=True)
        arena.zero_grad()
        m.train()
        loss = m.forward_loss(b["feats"], b["seq_lens"], b["labels"], b["label_lens"])
        loss.backward()
        RNN.join_wgrad_streams()
        torch.cuda.synchronize()
        RNN.check_errors()
        out.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = out
    assert torch.equal(l0, l1), (float(l0), float(l1))
    for n, g in g0.items():
        assert torch.equal(g, g1[n]), n
    gw = g1["lookahead_weight"]
    assert torch.isfinite(gw).all() and float(gw.abs().sum()) > 0


def _run_trainer(m, batches, freeze, **kw):
    from deepspeech_amd.trainer import LRSchedule, Trainer
    tr = Trainer(m, LRSchedule(1e-3, 2, 0.5), **kw)
    losses = []
    for b in batches:
        losses.append(float(tr.step(b)))
        if freeze:
            # the new parameter's learning effect removed: the identity again, master and shadow
            tr.flush()
            w = tr.model.lookahead_weight
            with torch.no_grad():
                w.copy_(_identity(w.shape[0], w.shape[1] - 1, w.device))
                w.bf16.copy_(w)
    tr.flush()
    torch.cuda.synchronize()
    views = {k: tr.arena.views(buf) for k, buf in (("flat", tr.arena.flat), ("m", tr.opt.m), ("v", tr.opt.v),
                                                   ("ema", tr.opt.ema), ("p16", tr.arena.p16))}
    return losses, views


@pytest.fixture(scope="module")
def plain_trajectory(cuda):
    m0, _ = _uni_pair(cuda)
    return _run_trainer(m0, _batches(cuda), False)


@pytest.mark.parametrize("kw", [dict(), dict(step_graphs=True, graph_warmup=1), dict(defer_update=True)],
                         ids=["eager", "step-graphs", "carried-update"])
def test_trainer_steps_with_frozen_identity_layer(cuda, plain_trajectory, kw):
    """Three Trainer steps (the LR decays once): with the lookahead weights put back to the
    identity after every step, losses, weights, Adam moments, EMA and shadows of every other
    parameter are bitwise those of the model without the layer, eager, through step graphs and
    with the optimizer update carried into the next forward."""
    l0, v0 = plain_trajectory
    _, m1 = _uni_pair(cuda)
    l1, v1 = _run_trainer(m1, _batches(cuda), True, **kw)
    assert l0 == l1
    for k, views in v0.items():
        for n, t in views.items():
            assert torch.equal(t, v1[k][n]), (k, n)


def test_step_graphs_equal_eager_with_a_learning_layer(cuda):
    _, a = _uni_pair(cuda)
    b = copy.deepcopy(a)
    for m in (a, b):
        with torch.no_grad():
            m.lookahead_weight.copy_(torch.randn(128, TAU + 1, generator=torch.Generator().manual_seed(1)) * 0.4)
    la, va = _run_trainer(a, _batches(cuda), False)
    lb, vb = _run_trainer(b, _batches(cuda), False, step_graphs=True, graph_warmup=1)
    assert la == lb
    for k, views in va.items():
        for n, t in views.items():
            assert torch.equal(t, vb[k][n]), (k, n)
    assert not torch.equal(va["flat"]["lookahead_weight"], _identity(128, TAU, cuda))


@pytest.mark.parametrize("bidir", [False, True], ids=["uni", "bidir"])
def test_model_grads_match_reference(cuda, bidir):
    """As tests/test_engine_gpu.py::test_model_grads_match_reference (its shape, its bounds:
    relative loss error < 3e-2, relative L2 gradient error <= 0.06 for every non-conv parameter,
    lookahead_weight included, its conv bounds), with a random lookahead layer, tau = 5."""
    import test_engine_gpu as TE
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.ops.optim import ParamArena
    torch.manual_seed(11)
    ref = DeepSpeech2(num_filters=32, num_hidden=64, num_rnn_layers=2, cell="gru", bidirectional=bidir,
                      lookahead=TAU).to(cuda)
    with torch.no_grad():
        ref.lookahead_weight.normal_(0.0, (TAU + 1) ** -0.5)
    hip = copy.deepcopy(ref)
    ref.set_engine("ref", F32)
    hip.set_engine("hip", BFT)
    batch = to_device(FixedShapeBatches(6, max_frames=260, seed=3, pool=1).next(), cuda)
    arena = ParamArena(hip, bf16_shadow=True)
    arena.zero_grad()
    lh = TE._loss(hip, batch, True)
    lh.backward()
    RNN.join_wgrad_streams()
    lr = TE._loss(ref, batch)
    lr.backward()
    torch.cuda.synchronize()
    RNN.check_errors()
    errs = TE._compare_grads(ref, hip, lh, lr, "gru")
    print("LOOKGRAD %s lookahead_weight rel L2 %.5f loss rel %.2e" % (
        "bidir" if bidir else "uni", errs["lookahead_weight"], abs(float(lh) - float(lr)) / abs(float(lr))))


# ------------------------------------------------------------------------------ recogniser
def _stream(m, feats, chunk, **kw):
    from deepspeech_amd.infer import StreamingRecognizer
    rec = StreamingRecognizer(m, batch=feats.shape[0], **kw)
    for s in range(0, feats.shape[1], chunk):
        rec.accept(feats[:, s:s + chunk])
    hyp = rec.finish()
    return rec, hyp


def _feats(cuda, T=421):
    return torch.randn(2, T, 161, generator=torch.Generator().manual_seed(8)).to(cuda)


def test_recogniser_identity_layer_equals_no_layer(cuda):
    from deepspeech_amd.infer import frames_out
    m0, m1 = _uni_pair(cuda)
    feats = _feats(cuda)
    for chunk in (37, 100):              # 37: the first chunk emits nothing
        r0, h0 = _stream(m0, feats, chunk)
        r1, h1 = _stream(m1, feats, chunk)
        a, b = torch.cat(r0.logprobs, 0), torch.cat(r1.logprobs, 0)
        assert a.shape == b.shape == (frames_out(421), 2, 29)
        assert torch.equal(a, b) and h0 == h1
        assert r1.finish() == h1 and sum(lp.shape[0] for lp in r1.logprobs) == frames_out(421)


def test_recogniser_graphs_equal_eager(cuda):
    from deepspeech_amd.infer import frames_out
    _, m1 = _uni_pair(cuda)
    with torch.no_grad():
        m1.lookahead_weight.copy_(torch.randn(128, TAU + 1, generator=torch.Generator().manual_seed(2)) * 0.4)
    feats = _feats(cuda)
    for chunk in (37, 100, 163):
        rg, hg = _stream(m1, feats, chunk, graphs=True)
        re, he = _stream(m1, feats, chunk, graphs=False)
        assert rg.use_graphs and not re.use_graphs
        # several chunks of one shape, so graphs are replayed; the dropped frames are in the key
        assert any(k[-1] > 0 for k in rg._graphs) and any(k[-1] == 0 for k in rg._graphs)
        a, b = torch.cat(rg.logprobs, 0), torch.cat(re.logprobs, 0)
        assert a.shape == (frames_out(421), 2, 29) and torch.equal(a, b) and hg == he
    # a second stream through the same recogniser (reset zeroes hist inside the graphs' buffers)
    rg.reset()
    for s in range(0, 421, 163):
        rg.accept(feats[:, s:s + 163])
    rg.finish()
    assert torch.equal(torch.cat(rg.logprobs, 0), a)


def test_recogniser_beam_decoder_sees_the_flushed_frames(cuda):
    from deepspeech_amd.infer import frames_out
    from deepspeech_amd.ops.decode import beam_decode
    _, m1 = _uni_pair(cuda)
    with torch.no_grad():
        m1.lookahead_weight.copy_(torch.randn(128, TAU + 1, generator=torch.Generator().manual_seed(2)) * 0.4)
    feats = torch.randn(2, 50 * 6 + 38, 161, generator=torch.Generator().manual_seed(0)).to(cuda)
    rec, got = _stream(m1, feats, 50, decoder="beam", beam_width=16)
    assert rec.gbeams is not None
    lp = torch.cat(rec.logprobs, 0)
    assert lp.shape[0] == frames_out(feats.shape[1])
    assert got == beam_decode(lp, torch.full((2,), lp.shape[0], dtype=torch.int32), 16)
    assert rec.finish() == got
