"""csrc/dropout.hip against the integer oracle (bitwise, tests/dropout_cases.py), then the wiring:
the fallback outside the kernel's contract, the autograd op, the HIP model, Trainer steps eager,
through step graphs and with the carried optimizer update, and the whole model against the
``ref`` engine under the same masks.

Printed (run with -s): DROPGRAD lines, the loss and worst gradient errors of the parity test with
dropout on next to a dropout-off run of the same models. profiles/dropout.md records them.
"""
import copy

import pytest
import torch

import conv_cases as CO
import dropout_cases as DC
from deepspeech_amd.models import DeepSpeech2
from deepspeech_amd.ops import dropout as D
from deepspeech_amd.ops import reference as R

pytestmark = pytest.mark.gpu
BFT, F32 = torch.bfloat16, torch.float32


def _ext():
    from deepspeech_amd.ops import _ext
    return _ext.ext()


def _launch(x, out, ctr, thr, locked, site, seed=DC.SEED):
    _ext().seq_dropout(x, out, ctr, seed & 0xffffffff, seed >> 32, site, thr, R.seq_dropout_scale(thr), locked)


# ------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("shape", DC.SHAPES, ids=DC.ident)
def test_kernel_equals_oracle(cuda, shape):
    """Out of place into a guarded buffer and in place on a guarded copy, the full parameter
    cross: both equal the oracle bitwise, the input is unchanged, nothing outside is written."""
    x = DC.inputs(shape, sum(shape))
    xd = x.to(cuda)
    st = D.DropoutState(cuda)
    assert D.kernel_covers(xd, st.ctr)
    for thr, locked, site, step, fu in DC.PARAMS:
        st.set(step, fu)
        want = DC.oracle(x, thr, locked, site, step, fu)
        out = CO.Guarded(shape, BFT, cuda)
        _launch(xd, out.t, st.ctr, thr, locked, site)
        out.verify("out of place")
        assert torch.equal(out.t.cpu(), want), (thr, locked, site, step, fu)
        inp = CO.Guarded(shape, BFT, cuda)
        inp.t.copy_(xd)
        _launch(inp.t, inp.t, st.ctr, thr, locked, site)
        inp.verify("in place")
        assert torch.equal(inp.t, out.t), (thr, locked, site, step, fu)
    assert torch.equal(xd.cpu(), x)


def test_kernel_seed_words_inf_and_nan(cuda):
    shape, thr, site = (3, 2, 40), 32768, 5
    seed = (0x9abcdef0 << 32) | 0x12345678
    x = DC.inputs(shape, 9)
    keep = R.seq_dropout_mask_ref(*shape, seed, 7, 0, site, thr, False)
    dropped, kept = (~keep).nonzero(), keep.nonzero()
    cells = [tuple(dropped[0]), tuple(dropped[1]), tuple(kept[0]), tuple(kept[1])]
    for c, v in zip(cells, (float("inf"), float("nan"), float("-inf"), float("nan"))):
        x[c] = v
    st = D.DropoutState(cuda)
    st.set(7, 0)
    xd = x.to(cuda)
    y = torch.empty_like(xd)
    _launch(xd, y, st.ctr, thr, False, site, seed)
    y = y.cpu()
    want = DC.oracle(x, thr, False, site, 7, 0, seed)
    assert float(y[cells[0]]) == 0 and float(y[cells[1]]) == 0 and float(y[cells[2]]) == float("-inf")
    assert bool(torch.isnan(y[cells[3]])) and int(torch.isnan(y).sum()) == 1
    assert torch.equal(torch.nan_to_num(y, nan=3.0), torch.nan_to_num(want, nan=3.0))
    assert not bool(torch.signbit(y[~keep]).any())


def test_fallback_outside_the_contract(cuda):
    """fp32, H = 12, a non-contiguous view and a CPU tensor take the composite: the oracle's bits."""
    st = D.DropoutState(cuda)
    st.set(7, 3)
    wide = DC.inputs((4, 3, 32), 4).to(cuda)
    cases = [DC.inputs((4, 3, 16), 1, F32).to(cuda), DC.inputs((4, 3, 12), 2).to(cuda), wide[:, :, ::2],
             wide[:, :, 4:20]]
    for x in cases:
        assert not D.kernel_covers(x, st.ctr)
        y = D.seq_dropout(x, st, DC.SEED, 2, 13107, "locked")
        assert y.device == x.device and DC.same_bits(y, DC.oracle(x, 13107, True, 2, 7, 3))
    cpu = D.DropoutState("cpu")
    cpu.set(7, 3)
    x = DC.inputs((4, 3, 16), 5)
    assert DC.same_bits(D.seq_dropout(x, cpu, DC.SEED, 2, 13107), DC.oracle(x, 13107, False, 2, 7, 3))
    ok = DC.inputs((4, 3, 16), 6).to(cuda)
    assert D.kernel_covers(ok, st.ctr) and not D.kernel_covers(ok, cpu.ctr)
    assert torch.equal(D.seq_dropout(ok, st, DC.SEED, 2, 13107).cpu(), DC.oracle(ok, 13107, False, 2, 7, 3))
    assert D.seq_dropout(ok, st, DC.SEED, 2, 0) is ok


@pytest.mark.parametrize("grad_inplace", [False, True], ids=["copy", "inplace"])
def test_op_backward_follows_ctr(cuda, grad_inplace):
    shape, thr, site = (33, 5, 264), 16384, 3
    st = D.DropoutState(cuda)
    x = DC.inputs(shape, 1).to(cuda).requires_grad_(True)
    dy = DC.inputs(shape, 2)
    ptr = st.ctr.data_ptr()
    for step, fu in ((7, 0), (8, 4)):
        st.set(step, fu)
        x.grad = None
        y = D.seq_dropout(x, st, DC.SEED, site, thr, "element", grad_inplace=grad_inplace)
        assert y.grad_fn is not None and len(y.grad_fn.saved_tensors) == 0     # nothing kept but ctr and constants
        g = dy.to(cuda)
        y.backward(g)
        assert torch.equal(y.detach().cpu(), DC.oracle(x, thr, False, site, step, fu))
        assert torch.equal(x.grad.cpu(), DC.oracle(dy, thr, False, site, step, fu))
        # in place the incoming gradient itself was rewritten, otherwise it is left as it came
        assert torch.equal(g, x.grad) if grad_inplace else torch.equal(g.cpu(), dy)
    assert st.ctr.data_ptr() == ptr
    # the mask is drawn when the kernel runs: a backward after ctr moved on takes the new words
    st.set(7, 0)
    x.grad = None
    y = D.seq_dropout(x, st, DC.SEED, site, thr)
    st.set(8, 4)
    y.backward(dy.to(cuda))
    assert torch.equal(x.grad.cpu(), DC.oracle(dy, thr, False, site, 8, 4))


# ------------------------------------------------------------------------------ the HIP model
def _batches(cuda, n=3):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    feed = FixedShapeBatches(6, max_frames=260, seed=3, pool=n)
    return [to_device(feed.next(), cuda) for _ in range(n)]


@pytest.mark.parametrize("kw", [dict(num_hidden=128, num_rnn_layers=2, bidirectional=False),
                                dict(num_hidden=64, num_rnn_layers=3, bidirectional=True),
                                dict(num_hidden=64, num_rnn_layers=2, bidirectional=True, layout="nhwc")],
                         ids=["2xGRU-128", "3xBiGRU-64", "nhwc-stacks"])
def test_hip_model_wiring(cuda, monkeypatch, kw):
    """What layer i+1 receives (and FusedBiLayer keeps as its bf16 input) is the oracle applied to
    layer i's output, bitwise; the top output is not dropped; eval() launches nothing."""
    from deepspeech_amd.ops import rnn as RNN
    torch.manual_seed(5)
    m = DeepSpeech2(num_filters=32, cell="gru", rnn_dropout=0.25, **kw).to(cuda).set_engine("hip", BFT)
    m.rnn_dropout_seed = DC.SEED
    split = m.direction_stacks()
    taps = []
    name = "recurrent_layer_split_hip" if split else "recurrent_layer_hip"
    real = getattr(RNN, name)

    def tapped(layer, *a, **k):
        out = real(layer, *a, **k)
        taps.append((a[:2] if split else a[:1], out))
        return out
    monkeypatch.setattr(RNN, name, tapped)
    b = _batches(cuda, 1)[0]
    m.train()
    m.dropout_state.set(5, 2)
    m.capture = True
    with torch.no_grad():
        m(b["feats"], b["seq_lens"])
    L = kw["num_rnn_layers"]
    assert len(taps) == L
    for i in range(L - 1):
        outs = taps[i][1] if split else (taps[i][1],)
        for d, (o, nxt) in enumerate(zip(outs, taps[i + 1][0])):
            assert nxt.dtype == BFT and nxt.is_contiguous()
            assert torch.equal(nxt.cpu(), DC.oracle(o, 16384, False, 2 * i + d, 5, 2)), (i, d)
    top = taps[-1][1]
    assert torch.equal(m.act_taps["rnn"], top[0] + top[1] if split else top)
    RNN.check_errors()
    calls = []
    monkeypatch.setattr(D, "_apply", lambda *a, **k: calls.append(a) or a[0])
    m.eval()
    with torch.no_grad():
        m(b["feats"], b["seq_lens"])
    assert not calls


def _uni(cuda, **extra):
    """The small uni-GRU model of tests/test_lookahead_gpu.py (_uni_pair), HIP engine"""
    torch.manual_seed(21)
    m = DeepSpeech2(num_filters=32, num_hidden=128, num_rnn_layers=2, cell="gru", bidirectional=False, **extra)
    m.rnn_dropout_seed = DC.SEED
    return m.to(cuda).set_engine("hip", BFT)


def _run_trainer(m, batches, **kw):
    from deepspeech_amd.trainer import LRSchedule, Trainer
    tr = Trainer(m, LRSchedule(1e-3, 2, 0.5), **kw)
    tr.first_utt = 12
    losses = [float(tr.step(b)) for b in batches]
    tr.flush()
    torch.cuda.synchronize()
    views = {k: tr.arena.views(buf) for k, buf in (("flat", tr.arena.flat), ("m", tr.opt.m), ("v", tr.opt.v),
                                                   ("ema", tr.opt.ema), ("p16", tr.arena.p16))}
    return losses, views


def _same(a, b):
    (la, va), (lb, vb) = a, b
    assert la == lb, (la, lb)
    for k, views in va.items():
        for n, t in views.items():
            assert torch.equal(t, vb[k][n]), (k, n)


@pytest.fixture(scope="module")
def eager_trajectory(cuda):
    return _run_trainer(_uni(cuda, rnn_dropout=0.25), _batches(cuda))


@pytest.mark.parametrize("kw", [dict(step_graphs=True, graph_warmup=1), dict(defer_update=True)],
                         ids=["step-graphs", "carried-update"])
def test_trainer_steps_equal_eager(cuda, eager_trajectory, kw):
    """Three Trainer steps (the LR decays once) with rnn_dropout = 0.25: step graphs (one eager
    step, the capture, two replays) and the carried optimizer update give the eager run's losses,
    weights, Adam moments, EMA and shadows bitwise. A replay reads the step from the device: a
    step baked into the graph would repeat step 1's mask at step 2."""
    _same(eager_trajectory, _run_trainer(_uni(cuda, rnn_dropout=0.25), _batches(cuda), **kw))


def test_trainer_dropout_changes_and_zero_is_the_plain_model(cuda, eager_trajectory):
    plain = _run_trainer(_uni(cuda), _batches(cuda))
    _same(plain, _run_trainer(_uni(cuda, rnn_dropout=0.0, rnn_dropout_mode="locked"), _batches(cuda)))
    assert plain[0][0] != eager_trajectory[0][0] and all(l == l for l in eager_trajectory[0])
    # the masks follow the step: the same batch gives another loss at another step
    b = _batches(cuda, 1)[0]
    m = _uni(cuda, rnn_dropout=0.25)
    m.train()
    out = []
    for step in (0, 1, 0):
        m.dropout_state.set(step, 0)
        with torch.no_grad():
            out.append(float(m.forward_loss(b["feats"], b["seq_lens"], b["labels"], b["label_lens"])))
    assert out[0] == out[2] and out[0] != out[1]


# ------------------------------------------------------------------------------ parity with the ref engine
@pytest.mark.parametrize("bidir", [False, True], ids=["uni", "bidir"])
def test_model_grads_match_reference(cuda, bidir):
    """As tests/test_lookahead_gpu.py::test_model_grads_match_reference (its shape, 2 x GRU-64 on
    6 x 260 frames, and through test_engine_gpu._loss / _compare_grads its bounds: relative loss
    error < 3e-2, relative L2 gradient error <= 0.06 for every non-conv parameter, 0.12 for the
    conv front-end), with rnn_dropout = 0.25 on both engines, which draw the same integer mask.
    The dropout-off run of the same weights is printed next to it."""
    import test_engine_gpu as TE
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.ops.optim import ParamArena
    batch = _batches(cuda, 1)[0]
    rows = {}
    for p in (0.0, 0.25):
        torch.manual_seed(11)
        ref = DeepSpeech2(num_filters=32, num_hidden=64, num_rnn_layers=2, cell="gru", bidirectional=bidir,
                          rnn_dropout=p).to(cuda)
        ref.rnn_dropout_seed = DC.SEED
        hip = copy.deepcopy(ref)
        ref.set_engine("ref", F32)
        hip.set_engine("hip", BFT)
        for m in (ref, hip):
            if p:
                m.dropout_state.set(3, 6)
        arena = ParamArena(hip, bf16_shadow=True)
        arena.zero_grad()
        lh = TE._loss(hip, batch, True)
        lh.backward()
        RNN.join_wgrad_streams()
        lr = TE._loss(ref, batch)
        lr.backward()
        torch.cuda.synchronize()
        RNN.check_errors()
        lh, lr = lh.detach(), lr.detach()
        gref = dict((n, q.grad) for n, q in ref.named_parameters())
        errs = {n: TE._rel(q.grad, gref[n]) for n, q in hip.named_parameters() if not n.endswith(("conv1.bias",
                                                                                                  "conv2.bias"))}
        worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
        print("DROPGRAD %s p=%.2f loss hip %.5f ref %.5f rel %.2e; worst rel L2: %s" % (
            "bidir" if bidir else "uni", p, float(lh), float(lr), abs(float(lh) - float(lr)) / abs(float(lr)),
            ", ".join("%s %.4f" % kv for kv in worst)))
        rows[p] = (ref, hip, lh, lr)
    assert float(rows[0.25][3]) != float(rows[0.0][3])
    for p in (0.0, 0.25):
        TE._compare_grads(*rows[p], "gru")
