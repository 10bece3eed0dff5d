"""Lookahead convolution without a GPU: the pure-torch reference against literal loops, its
gradients, the model / arena / flag / checkpoint wiring, and the streaming recogniser's delay and
flush on the reference engine. The definition and the case grid are in tests/lookahead_cases.py."""
import json

import pytest
import torch

import lookahead_cases as LC
from deepspeech_amd import config as C
from deepspeech_amd.infer import StreamingRecognizer, frames_out
from deepspeech_amd.models import DeepSpeech2
from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops.optim import ParamArena
from deepspeech_amd.trainer import LRSchedule, Trainer
from deepspeech_amd.utils import checkpoint as CK

F64 = torch.float64


# ------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("c", LC.SMALL, ids=LC.ident)
def test_reference_and_oracle_against_loops(c):
    d = LC.make("B", *c)
    r, dh, dw = LC.loops(d["h"], d["dr"], d["w"], d["lens"])
    for got, want in ((d["r"], r), (d["dh"], dh), (d["dw"], dw)):
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
    h = d["h"].clone().requires_grad_(True)
    w = d["w"].clone().requires_grad_(True)
    out = R.lookahead_ref(h, w, d["lens"])
    assert out.dtype == F64 and torch.allclose(out, r, rtol=0, atol=1e-12)
    out.backward(d["dr"])            # dr is nonzero at invalid positions: it must be ignored
    assert torch.allclose(h.grad, dh, rtol=0, atol=1e-12)
    assert torch.allclose(w.grad, dw, rtol=0, atol=1e-11)


@pytest.mark.parametrize("fam", ["A", "B"])
def test_families_keep_their_promises(fam):
    for c in LC.GRID:
        if c[1] * c[2] * c[3] <= 130 * 9 * 40:
            LC.preconditions(LC.make(fam, *c))
    LC.preconditions(LC.make(fam, 20, 130, 9, 800) if (20, 130, 9, 800) in LC.GRID else LC.make(fam, *LC.GRID[-1]))


def test_grid_covers_every_value():
    assert {c[0] for c in LC.GRID} == set(LC.TAUS)
    for tau in LC.TAUS:
        mine = [c for c in LC.GRID if c[0] == tau]
        assert {c[1] for c in mine} == set(LC.t_values(tau))
        assert {(c[2], c[3]) for c in mine} == {(b, h) for b in LC.BS for h in LC.HS}


def test_gradcheck_ragged():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(9, 3, 4, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(4, 4, generator=g, dtype=F64, requires_grad=True)
    lens = torch.tensor([9, 1, 6], dtype=torch.int32)
    assert torch.autograd.gradcheck(lambda a, b: R.lookahead_ref(a, b, lens), (h, w))


def test_op_composite_on_cpu_matches_reference():
    """Outside the kernels' contract (here: CPU, fp32) LookaheadConv is the torch composite."""
    from deepspeech_amd.ops.lookahead import LookaheadConv
    d = LC.make("B", 7, 9, 3, 40)
    h = d["h"].float().requires_grad_(True)
    w = torch.nn.Parameter(d["w"].float())
    r = LookaheadConv.apply(h, w, d["lens"])
    r.backward(d["dr"].float())
    assert torch.allclose(r.double(), d["r"], atol=1e-5)
    assert torch.allclose(h.grad.double(), d["dh"], atol=1e-5)
    assert torch.allclose(w.grad.double(), d["dw"], atol=1e-4)


# ------------------------------------------------------------------------------ model wiring
def _models(tau=7, **kw):
    torch.manual_seed(3)
    base = dict(num_filters=4, num_hidden=16, num_rnn_layers=2, cell="gru", bidirectional=False)
    base.update(kw)
    m0 = DeepSpeech2(**base)
    m1 = DeepSpeech2(lookahead=tau, **base)
    missing = m1.load_state_dict(m0.state_dict(), strict=False)
    assert missing.missing_keys == ["lookahead_weight"] and not missing.unexpected_keys
    return m0, m1


@pytest.mark.parametrize("kw", [dict(), dict(bidirectional=True), dict(bidirectional=True, layout="nhwc")],
                         ids=["uni", "bidir", "direction-stacks"])
def test_identity_weights_change_nothing(kw):
    m0, m1 = _models(7, **kw)
    ident = torch.zeros(16, 8)
    ident[:, 0] = 1
    assert torch.equal(m1.lookahead_weight.detach(), ident)
    feats = torch.randn(3, 150, 161)
    seq = torch.tensor([150, 97, 120], dtype=torch.int32)
    with torch.no_grad():
        a, la = m0.eval()(feats, seq)
        m1.eval().capture = True
        b, lb = m1(feats, seq)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert "lookahead" in m1.act_taps and m1.act_taps["lookahead"].shape == m1.act_taps["rnn"].shape
    # and a non-identity layer does change them, through forward_loss too
    with torch.no_grad():
        m1.lookahead_weight.normal_()
        c, _ = m1(feats, seq)
    assert not torch.equal(a, c)
    labels = torch.randint(0, 28, (3, 5))
    ll = torch.full((3,), 5, dtype=torch.int32)
    m1.train()
    m1.forward_loss(feats, seq, labels, ll).backward()
    assert m1.lookahead_weight.grad is not None and float(m1.lookahead_weight.grad.abs().sum()) > 0


def test_no_lookahead_registers_nothing():
    kw = dict(num_filters=4, num_hidden=16, num_rnn_layers=2, cell="gru", bidirectional=False)
    plain, zero, la = DeepSpeech2(**kw), DeepSpeech2(lookahead=0, **kw), DeepSpeech2(lookahead=5, **kw)
    names = [n for n, _ in plain.named_parameters()]
    assert names == [n for n, _ in zero.named_parameters()] and not any("lookahead" in n for n in names)
    with_layer = [n for n, _ in la.named_parameters()]
    assert with_layer.count("lookahead_weight") == 1 and [n for n in with_layer if n != "lookahead_weight"] == names
    tf0 = [(a, b) for a, b, _, _ in CK.tf_name_map(zero)]
    assert tf0 == [(a, b) for a, b, _, _ in CK.tf_name_map(plain)] and not any("lookahead" in a for a, _ in tf0)
    assert [(a, b) for a, b, _, _ in CK.tf_name_map(la)] == tf0 + [("lookahead/weights", "lookahead_weight")]
    assert [[n for n, _ in g] for g in zero.arena_groups()] == [[n for n, _ in g] for g in plain.arena_groups()]
    f0, f1 = zero.flops_breakdown(2, 200), la.flops_breakdown(2, 200)
    assert "lookahead" not in f0 and f0 == plain.flops_breakdown(2, 200)
    assert f1.pop("lookahead") == 2.0 * 2 * frames_out(200) * 16 * 6 and f1 == f0
    with pytest.raises(ValueError):
        DeepSpeech2(lookahead=32, **kw)


def test_arena_places_it_after_the_head():
    _, m1 = _models(5)
    arena = ParamArena(m1)
    i = arena.names.index("fc_weight")
    assert arena.names[:i + 2] == ["fc_bias", "fc_weight", "lookahead_weight"]
    assert arena.names[i + 2].startswith("rnn.1.")


def test_flag_round_trip(tmp_path):
    a = C.parse_train_args(["--lookahead", "20", "--rnn_type", "uni-dir", "--train_dir", str(tmp_path)])
    assert a.lookahead == 20 and C.model_kwargs_from_args(a)["lookahead"] == 20
    assert C.parse_train_args([]).lookahead == 0 and C.model_kwargs_from_args(C.parse_train_args([]))["lookahead"] == 0
    C.dump_param_json(a, str(tmp_path))
    b = C.parse_train_args(["--checkpoint", str(tmp_path)])
    assert b.lookahead == 20
    e = C.parse_eval_args(["--checkpoint_dir", str(tmp_path)])
    assert C.model_kwargs_from_args(e)["lookahead"] == 20
    assert DeepSpeech2(**dict(C.model_kwargs_from_args(e), num_hidden=16, num_filters=4)).lookahead == 20
    # a parameter file from before the flag rebuilds the model without the layer
    old = tmp_path / "old"
    old.mkdir()
    json.dump({"num_hidden": 64, "num_rnn_layers": 3, "rnn_type": "uni-dir", "num_filters": 8, "use_fp16": False},
              open(old / "deepSpeech_parameters.json", "w"))
    assert C.model_kwargs_from_args(C.parse_eval_args(["--checkpoint_dir", str(old)]))["lookahead"] == 0


def _trainer(tau):
    torch.manual_seed(0)
    m = DeepSpeech2(num_filters=4, num_hidden=16, num_rnn_layers=2, cell="gru", bidirectional=False, lookahead=tau)
    return Trainer(m, LRSchedule(1e-3, 100, 0.9), moving_avg_decay=0.99)


def _batch():
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    return to_device(FixedShapeBatches(2, max_frames=120, seed=0, pool=1).next(), torch.device("cpu"))


@pytest.mark.parametrize("fmt", ["tf", "torch"])
def test_checkpoint_round_trip(tmp_path, fmt):
    t = _trainer(5)
    b = _batch()
    for _ in range(2):
        t.step(b)
    ident = torch.zeros(16, 6)
    ident[:, 0] = 1
    assert not torch.equal(t.model.lookahead_weight.detach(), ident)          # it learns
    mgr = CK.CheckpointManager(str(tmp_path), async_save=False, fmt=fmt)
    path = mgr.save(t, 2)
    data = CK.load_checkpoint_file(path)
    ema = t.arena.views(t.opt.ema)["lookahead_weight"]
    assert torch.equal(data["lookahead/weights"], t.model.lookahead_weight.detach())
    assert torch.equal(data["lookahead/weights/ExponentialMovingAverage"], ema)
    assert "lookahead/weights" + CK.ADAM_M in data and "lookahead/weights" + CK.ADAM_V in data
    t2 = _trainer(5)
    CK.restore(t2, str(tmp_path))
    assert torch.equal(t2.model.lookahead_weight, t.model.lookahead_weight)
    assert torch.equal(t2.arena.views(t2.opt.ema)["lookahead_weight"], ema)
    assert torch.equal(t2.opt.m, t.opt.m) and torch.equal(t2.opt.v, t.opt.v)
    # evaluation weights: the EMA slot
    m = DeepSpeech2(num_filters=4, num_hidden=16, num_rnn_layers=2, cell="gru", bidirectional=False, lookahead=5)
    CK.load_model_from_tf(m, {k: v for k, v in data.items() if torch.is_tensor(v)}, use_ema=True)
    assert torch.equal(m.lookahead_weight.detach(), ema)


def test_strict_restore_of_a_checkpoint_without_the_layer_raises(tmp_path):
    t0 = _trainer(0)
    t0.step(_batch())
    CK.CheckpointManager(str(tmp_path), async_save=False).save(t0, 1)
    with pytest.raises(KeyError, match="lookahead/weights"):
        CK.restore(_trainer(5), str(tmp_path))


# ------------------------------------------------------------------------------ streaming
def _stream_model(tau=5):
    from test_streaming import _model
    base = _model()
    torch.manual_seed(9)
    m = DeepSpeech2(num_filters=4, num_hidden=48, num_rnn_layers=2, cell="gru", bidirectional=False, lookahead=tau)
    m.load_state_dict(base.state_dict(), strict=False)
    with torch.no_grad():
        m.lookahead_weight.normal_(0.0, (tau + 1) ** -0.5)
    return m.eval()


@pytest.mark.parametrize("chunk", [37, 100, 163])
def test_stream_matches_full_utterance(chunk):
    tau = 5
    m = _stream_model(tau)
    T, B = 421, 2
    feats = torch.randn(B, T, 161, generator=torch.Generator().manual_seed(chunk))
    with torch.no_grad():
        logits, lens = m(feats, torch.full((B,), T, dtype=torch.int32))
    full = torch.log_softmax(logits.float(), -1)
    rec = StreamingRecognizer(m, batch=B)
    rows = []
    for s in range(0, T, chunk):
        rec.accept(feats[:, s:s + chunk])
        rows.append(sum(lp.shape[0] for lp in rec.logprobs))
        assert rows[-1] == max(0, rec.done - tau) == rec.emitted          # the output lags by tau frames
    assert rows[0] < frames_out(chunk) or frames_out(chunk) == 0
    hyp = rec.finish()
    got = torch.cat(rec.logprobs, 0)
    assert got.shape == full.shape == (frames_out(T), B, 29)
    assert torch.allclose(got, full, atol=2e-4), (got - full).abs().max()
    assert hyp == R.greedy_decode(full, lens)
    assert rec.finish() == hyp and sum(lp.shape[0] for lp in rec.logprobs) == frames_out(T)      # flushed once
    with pytest.raises(RuntimeError):
        rec.accept(feats[:, :chunk])
    rec.reset()
    assert rec.emitted == 0 and float(rec._hist.abs().sum()) == 0.0
    rec.accept(feats[:, :200])
    rec.finish()
    assert torch.allclose(torch.cat(rec.logprobs, 0)[:10], got[:10], atol=2e-4)


def test_stream_shorter_than_the_lookahead():
    tau = 5
    m = _stream_model(tau)
    T, B = 38 + 4 * 2, 2                                   # 3 output frames < tau
    assert 0 < frames_out(T) < tau
    feats = torch.randn(B, T, 161, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        logits, _ = m(feats, torch.full((B,), T, dtype=torch.int32))
    full = torch.log_softmax(logits.float(), -1)
    rec = StreamingRecognizer(m, batch=B)
    rec.accept(feats[:, :41])
    rec.accept(feats[:, 41:])
    assert rec.logprobs == []
    rec.finish()
    got = torch.cat(rec.logprobs, 0)
    assert got.shape == full.shape == (frames_out(T), B, 29)
    assert torch.allclose(got, full, atol=2e-4)
    empty = StreamingRecognizer(m, batch=B)
    assert empty.finish() == [[], []] and empty.logprobs == []


def test_finish_timed_flushes_first():
    m = _stream_model(5)
    T, B = 300, 1
    feats = torch.randn(B, T, 161, generator=torch.Generator().manual_seed(2))
    rec = StreamingRecognizer(m, batch=B)
    for s in range(0, T, 100):
        rec.accept(feats[:, s:s + 100])
    rec.finish_timed()
    assert sum(lp.shape[0] for lp in rec.logprobs) == frames_out(T)
