"""Dropout between recurrent layers on the CPU: the oracle against the definition, the composite
and its gradient, the model wiring on the ``ref`` engine, the driver flags and the kernel's
register budget. tests/dropout_cases.py holds the cases; the kernel itself is checked in
tests/test_dropout_gpu.py."""
import json
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

import dropout_cases as DC
from deepspeech_amd.models import DeepSpeech2
from deepspeech_amd.ops import dropout as D
from deepspeech_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BFT = torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------ the oracle
def test_known_answer_and_threshold():
    ctr, key, want = DC.KNOWN
    assert R.philox4x32(ctr, key) == want
    assert [R.seq_dropout_threshold(p) for p in (0.0, 0.1, 0.2, 0.25, 0.5, 0.999999)] == [0, 6554, 13107, 16384, 32768,
                                                                                        65535]
    assert R.seq_dropout_scale(32768) == 2.0 and R.seq_dropout_scale(65535) == 65536.0
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            R.seq_dropout_threshold(p)


@pytest.mark.parametrize("locked", [False, True], ids=["element", "locked"])
def test_oracle_is_the_definition(locked):
    T, N, H = 5, 2, 40
    step, fu, site, thr = 2 ** 31 + 5, 0xffffffff, 9, 32768            # first_utt + 1 wraps to 0
    m = R.seq_dropout_mask_ref(T, N, H, DC.SEED, step, fu, site, thr, locked)
    assert m.dtype == torch.bool and tuple(m.shape) == (T, N, H)
    want = [[[DC.scalar_keep(t, b, i, DC.SEED, step, fu, site, thr, locked) for i in range(H)] for b in range(N)]
            for t in range(T)]
    assert torch.equal(m, torch.tensor(want))
    # a seed above 32 bits reaches the second key word
    big = (7 << 32) | 5
    m2 = R.seq_dropout_mask_ref(2, 1, 8, big, 1, 0, 0, thr, locked)
    assert m2.tolist() == [[[DC.scalar_keep(t, 0, i, big, 1, 0, 0, thr, locked) for i in range(8)]] for t in range(2)]
    # any H: a last partial group uses its first slots
    assert torch.equal(R.seq_dropout_mask_ref(T, N, 12, DC.SEED, step, fu, site, thr, locked), m[:, :, :12])


def test_batch_step_site_and_mode():
    a = dict(seed=DC.SEED, step=7, site=2, thr=13107)
    full = R.seq_dropout_mask_ref(6, 4, 40, first_utt=0, locked=False, **a)
    assert torch.equal(R.seq_dropout_mask_ref(6, 2, 40, first_utt=2, locked=False, **a), full[:, 2:4])
    assert not torch.equal(R.seq_dropout_mask_ref(6, 4, 40, first_utt=0, locked=False, **dict(a, step=8)), full)
    assert not torch.equal(R.seq_dropout_mask_ref(6, 4, 40, first_utt=0, locked=False, **dict(a, site=3)), full)
    assert not torch.equal(R.seq_dropout_mask_ref(6, 4, 40, first_utt=0, locked=False, **dict(a, seed=1235)), full)
    lock = R.seq_dropout_mask_ref(6, 4, 40, first_utt=0, locked=True, **a)
    assert bool((lock == lock[0:1]).all()) and not torch.equal(lock, full)
    assert not bool((full == full[0:1]).all())
    assert torch.equal(R.seq_dropout_mask_ref(6, 2, 40, first_utt=2, locked=True, **a), lock[:, 2:4])


@pytest.mark.parametrize("shape,thr,want", DC.COUNTS, ids=[DC.ident(c[0] + (c[1],)) for c in DC.COUNTS])
def test_dropped_counts(shape, thr, want):
    m = R.seq_dropout_mask_ref(*shape, DC.SEED, 7, 0, 2, thr, False)
    n, p = m.numel(), thr / 65536
    dropped = n - int(m.sum())
    print("DROPCOUNT %s thr %d dropped %d of %d, %.2f sigma" % (shape, thr, dropped, n,
                                                              abs(dropped - n * p) / math.sqrt(n * p * (1 - p))))
    assert abs(dropped - n * p) <= 4 * math.sqrt(n * p * (1 - p))
    assert dropped == want                       # the recorded oracle value: the streams do not move


# ------------------------------------------------------------------------------ the composite and the op
def _state(step=7, first_utt=0, dev="cpu"):
    st = D.DropoutState(dev)
    st.set(step, first_utt)
    return st


def test_state_words():
    st = _state(2 ** 32 + 2 ** 31 + 5, 0xfffffffe)
    assert st.ctr.dtype == torch.int32 and st.ctr.tolist() == [2 ** 31 + 5 - 2 ** 32, -2]
    assert st.get() == (2 ** 31 + 5, 0xfffffffe)


@pytest.mark.parametrize("dtype", [F32, BFT], ids=["fp32", "bf16"])
def test_thr_edges_and_values(dtype):
    x = DC.inputs((5, 2, 40), 1, dtype)
    st = _state()
    assert D.seq_dropout(x, st, DC.SEED, 2, 0) is x
    assert R.seq_dropout_ref(x, DC.SEED, 7, 0, 2, 0, False) is x
    y = D.seq_dropout(x, st, DC.SEED, 2, 65535)
    assert y.dtype == dtype and bool(torch.isfinite(y).all())
    assert int((y != 0).sum()) <= 1 + int(x.numel() * 8 / 65536)
    for mode in D.MODES:
        y = D.seq_dropout(x, st, DC.SEED, 2, 16384, mode)
        keep = R.seq_dropout_mask_ref(5, 2, 40, DC.SEED, 7, 0, 2, 16384, mode == "locked")
        scale = R.seq_dropout_scale(16384)
        want = torch.where(keep, (x.float() * scale).to(dtype), torch.zeros((), dtype=dtype))
        assert DC.same_bits(y, want)
        assert not bool(torch.signbit(y[~keep]).any())          # +0, not -0
    with pytest.raises(ValueError):
        D.seq_dropout(x, st, DC.SEED, 16384, 5)
    with pytest.raises(ValueError):
        D.seq_dropout(x, st, DC.SEED, 0, 5, "frame")


@pytest.mark.parametrize("dtype", [F32, BFT], ids=["fp32", "bf16"])
def test_gradient_is_the_same_map(dtype):
    thr, site = 32768, 4
    x = DC.inputs((5, 2, 40), 2, dtype).requires_grad_(True)
    dy = DC.inputs((5, 2, 40), 3, dtype)
    keep = R.seq_dropout_mask_ref(5, 2, 40, DC.SEED, 7, 0, site, thr, False)
    dropped = (~keep).nonzero()
    dy[tuple(dropped[0])] = float("inf")
    dy[tuple(dropped[1])] = float("nan")
    kept = keep.nonzero()
    dy[tuple(kept[0])] = float("inf")
    st = _state()
    y = D.seq_dropout(x, st, DC.SEED, site, thr)
    before = dy.clone()
    y.backward(dy)
    assert DC.same_bits(dy, before)                 # a caller's gradient is not rewritten
    want = torch.where(keep, (dy.float() * R.seq_dropout_scale(thr)).to(dtype), torch.zeros((), dtype=dtype))
    assert DC.same_bits(x.grad, want)
    assert float(x.grad[tuple(dropped[0])]) == 0 and float(x.grad[tuple(dropped[1])]) == 0
    assert math.isinf(float(x.grad[tuple(kept[0])]))
    # forward: inf / NaN under a dropped element do not survive, a kept one passes through
    xi = x.detach().clone()
    xi[tuple(dropped[0])], xi[tuple(dropped[1])], xi[tuple(kept[0])] = float("inf"), float("nan"), float("-inf")
    yi = D.seq_dropout(xi, st, DC.SEED, site, thr)
    assert float(yi[tuple(dropped[0])]) == 0 and float(yi[tuple(dropped[1])]) == 0
    assert float(yi[tuple(kept[0])]) == float("-inf")
    assert int((~torch.isfinite(yi)).sum()) == 1
    # the composite's own autograd agrees (the ref engine differentiates it)
    x2 = x.detach().clone().requires_grad_(True)
    R.seq_dropout_ref(x2, DC.SEED, 7, 0, site, thr, False).backward(before)
    assert DC.same_bits(x2.grad, want)
    # a later step's backward takes the later step's mask, nothing re-created
    x3 = x.detach().clone().requires_grad_(True)
    st.set(8, 0)
    D.seq_dropout(x3, st, DC.SEED, site, thr).backward(torch.ones_like(x3))
    assert torch.equal(x3.grad != 0, R.seq_dropout_mask_ref(5, 2, 40, DC.SEED, 8, 0, site, thr, False))


# ------------------------------------------------------------------------------ the model, ref engine
KW = dict(num_filters=4, num_hidden=16, num_rnn_layers=3, cell="gru")


def _feats(n=3, frames=90):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, frames, 161, generator=g), torch.tensor([frames, frames - 17, frames - 30][:n])


def _tapped(model):
    """Record (input, output) of every recurrent layer's forward_ref / forward_ref_split call."""
    taps = []
    for layer in model.rnn:
        for name in ("forward_ref", "forward_ref_split"):
            def wrap(*a, _f=getattr(layer, name)):
                out = _f(*a)
                taps.append((a[:-1], out))
                return out
            setattr(layer, name, wrap)
    return taps


@pytest.mark.parametrize("bidir", [True, False], ids=["bidir", "uni"])
@pytest.mark.parametrize("mode", ["element", "locked"])
def test_model_wiring_ref_engine(bidir, mode):
    torch.manual_seed(3)
    plain = DeepSpeech2(bidirectional=bidir, **KW)
    drop = DeepSpeech2(bidirectional=bidir, rnn_dropout=0.25, rnn_dropout_mode=mode, **KW)
    drop.load_state_dict(plain.state_dict())
    drop.rnn_dropout_seed = DC.SEED
    assert plain.dropout_state is None and drop.rnn_dropout_thr == 16384
    feats, lens = _feats()
    plain.eval(), drop.eval()
    with torch.no_grad():
        assert torch.equal(drop(feats, lens)[0], plain(feats, lens)[0])
    drop.train()
    drop.dropout_state.set(11, 4)
    taps = _tapped(drop)
    drop.capture = True
    with torch.no_grad():
        logits, _ = drop(feats, lens)
    assert len(taps) == 3
    for i in range(2):
        want = R.seq_dropout_ref(taps[i][1], DC.SEED, 11, 4, 2 * i, 16384, mode == "locked")
        assert torch.equal(taps[i + 1][0][0], want), i
        assert not torch.equal(want, taps[i][1])
    assert torch.equal(drop.act_taps["rnn"], taps[2][1])            # the top output is untouched
    plain.train()
    with torch.no_grad():
        assert not torch.equal(logits, plain(feats, lens)[0])


def test_model_wiring_direction_stacks():
    torch.manual_seed(4)
    drop = DeepSpeech2(layout="nhwc", rnn_dropout=0.5, **KW)
    drop.rnn_dropout_seed = DC.SEED
    drop.train()
    drop.dropout_state.set(3, 0)
    taps = _tapped(drop)
    drop.capture = True
    feats, lens = _feats()
    with torch.no_grad():
        drop(feats, lens)
    for i in range(2):
        for d in range(2):
            want = R.seq_dropout_ref(taps[i][1][d], DC.SEED, 3, 0, 2 * i + d, 32768, False)
            assert torch.equal(taps[i + 1][0][d], want), (i, d)
    assert torch.equal(drop.act_taps["rnn"], taps[2][1][0] + taps[2][1][1])


def test_model_edges():
    with pytest.raises(ValueError):
        DeepSpeech2(stack_fix=False, rnn_dropout=0.1, **KW)
    with pytest.raises(ValueError):
        DeepSpeech2(rnn_dropout=1.0, **KW)
    with pytest.raises(ValueError):
        DeepSpeech2(rnn_dropout=0.1, rnn_dropout_mode="frame", **KW)
    DeepSpeech2(stack_fix=False, **KW)
    torch.manual_seed(6)
    kw = dict(KW, num_rnn_layers=1)
    plain, one = DeepSpeech2(**kw), DeepSpeech2(rnn_dropout=0.5, **kw)
    one.load_state_dict(plain.state_dict())
    feats, lens = _feats()
    plain.train(), one.train()
    with torch.no_grad():
        assert torch.equal(one(feats, lens)[0], plain(feats, lens)[0])
    assert list(one.state_dict()) == list(plain.state_dict())


def test_trainer_sets_the_state():
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.trainer import LRSchedule, Trainer
    torch.manual_seed(7)
    m = DeepSpeech2(rnn_dropout=0.25, **dict(KW, num_rnn_layers=2))
    tr = Trainer(m, LRSchedule(1e-3, 100, 0.9))
    assert tr.first_utt == 0
    tr.first_utt = 6
    batch = to_device(FixedShapeBatches(2, max_frames=120, seed=1, pool=1).next(), torch.device("cpu"))
    for step in range(2):
        assert math.isfinite(float(tr.step(batch)))
        assert m.dropout_state.get() == (step, 6)
    plain = Trainer(DeepSpeech2(**dict(KW, num_rnn_layers=2)), LRSchedule(1e-3, 100, 0.9))
    assert plain.model.dropout_state is None and math.isfinite(float(plain.step(batch)))


# ------------------------------------------------------------------------------ the driver
def test_flags_are_training_hyper_parameters():
    from deepspeech_amd import config as C
    a = C.parse_train_args([])
    assert a.rnn_dropout == 0.0 and a.rnn_dropout_mode == "element" and a.keep_prob == 0.5
    a = C.parse_train_args(["--rnn_dropout", "0.1", "--rnn_dropout_mode", "locked"])
    assert a.rnn_dropout == 0.1 and a.rnn_dropout_mode == "locked"
    with pytest.raises(SystemExit):
        C.parse_train_args(["--rnn_dropout_mode", "frame"])
    for k in ("rnn_dropout", "rnn_dropout_mode"):
        assert k not in C.RESUME_KEYS and k not in C.EVAL_KEYS
        assert not hasattr(C.build_eval_parser().parse_args([]), k)
        assert k not in C.model_kwargs_from_args(a)
    # --keep_prob stays parsed and switches nothing on (quirk Q8)
    assert DeepSpeech2(**KW).rnn_dropout_thr == 0
    helps = {act.dest: act.help for act in C.build_train_parser()._actions}
    assert "unused" in helps["keep_prob"] and "--rnn_dropout" in helps["keep_prob"]


def _train_cmd(d, steps, extra):
    return [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--batch_size", "2", "--num_hidden", "16",
            "--num_rnn_layers", "2", "--num_filters", "4", "--cell", "gru", "--device", "cpu", "--max_steps",
            str(steps), "--train_dir", d, "--log_every", "1000", "--checkpoint_every", "1", "--async_checkpoint",
            "False"] + extra


def _last_loss(d, step):
    recs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    recs = [r for r in recs if r.get("step") == step and "loss" in r]
    assert recs, "no loss record of step %d" % step
    return recs[-1]["loss"]


def test_train_driver_flag(tmp_path):
    """deepspeech_amd.train --dummy True on the CPU (ref engine), 2 x GRU-16, 3 steps, the loss of
    step 2 compared: --rnn_dropout 0 and --keep_prob are bitwise the run without a flag, a
    probability changes it, and a run resumed from the step-1 checkpoint reproduces the
    uninterrupted run's step 2 bitwise (same masks at the same global step)."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    on = ["--rnn_dropout", "0.25"]
    runs = {"plain": (3, []), "off": (3, ["--rnn_dropout", "0", "--keep_prob", "0.9"]), "drop": (3, on),
            "locked": (3, on + ["--rnn_dropout_mode", "locked"]), "head": (2, on)}
    procs = {k: subprocess.Popen(_train_cmd(str(tmp_path / k), n, extra), env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for k, (n, extra) in runs.items()}
    outs = {}
    for k, p in procs.items():
        outs[k] = p.communicate(timeout=600)[0]
        assert p.returncode == 0, outs[k][-3000:]
    loss = {k: _last_loss(str(tmp_path / k), runs[k][0] - 1) for k in runs}
    assert loss["off"] == loss["plain"]
    assert math.isfinite(loss["drop"]) and loss["drop"] != loss["plain"]
    assert math.isfinite(loss["locked"]) and loss["locked"] not in (loss["plain"], loss["drop"])
    assert "rnn_dropout:  p=0.25 (16384/65536), element" in outs["drop"]
    assert "rnn_dropout" not in outs["plain"] and "rnn_dropout" not in outs["off"]
    d = str(tmp_path / "head")
    r = subprocess.run(_train_cmd(d, 3, on + ["--checkpoint", d]), env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "has checkpoint" in r.stdout
    assert _last_loss(d, 2) == loss["drop"]


# ------------------------------------------------------------------------------ the kernel's registers
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
def test_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    rows = KR.analyse(os.path.join(ROOT, "deepspeech_amd", "csrc", "dropout.hip"))
    assert rows, "no kernels found"
    for r in rows:
        assert not r.get("VGPRs Spill", 0) and not r.get("ScratchSize [bytes/lane]", 0), r
