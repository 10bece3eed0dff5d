"""Gradient-norm clipping, CPU side: the definition (ops/reference.py clip_from_sumsq /
clip_coef_ref / clipped_adam_ref) against an fp64 oracle, the CPU branch of FusedAdamEMA, the ref
engine Trainer, the command line and a 2-rank gloo run.

Definition: x_i = fl32(g_i gscale), S = sum x_i^2, norm = fl32(sqrt(S)); coef = 1.0f (selected) if
norm <= C else fl32(C / norm); a non-finite norm makes the step bad: coef 0 and nothing updated.

Bounds. The composite sums S in fp32 in torch's order: n products and at most n additions, each
correctly rounded, so |S32 - S| <= (n + 1) u S with u = 2^-24 (all terms >= 0), the norm inherits
half of that relative error plus the rounding of the square root, and the coefficient that plus
the quotient's rounding: (n / 2 + 3) u relative for both."""
import json
import math
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from deepspeech_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


def _f32(x):
    return float(torch.tensor(x, dtype=F32))


def _grad(n, seed=0, scale=1.0):
    return scale * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=F32)


# ------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("n,gscale,C", [(1, 1.0, 0.5), (1000, 0.5, 3.0), (4097, _f32(1 / 3), 400.0), (4097, 1.0, 7.0)])
def test_coef_against_the_fp64_oracle(n, gscale, C):
    g = _grad(n, n)
    S, norm, coef, bad = R.clip_coef_ref(g, gscale, C)
    S64, norm64, coef64, bad64 = R.clip_coef_ref(g, gscale, C, oracle=True)
    # the oracle itself against plain fp64 arithmetic
    x = (g * torch.tensor(gscale, dtype=F32)).to(F64)
    want = float((x * x).sum())
    assert abs(S64 - want) <= U * want
    assert abs(norm64 - math.sqrt(want)) <= 2 * U * math.sqrt(want)
    assert not bad and not bad64
    tol = (n / 2 + 3) * U
    assert abs(S - want) <= (n + 1) * U * want
    assert abs(norm - math.sqrt(want)) <= tol * math.sqrt(want)
    if math.sqrt(want) * (1 + tol) < C:
        assert coef == 1.0 and coef64 == 1.0
    elif math.sqrt(want) * (1 - tol) > C:
        assert abs(coef - C / math.sqrt(want)) <= tol * C / math.sqrt(want)
        assert abs(coef64 - C / math.sqrt(want)) <= 3 * U * C / math.sqrt(want)
        assert coef < 1.0
    # the clipped gradient's norm is C (to the rounding of its n products)
    if coef < 1.0:
        y = (x.to(F32) * torch.tensor(coef, dtype=F32)).to(F64)
        assert abs(math.sqrt(float((y * y).sum())) - C) <= (tol + 2 * U) * C


def test_norm_equal_to_the_threshold_is_not_clipped():
    # S = 25 exactly: norm == C == 5 selects 1.0f; the next fp32 above C clips, the one below does not
    assert R.clip_from_sumsq(25.0, 5.0) == (5.0, 1.0, False)
    g = torch.tensor([3.0, 4.0], dtype=F32)
    assert R.clip_coef_ref(g, 1.0, 5.0) == (25.0, 5.0, 1.0, False)
    below = float(torch.nextafter(torch.tensor(5.0, dtype=F32), torch.tensor(0.0, dtype=F32)))
    norm, coef, bad = R.clip_from_sumsq(25.0, below)
    assert norm == 5.0 and not bad and coef == float(torch.tensor(below, dtype=F32) / torch.tensor(5.0, dtype=F32)) < 1.0
    above = float(torch.nextafter(torch.tensor(5.0, dtype=F32), torch.tensor(9.0, dtype=F32)))
    assert R.clip_from_sumsq(25.0, above) == (5.0, 1.0, False)


def test_zero_gradient_has_coef_one():
    assert R.clip_coef_ref(torch.zeros(37), 1.0, 1e-30) == (0.0, 0.0, 1.0, False)
    assert R.clip_coef_ref(torch.zeros(0), 1.0, 1.0) == (0.0, 0.0, 1.0, False)
    assert R.clip_from_sumsq(0.0, 400.0) == (0.0, 1.0, False)


def test_infinite_threshold_never_clips():
    for scale in (1e-3, 1.0, 1e15):
        S, norm, coef, bad = R.clip_coef_ref(_grad(100, 3, scale), 1.0, float("inf"))
        assert coef == 1.0 and not bad and norm > 0
    # ... but still refuses a non-finite norm
    assert R.clip_coef_ref(torch.tensor([float("inf")]), 1.0, float("inf"))[2:] == (0.0, True)
    for C in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            R.clip_from_sumsq(1.0, C)


def test_clipped_adam_composite_against_its_oracle():
    n = 515
    gen = torch.Generator().manual_seed(5)
    p, m, e = torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    v, g = 0.01 * torch.rand(n, generator=gen), torch.randn(n, generator=gen)
    hy = dict(lr_t=_f32(1e-3), b1=_f32(0.9), b2=_f32(0.999), eps=_f32(1e-8), gscale=0.5, coef=_f32(0.3), keep=_f32(0.99))
    want = R.clipped_adam_ref(p, g, m, v, e, None, oracle=True, **hy)
    got = [t.clone() for t in (p, m, v, e)]
    p16 = torch.zeros(n, dtype=torch.bfloat16)
    assert R.clipped_adam_ref(got[0], g, got[1], got[2], got[3], p16, **hy) is None
    for k, t in zip(("p", "m", "v", "ema"), got):
        # a handful of fp32 roundings per element, on magnitudes <= 4
        assert float((t.to(F64) - want[k]).abs().max()) <= 64 * U, k
    assert torch.equal(p16, got[0].to(torch.bfloat16))
    # m from zero is (1 - b1) (g gscale) coef op by op; coef = 1 and coef = None are the same bits
    m0 = torch.zeros(n)
    R.clipped_adam_ref(p.clone(), g, m0, v.clone(), None, None, **hy)
    gj = (g * 0.5) * torch.tensor(hy["coef"])
    assert torch.equal(m0, torch.zeros(n).mul_(hy["b1"]).add_(gj, alpha=1 - hy["b1"]))
    a, b = [t.clone() for t in (p, m, v, e)], [t.clone() for t in (p, m, v, e)]
    R.clipped_adam_ref(a[0], g, a[1], a[2], a[3], None, **dict(hy, coef=1.0))
    R.clipped_adam_ref(b[0], g, b[1], b[2], b[3], None, **dict(hy, coef=None))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------ FusedAdamEMA on the CPU
def _opt(n=300, **kw):
    from deepspeech_amd.ops.optim import FusedAdamEMA, ParamArena
    torch.manual_seed(1)
    lin = torch.nn.Linear(n // 10, 10, bias=False)
    arena = ParamArena(lin)
    return FusedAdamEMA(arena, lr=1e-2, ema_decay=0.99, bf16_copy=True, **kw)


def _arrays(o):
    return [o.arena.flat, o.m, o.v, o.ema, o.p16]


def test_optimizer_clips_to_the_threshold_and_counts():
    o, plain = _opt(max_grad_norm=0.5), _opt()
    assert o.clip and not plain.clip and plain.clip_state is None
    g = _grad(o.arena.numel, 2)
    for x in (o, plain):
        x.arena.grad.copy_(g)
    o.step(1e-2, 0)
    st = o.clip_stats()
    S, norm, coef, bad = R.clip_coef_ref(g, 1.0, 0.5)
    assert (st["sumsq"], st["grad_norm"], st["clip_coef"], st["bad"]) == (S, norm, coef, 0) and coef < 1
    assert (st["steps"], st["clipped_steps"], st["skipped_steps"]) == (1, 1, 0)
    # the same as an unclipped step on the gradient scaled by coef
    plain.arena.grad.mul_(torch.tensor(coef, dtype=F32))
    plain.step(1e-2, 0)
    for a, b in zip(_arrays(o), _arrays(plain)):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError):
        plain.measure_norm()
    with pytest.raises(RuntimeError):
        plain.clip_stats()
    for bad_c in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            _opt(max_grad_norm=bad_c)


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf"), 1e20])
@pytest.mark.parametrize("C", [1.0, float("inf")])
def test_bad_step_leaves_every_array_bitwise_unchanged(poison, C):
    o = _opt(max_grad_norm=C)
    o.arena.grad.copy_(_grad(o.arena.numel, 4))
    o.step(1e-2, 0)                                   # moments and EMA away from their start
    o.arena.grad[o.arena.numel // 2] = poison
    snap = [t.clone().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) for t in _arrays(o)]
    o.step(1e-2, 1)
    st = o.clip_stats()
    assert st["bad"] == 1 and st["clip_coef"] == 0.0 and not math.isfinite(st["grad_norm"])
    assert (st["steps"], st["skipped_steps"]) == (2, 1)
    assert int(o.clip_bad_flag()) == 1
    for a, s in zip(_arrays(o), snap):
        assert torch.equal(a.view(s.dtype), s)
    o.arena.grad[o.arena.numel // 2] = 0.0           # the next good step updates again
    o.step(1e-2, 2)
    assert o.clip_stats()["bad"] == 0 and not torch.equal(_arrays(o)[0].view(torch.int32), snap[0])


# ------------------------------------------------------------------------------ Trainer, ref engine
def _trainer(**kw):
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.trainer import LRSchedule, Trainer
    torch.manual_seed(0)
    m = DeepSpeech2(num_filters=4, num_hidden=16, num_rnn_layers=2, cell="gru")
    return Trainer(m, LRSchedule(1e-2, 3, 0.5), moving_avg_decay=0.99, **kw)


def _batches(n, seed=10):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    return [to_device(FixedShapeBatches(2, max_frames=140, seed=seed + i, pool=1).next(), torch.device("cpu")) for i in range(n)]


def _tstate(tr):
    return [tr.arena.flat, tr.arena.grad, tr.opt.m, tr.opt.v, tr.opt.ema]


def test_trainer_with_a_huge_threshold_is_bitwise_the_plain_trainer():
    plain, big = _trainer(), _trainer(max_grad_norm=1e30)
    for b in _batches(5):
        assert float(plain.step(b)) == float(big.step(b))
    for x, y in zip(_tstate(plain), _tstate(big)):
        assert torch.equal(x, y)
    st = big.opt.clip_stats()
    assert (st["steps"], st["clipped_steps"], st["skipped_steps"], st["clip_coef"]) == (5, 0, 0, 1.0)
    assert st["grad_norm"] > 0


def test_trainer_clips_and_skip_policy_shares_the_flag():
    probe = _trainer(max_grad_norm=float("inf"))
    bs = _batches(3)
    probe.step(bs[0])
    n0 = probe.opt.clip_stats()["grad_norm"]
    tr, plain = _trainer(max_grad_norm=n0 / 2, nan_policy="skip"), _trainer()
    for b in bs:
        tr.step(b)
        plain.step(b)
    st = tr.opt.clip_stats()
    assert st["clipped_steps"] == 3 and st["skipped_steps"] == 0 and 0 < st["clip_coef"] < 1
    assert tr.last_skip.data_ptr() == tr.opt.clip_bad_flag().data_ptr() and int(tr.last_skip) == 0
    assert not torch.equal(tr.arena.flat, plain.arena.flat)


def test_cli_flag_is_a_training_hyper_parameter(tmp_path):
    from deepspeech_amd import config as C
    a = C.parse_train_args([])
    assert a.max_grad_norm == 0.0
    a = C.parse_train_args(["--max_grad_norm", "400"])
    assert a.max_grad_norm == 400.0
    assert C.parse_train_args(["--max_grad_norm", "inf"]).max_grad_norm == float("inf")
    assert "max_grad_norm" not in C.RESUME_KEYS and "max_grad_norm" not in C.EVAL_KEYS
    # a checkpoint directory written with the flag does not hand it to a resumed run or to evaluation
    C.dump_param_json(a, str(tmp_path))
    assert json.load(open(os.path.join(str(tmp_path), "deepSpeech_parameters.json")))["max_grad_norm"] == 400.0
    r = C.parse_train_args(["--checkpoint", str(tmp_path)])
    assert r.max_grad_norm == 0.0
    r = C.parse_train_args(["--checkpoint", str(tmp_path), "--max_grad_norm", "5"])
    assert r.max_grad_norm == 5.0
    e = C.parse_eval_args(["--checkpoint_dir", str(tmp_path)])
    assert not hasattr(e, "max_grad_norm")


def test_train_driver_logs_the_norm_only_with_the_flag(tmp_path):
    """deepspeech_amd.train --dummy True on the CPU (ref engine), 2 x GRU-16, 12 steps: with
    --max_grad_norm the metrics and the log carry grad_norm, clip_coef and the counters; with a
    huge threshold the losses are those of the run without the flag, whose records have no such keys."""
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")

    def cmd(d, extra):
        return [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--batch_size", "2", "--num_hidden", "16",
                "--num_rnn_layers", "2", "--num_filters", "4", "--cell", "gru", "--device", "cpu", "--max_steps", "12",
                "--train_dir", d, "--log_every", "11", "--summary_every", "1", "--summaries_on_dummy", "True",
                "--activation_summaries", "False", "--checkpoint_every", "0"] + extra
    runs = {"plain": [], "huge": ["--max_grad_norm", "1e30"], "clip": ["--max_grad_norm", "1e-3"]}
    procs = {k: subprocess.Popen(cmd(str(tmp_path / k), extra), env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for k, extra in runs.items()}
    outs, recs = {}, {}
    for k, p in procs.items():
        outs[k] = p.communicate(timeout=600)[0]
        assert p.returncode == 0, outs[k][-3000:]
        recs[k] = [r for r in map(json.loads, open(os.path.join(str(tmp_path / k), "metrics.jsonl"))) if "loss" in r]
        assert [r["step"] for r in recs[k]] == list(range(12))
    keys = ("grad_norm", "clip_coef", "clipped_steps", "skipped_steps")
    assert not any(k in r for r in recs["plain"] for k in keys) and "max_grad_norm" not in outs["plain"]
    assert [r["loss"] for r in recs["huge"]] == [r["loss"] for r in recs["plain"]]
    assert [(r["clip_coef"], r["clipped_steps"], r["skipped_steps"]) for r in recs["huge"]] == [(1.0, 0, 0)] * 12
    assert [r["clipped_steps"] for r in recs["clip"]] == list(range(1, 13))
    assert all(0 < r["clip_coef"] < 1 and r["grad_norm"] > 1e-3 for r in recs["clip"])
    assert "max_grad_norm: 0.001" in outs["clip"] and "grad_norm = " in outs["clip"]
    assert "grad_norm = " not in outs["plain"]
    assert recs["clip"][11]["loss"] != recs["plain"][11]["loss"]


# ------------------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, C, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    from deepspeech_amd.parallel.dist import init_distributed, shutdown
    ctx = init_distributed("cpu")
    tr = _trainer(world_size=world, bucket_mb=0.001, max_grad_norm=C)
    assert len(tr.bucketer.buckets) >= 3
    coefs = []
    for b in _batches(2 * world)[rank::world]:
        tr.step(b)
        coefs.append(tr.opt.clip_stats())
    torch.save({"w": tr.arena.flat.clone(), "ema": tr.opt.ema.clone(), "stats": coefs}, "%s.%d" % (out, rank))
    shutdown(ctx)


def test_dp2_ranks_derive_the_same_coefficient(tmp_path):
    """Both ranks hold the bitwise equal reduced gradient, so each derives the same coefficient from
    it (the norm of the mean gradient: gscale = 1 / world is inside x_i) and they end with equal
    weights; every step clips at this threshold."""
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(2, _free_port(), 1e-3, out), nprocs=2, join=True)
    a, b = (torch.load("%s.%d" % (out, r), weights_only=True) for r in range(2))
    assert a["stats"] == b["stats"]
    assert [s["clipped_steps"] for s in a["stats"]] == [1, 2]
    assert all(0 < s["clip_coef"] < 1 and s["grad_norm"] > 1e-3 for s in a["stats"])
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["ema"], b["ema"])
