"""SpecAugment on the CPU: the generator, the plan oracle, the CPU path of ops/specaug.py, the
policy parser and the training driver's --specaug flag."""
import json
import math
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import specaug_cases as SC
from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops.specaug import SpecAugment, SpecAugPolicy, kernels_cover, specaug_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % v for v in R.philox4x32(ctr, key)) == want
    # the vectorised form the plan oracle uses gives the same words
    got = R.philox4x32(tuple(np.array([c, 0], np.uint64) for c in kat[2][0]),
                       tuple(np.array([k, 0], np.uint64) for k in kat[2][1]))
    assert " ".join("%08x" % int(v[0]) for v in got) == kat[2][2]
    assert " ".join("%08x" % int(v[1]) for v in got) == kat[0][2]


def test_grid_preconditions_and_plan_invariants():
    """Every mask inside [0, F] / [0, L], d0 in [1, L-2] (asserted inside), and the grid reaches
    every branch: masks at both edges, zero widths, overlaps, a time mask ending at L-1, warps
    of either sign and zero, forced identities, a p-cut cap."""
    seen = SC.preconditions()
    assert all(v > 0 for v in seen.values()), seen
    assert len(SC.CASES) == 60


def test_draw_statistics():
    """Over N = 20000 utterances the mean of a uniform integer draw on [0, n] lies within
    5 sigma / sqrt(N) of n / 2, sigma^2 = ((n + 1)^2 - 1) / 12: fw (n = Fw), w + W (n = 2W) and
    t0 with zero-width masks (n = L)."""
    N, L, F, Fw, W = 20000, 700, 161, 27, 40
    pol = SimpleNamespace(nF=1, Fw=Fw, nT=1, Tw=0, p_ppm=1000000, W=W)
    plan = R.specaug_plan_ref(torch.full((N,), L, dtype=torch.int32), L, F, pol, 99, 3).double()

    def check(col, n, shift=0.0):
        sigma = math.sqrt(((n + 1) ** 2 - 1) / 12.0)
        assert abs(float(col.mean()) + shift - n / 2.0) <= 5 * sigma / math.sqrt(N), (float(col.mean()), n)

    check(plan[:, 3], Fw)
    check(plan[:, 1], 2 * W, shift=W)
    check(plan[:, 4], L)
    n0 = L - 2 * W - 2
    check(plan[:, 0] - (W + 1), n0 - 1)
    assert plan[:, 3].min() == 0 and plan[:, 3].max() == Fw and plan[:, 1].min() == -W and plan[:, 1].max() == W


def test_plan_is_pure():
    """Utterance u's plan is the same alone, in a batch of 33, or split over two "ranks"."""
    pol = SpecAugPolicy.parse("W=5,F=27,nF=2,T=30,nT=2,p=0.5")
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(0, 140, (33,), generator=g, dtype=torch.int32)
    whole = specaug_plan(lens, 130, 161, pol, 1234, 7, first_utt=0)
    for u in (0, 16, 32):
        assert torch.equal(specaug_plan(lens[u:u + 1], 130, 161, pol, 1234, 7, first_utt=u), whole[u:u + 1])
    halves = [specaug_plan(lens[:16], 130, 161, pol, 1234, 7, first_utt=0),
              specaug_plan(lens[16:], 130, 161, pol, 1234, 7, first_utt=16)]
    assert torch.equal(torch.cat(halves), whole)


def test_plan_depends_on_seed_and_step_and_their_high_words():
    pol = SpecAugPolicy.parse("ld")
    lens = torch.full((8,), 400, dtype=torch.int32)
    base = specaug_plan(lens, 400, 161, pol, 1234, 5)
    assert torch.equal(base, specaug_plan(lens, 400, 161, pol, 1234, 5))
    for seed, step in ((1235, 5), (1234 + 2 ** 32, 5), (1234, 6), (1234, 5 + 2 ** 32)):
        assert not torch.equal(base, specaug_plan(lens, 400, 161, pol, seed, step)), (seed, step)


@pytest.mark.parametrize("idx", range(0, 60, 3))
def test_cpu_path_equals_oracle(idx):
    c = SC.CASES[idx]
    x, lens = SC.inputs(idx)
    aug = SpecAugment(SpecAugPolicy(nF=c.nF, Fw=c.Fw, nT=c.nT, Tw=c.Tw, p_ppm=c.p_ppm, W=c.W, fill=c.fill), c.seed)
    assert not kernels_cover(x)
    keep = x.clone()
    out, plan = aug(x, lens, c.step, first_utt=c.first_utt, return_plan=True)
    if aug.policy.empty:
        assert out is x and plan is None
        return
    assert torch.equal(x, keep) and out is not x
    assert torch.equal(plan, SC.oracle_plan(idx))
    fill = R.specaug_mean_ref(x, lens) if c.fill == "mean" else None
    if fill is not None:
        SC.check_mean(fill, x, lens)
    SC.check_apply(out, x, lens, plan, fill, c.nF)
    L = lens.long().clamp(0, c.T)
    pad = torch.arange(c.T)[None, :] >= L[:, None]
    assert torch.equal(SC.bits(out)[pad], SC.bits(x)[pad])
    if c.W == 0:
        y = x.clone()
        assert aug(y, lens, c.step, first_utt=c.first_utt, inplace=True) is y
        assert torch.equal(SC.bits(y), SC.bits(out))


def test_nan_under_a_mask_becomes_the_fill():
    pol = SpecAugPolicy(nF=1, Fw=8, nT=1, Tw=20, fill="zero")
    lens = torch.tensor([40, 25, 0], dtype=torch.int32)
    x = torch.randn(3, 40, 16, generator=torch.Generator().manual_seed(2))
    plan = specaug_plan(lens, 40, 16, pol, 7, 0)
    tm, fm = R.specaug_masks(lens, plan, 40, 16, 1)
    masked = tm[:, :, None] | (fm[:, None, :] & (torch.arange(40)[None, :] < lens[:, None])[:, :, None])
    assert masked.any() and not masked[2].any()
    x[masked] = float("nan")
    out = SpecAugment(pol, 7)(x, lens, 0)
    assert not torch.isnan(out).any()
    assert bool((out[masked] == 0).all()) and torch.equal(out[~masked], x[~masked])


def test_empty_policy_and_inplace_warp():
    x = torch.randn(2, 9, 5)
    lens = torch.tensor([9, 4], dtype=torch.int32)
    assert SpecAugment(SpecAugPolicy(), 1)(x, lens, 0) is x
    assert SpecAugment(SpecAugPolicy.parse("F=3,T=4"), 1)(x, lens, 0) is x       # widths without counts
    with pytest.raises(ValueError):
        SpecAugment(SpecAugPolicy(W=2), 1)(x, lens, 0, inplace=True)


def test_policy_parser_and_presets():
    p = SpecAugPolicy.parse("F=27,nF=2,T=100,nT=2,p=0.2,W=0,fill=mean")
    assert p == SpecAugPolicy(nF=2, Fw=27, nT=2, Tw=100, p_ppm=200000, W=0, fill="mean")
    assert SpecAugPolicy.parse("ld") == SpecAugPolicy(nF=2, Fw=27, nT=2, Tw=100, p_ppm=1000000, W=80)
    assert SpecAugPolicy.parse("ls") == SpecAugPolicy(nF=2, Fw=15, nT=2, Tw=70, p_ppm=200000, W=40)
    assert SpecAugPolicy.parse(" nT=1 , T=5, fill=zero ") == SpecAugPolicy(nT=1, Tw=5, fill="zero")
    assert SpecAugPolicy.parse(str(p)) == p
    assert SpecAugPolicy.parse("").empty
    for bad in ("nF=9", "nT=17", "p=1.5", "p=-0.1", "W=-1", "F=-3", "fill=noise", "Q=1", "nF", "nF=2,nF=2", "T=x"):
        with pytest.raises(ValueError):
            SpecAugPolicy.parse(bad)


def test_flag_is_a_training_hyper_parameter():
    from deepspeech_amd import config as C
    assert C.parse_train_args([]).specaug == ""
    assert C.parse_train_args(["--specaug", "ls"]).specaug == "ls"
    assert "specaug" not in C.RESUME_KEYS and "specaug" not in C.EVAL_KEYS
    assert not hasattr(C.build_eval_parser().parse_args([]), "specaug")


# ------------------------------------------------------------------------------ the driver
SPEC = "F=27,nF=2,T=20,nT=2,p=1.0"


def _train_cmd(d, steps, extra):
    return [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--batch_size", "2", "--num_hidden", "16",
            "--num_rnn_layers", "1", "--num_filters", "4", "--device", "cpu", "--max_steps", str(steps),
            "--train_dir", d, "--log_every", "1000", "--checkpoint_every", "1", "--async_checkpoint", "False"] + extra


def _last_loss(d, step):
    recs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    recs = [r for r in recs if r.get("step") == step and "loss" in r]
    assert recs, "no loss record of step %d" % step
    return recs[-1]["loss"]


def test_train_driver_flag(tmp_path):
    """deepspeech_amd.train --dummy True on the CPU, tiny model, 3 steps; the loss of the last
    step (step 2, which depends on both steps before it) is compared: --specaug "" is bitwise the
    run without the flag, a policy changes it, and a run resumed from the step-1 checkpoint
    reproduces the uninterrupted run's step 2 bitwise (same masks at the same global step)."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    runs = {"plain": (3, []), "off": (3, ["--specaug", ""]), "aug": (3, ["--specaug", SPEC]),
            "head": (2, ["--specaug", SPEC])}
    procs = {k: subprocess.Popen(_train_cmd(str(tmp_path / k), n, extra), env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for k, (n, extra) in runs.items()}
    outs = {}
    for k, p in procs.items():
        outs[k] = p.communicate(timeout=600)[0]
        assert p.returncode == 0, outs[k][-3000:]
    loss = {k: _last_loss(str(tmp_path / k), runs[k][0] - 1) for k in runs}
    assert loss["off"] == loss["plain"]
    assert math.isfinite(loss["aug"]) and loss["aug"] != loss["plain"]
    assert "specaug:  F=27,nF=2,T=20,nT=2,p=1,W=0,fill=mean" in outs["aug"]
    assert "specaug" not in outs["plain"] and "specaug" not in outs["off"]
    d = str(tmp_path / "head")
    r = subprocess.run(_train_cmd(d, 3, ["--specaug", SPEC, "--checkpoint", d]), env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "has checkpoint" in r.stdout
    assert _last_loss(d, 2) == loss["aug"]
