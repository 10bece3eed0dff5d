"""Speed perturbation (ops/speed.py) on the CPU: the policy parser, the plan as a pure function of
(seed, step, utterance, length, guards), the reference output, the audio front end, and the train
driver's flag with a resumed dummy-audio run."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops import speed as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POL = SP.SpeedPolicy.parse("0.9,1.0,1.1")
S = 2400


def _signal(B, S, seed=0):
    return torch.randn(B, S, generator=torch.Generator().manual_seed(seed)) * 0.3


# ----------------------------------------------------------------------------------- the policy
def test_parser_and_refusals():
    assert POL.pcts == (90, 100, 110)
    assert SP.SpeedPolicy.parse(" 1.1 , 0.5,2.0 ").pcts == (110, 50, 200)
    assert SP.SpeedPolicy.parse("0.905").pcts == (90,) and SP.SpeedPolicy.parse("1.004").pcts == (100,)   # round, once
    assert SP.SpeedPolicy.parse(str(POL)) == POL
    nine = ",".join("%.2f" % (0.9 + 0.01 * i) for i in range(9))
    for bad in (nine, "0.9,0.9", "0.9,0.901", "0.49", "2.01", "0.9,,1.1", "0.9,", "", "fast"):
        with pytest.raises(ValueError):
            SP.SpeedPolicy.parse(bad)
    assert len(SP.SpeedPolicy.parse(nine[:-5]).pcts) == 8


def test_variant_tables_are_the_resampler_s():
    recs, table = POL.records, POL.table
    assert [r[:4] for r in recs] == [(90, 10, 9, 48), (100, 1, 1, 0), (110, 10, 11, 54)]
    for p, L, M, K, off in recs:
        if p != 100:
            assert off % 4 == 0
            h = R.resample_table(p, 100)[3].astype(np.float32)
            assert np.array_equal(table[off:off + L * K].numpy().reshape(L, K), h)
    assert SP.speed_out_width(S, POL) == 2720 and SP.speed_out_width(S, (110,)) == S    # N_90(2400) = 2667
    assert SP.speed_out_width(1, (100,)) == 160


# ------------------------------------------------------------------------------------- the plan
def test_plan_of_an_utterance_does_not_depend_on_the_batch():
    lens = torch.tensor([2400, 1000, 777, 2399, 160, 1], dtype=torch.int32)
    full = R.speed_plan_ref(lens, 6, S, POL, seed=5, step=9, first_utt=40)
    for b in range(6):
        alone = R.speed_plan_ref(lens[b:b + 1], 1, S, POL, 5, 9, first_utt=40 + b)
        assert torch.equal(alone[0], full[b])
        other = torch.tensor([5, 6, 7, int(lens[b]), 8], dtype=torch.int32)      # row 3 of another batch
        assert torch.equal(R.speed_plan_ref(other, 5, S, POL, 5, 9, first_utt=40 + b - 3)[3], full[b])
    split = torch.cat([R.speed_plan_ref(lens[:2], 2, S, POL, 5, 9, first_utt=40),
                       R.speed_plan_ref(lens[2:], 4, S, POL, 5, 9, first_utt=42)])
    assert torch.equal(split, full)
    assert not torch.equal(R.speed_plan_ref(lens, 6, S, POL, 5, 10, first_utt=40), full)
    big = 7 << 33                                                             # the high step word counts
    assert not torch.equal(R.speed_plan_ref(lens, 6, S, POL, 5, big + 9, first_utt=40), full)
    for b in range(6):
        pct, n_out = full[b].tolist()
        assert pct in POL.pcts and n_out == R.speed_out_len(int(lens[b]), pct)


def test_block_differs_from_the_noise_plan_s():
    seed, step, u = 11, 4, 3
    key = (seed & 0xffffffff, seed >> 32)
    noise = R.philox4x32((0, u, step, R.WAVEAUG_STREAM), key)
    speed = R.philox4x32((1, u, step, R.WAVEAUG_STREAM), key)
    assert set(noise).isdisjoint(speed)
    v = (speed[0] * 3) >> 32
    assert int(R.speed_plan_ref([S], 1, S, POL, seed, step, first_utt=u)[0, 0]) == POL.pcts[v]


def test_guards_fall_back_to_the_identity():
    B = 64
    lens = torch.full((B,), 1800, dtype=torch.int32)
    free = R.speed_plan_ref(lens, B, S, POL, 2, 0)
    fast, slow = free[:, 0] == 110, free[:, 0] == 90
    assert bool(fast.any()) and bool(slow.any())
    assert set(free[fast, 1].tolist()) == {1637} and set(free[slow, 1].tolist()) == {2000}
    floor = R.speed_plan_ref(lens, B, S, POL, 2, 0, min_out=torch.full((B,), 1638))
    assert bool((floor[fast] == torch.tensor([100, 1800])).all()) and torch.equal(floor[~fast], free[~fast])
    assert torch.equal(R.speed_plan_ref(lens, B, S, POL, 2, 0, min_out=torch.full((B,), 1637)), free)
    cap = R.speed_plan_ref(lens, B, S, POL, 2, 0, max_out=1999)
    assert bool((cap[slow] == torch.tensor([100, 1800])).all()) and torch.equal(cap[~slow], free[~slow])
    assert torch.equal(R.speed_plan_ref(lens, B, S, POL, 2, 0, max_out=2000), free)
    # the identity itself is outside the bounds: still the identity
    both = R.speed_plan_ref(lens, B, S, POL, 2, 0, min_out=torch.full((B,), 5000), max_out=10)
    assert bool((both == torch.tensor([100, 1800])).all())
    empty = R.speed_plan_ref(torch.zeros(B, dtype=torch.int32), B, S, POL, 2, 0)
    assert bool((empty == torch.tensor([100, 0])).all())
    clamped = R.speed_plan_ref(torch.tensor([-5, 99999]), 2, S, (100,), 2, 0)
    assert clamped.tolist() == [[100, 0], [100, S]]


def test_every_variant_is_drawn_about_a_third_of_the_time():
    count = {p: 0 for p in POL.pcts}
    for step in range(30):
        plan = R.speed_plan_ref(None, 100, S, POL, 0, step)
        for p in plan[:, 0].tolist():
            count[p] += 1
    print(count)
    assert sum(count.values()) == 3000 and all(900 <= c <= 1100 for c in count.values())


# ----------------------------------------------------------------------------------- the output
def test_identity_policy_returns_the_input_bit_for_bit():
    B = 3
    x = _signal(B, 333)
    x[0, 5], x[1, 7] = -0.0, float("inf")
    lens = torch.tensor([333, 200, 0], dtype=torch.int32)
    x[1, 200:] = float("nan")
    sp = SP.SpeedPerturb(SP.SpeedPolicy((100,)), seed=1)
    y, out_lens = sp(x, lens, step=0)
    assert y.shape == (B, 480) and y.dtype == torch.float32 and out_lens.tolist() == [333, 200, 0]
    for b, n in enumerate(out_lens.tolist()):
        assert torch.equal(y[b, :n].view(torch.int32), x[b, :n].view(torch.int32))
        assert bool((y[b, n:].view(torch.int32) == 0).all())                   # +0 over NaN
    xi = torch.randint(-32768, 32768, (B, 333), generator=torch.Generator().manual_seed(2)).to(torch.int16)
    xi[0, 0], xi[0, 1] = -32768, 32767
    yi, _ = sp(xi, None, step=0)
    assert yi.dtype == torch.float32 and torch.equal(yi[:, :333], xi.to(torch.float32)) and not yi[:, 333:].any()


def test_reference_rows_are_resample_ref_of_the_row_alone():
    B = 6
    x = _signal(B, S, 3)
    lens = torch.tensor([2400, 921, 1127, 1, 0, 2399], dtype=torch.int32)
    for b in range(B):
        x[b, int(lens[b]):] = float("nan")
    sp = SP.SpeedPerturb(POL, seed=7)
    step = next(s for s in range(100) if set(R.speed_plan_ref(lens, B, S, POL, 7, s, 5)[:, 0].tolist()) == set(POL.pcts))
    y, out_lens = sp(x, lens, step=step, first_utt=5)
    assert y.shape == (B, 2720) and set(sp.plan[:, 0].tolist()) == set(POL.pcts)
    assert torch.equal(out_lens, sp.plan[:, 1])
    for b in range(B):
        pct, n_out = sp.plan[b].tolist()
        row = x[b, :int(lens[b])].numpy()
        want = row if pct == 100 else R.resample_ref(row, pct, 100).astype(np.float32)
        assert want.shape[0] == n_out
        assert np.array_equal(y[b, :n_out].numpy(), want)
        assert bool((y[b, n_out:].view(torch.int32) == 0).all())
    tight = sp.tight_width(lens, B, S, step, 5)
    assert tight == R.speed_round_width(int(out_lens.max())) and tight % 160 == 0
    y2, l2 = sp(x, lens, step=step, first_utt=5, out_width=tight)
    assert torch.equal(y2, y[:, :tight]) and torch.equal(l2, out_lens)
    comp, lc = SP.speed_composite(x, lens, sp.plan, POL, 2720)              # the torch composite, on the CPU
    assert torch.equal(lc, out_lens) and bool(torch.isfinite(comp).all())
    assert float((comp - y).abs().max()) < 1e-5 and bool((comp[:, 2667:] == 0).all())
    for bad in (100, 0, 2700):
        with pytest.raises(ValueError):
            sp(x, lens, step=2, out_width=bad)


# -------------------------------------------------------------------------------- the front end
def _audio_batch(N=4, frames=60, seed=1):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    hb = FixedShapeBatches(N, frames, seed=seed, pool=1, audio=True).next()
    hb.labels[:, 2:], hb.label_lens[:] = -1, 2          # short labels: the CTC floor leaves room to speed up
    return hb, to_device(hb, torch.device("cpu"))


def test_ctc_floor_and_frame_cap_in_samples():
    from deepspeech_amd.data import audio_batch as AB
    from deepspeech_amd.ops.featurize import num_frames
    for kind in ("mfcc", "spectrogram"):
        for frames in (1, 2, 3, 50, 118):
            n = AB.samples_for_frames(frames, kind)
            assert num_frames(n, kind) >= frames and (n == 0 or num_frames(n - 1, kind) < frames)
            m = AB.max_samples_for_frames(frames, kind)
            assert num_frames(m, kind) <= frames < num_frames(m + 1, kind)
    labels = torch.tensor([[3, 3, 4, 4, 4, 0], [1, 2, 3, 0, 0, 0], [5, 0, 0, 0, 0, 0]], dtype=torch.int32)
    got = AB.ctc_min_samples(labels, torch.tensor([5, 3, 1], dtype=torch.int32), "mfcc")
    want = [AB.samples_for_frames(4 * t2 + 34, "mfcc") for t2 in (5 + 3, 3, 1)]   # the store's min_frames rule
    assert got.dtype == torch.int32 and got.tolist() == want


def test_front_end_on_the_cpu_equals_featurizing_the_reference_rows():
    from deepspeech_amd.data import audio_batch as AB
    from deepspeech_amd.ops.featurize import AudioFeaturizer
    hb, b = _audio_batch()
    N, Rr, _ = b["feats"].shape
    pcm, lens = b["feats"].reshape(N, Rr * 160), (b["seq_lens"] * 160).to(torch.int32)
    min_out = AB.ctc_min_samples(b["labels"], b["label_lens"], "mfcc")
    step = next(s for s in range(100)
                if set(R.speed_plan_ref(lens, N, Rr * 160, POL, 3, s, 8, min_out)[:, 0].tolist()) == set(POL.pcts))
    sp = SP.SpeedPerturb(POL, seed=3)
    front = AB.AudioFrontEnd("mfcc", "cpu", speed=sp)
    out = front(b, step=step, first_utt=8, training=True)
    plan = sp.plan.clone()
    assert set(plan[:, 0].tolist()) == set(POL.pcts)
    W = SP.speed_out_width(Rr * 160, POL)
    rows, counts = torch.zeros(N, W), []
    for i in range(N):
        pct, n_out = plan[i].tolist()
        row = pcm[i, :int(lens[i])].numpy()
        r = row if pct == 100 else R.resample_ref(row, pct, 100).astype(np.float32)
        assert r.shape[0] == n_out >= int(min_out[i])
        rows[i, :n_out] = torch.from_numpy(r)
        counts.append(n_out)
    feats, frames = AudioFeaturizer("mfcc", device="cpu", normalize="utterance")(rows, torch.tensor(counts, dtype=torch.int32))
    assert torch.equal(out["feats"], feats) and torch.equal(out["seq_lens"], frames)
    # the host batch gives the tight width: the same frames, fewer padding rows
    tight = front(b, step=step, first_utt=8, training=True, host=hb)
    T = tight["feats"].shape[1]
    assert T <= feats.shape[1] and torch.equal(tight["seq_lens"], frames)
    assert torch.equal(tight["feats"], feats[:, :T]) and not feats[:, T:].any()
    # a frame cap below every slowed-down row: none is slowed down
    capped = AB.AudioFrontEnd("mfcc", "cpu", speed=sp, max_frames=int(b["seq_lens"].min()) - 1)
    capped(b, step=step, first_utt=8, training=True)
    assert 90 not in sp.plan[:, 0].tolist() and 110 in sp.plan[:, 0].tolist()


def test_front_end_never_perturbs_outside_training():
    from deepspeech_amd.data.audio_batch import AudioFrontEnd
    _, b = _audio_batch()
    sp = SP.SpeedPerturb(POL, seed=3)
    plain, front = AudioFrontEnd("mfcc", "cpu"), AudioFrontEnd("mfcc", "cpu", speed=sp)
    base = plain(b)
    for kw in (dict(), dict(step=4, first_utt=8), dict(step=4, training=False)):
        out = front(b, **kw)
        assert torch.equal(out["feats"], base["feats"]) and torch.equal(out["seq_lens"], base["seq_lens"])
    assert sp.plan is None


# ------------------------------------------------------------------------------------ the driver
def test_speed_perturb_is_a_training_hyper_parameter():
    from deepspeech_amd import config as C
    assert "speed_perturb" not in C.RESUME_KEYS and "speed_perturb" not in C.EVAL_KEYS
    assert C.build_train_parser().parse_args([]).speed_perturb == ""
    assert not hasattr(C.build_eval_parser().parse_args([]), "speed_perturb")


def test_driver_raises_on_a_frame_store():
    from deepspeech_amd import config as C
    from deepspeech_amd import train as TR

    class _Index:
        is_audio = False

    class _Src:
        index = _Index()
    args = C.build_train_parser().parse_args(["--speed_perturb", "0.9,1.0,1.1"])
    with pytest.raises(ValueError, match="--speed_perturb.*preprocess --store audio"):
        TR.build_front_end(args, _Src(), torch.device("cpu"), False)
    args = C.build_train_parser().parse_args(["--dummy", "True", "--speed_perturb", "0.9,1.0,1.1"])
    with pytest.raises(ValueError, match="preprocess --store audio"):
        TR.build_front_end(args, _Src(), torch.device("cpu"), False)
    args = C.build_train_parser().parse_args(["--dummy", "True", "--dummy_audio", "True", "--speed_perturb", "0.9,1.1",
                                              "--max_frames", "500"])
    front = TR.build_front_end(args, _Src(), torch.device("cpu"), False)
    assert front.speed.policy.pcts == (90, 110) and front.wave_aug is None and front.max_out == 400 + 160 * 499


def _train_cmd(d, steps, extra):
    return [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--dummy_audio", "True", "--dummy_frames", "80",
            "--batch_size", "3", "--num_hidden", "16", "--num_rnn_layers", "1", "--num_filters", "4", "--device", "cpu",
            "--max_steps", str(steps), "--train_dir", d, "--log_every", "1000", "--checkpoint_every", "1",
            "--async_checkpoint", "False"] + extra


def _last_loss(d, step):
    recs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    recs = [r for r in recs if r.get("step") == step and "loss" in r]
    assert recs, "no loss record of step %d" % step
    return recs[-1]["loss"]


def test_a_resumed_dummy_audio_run_reproduces_the_uninterrupted_one(tmp_path):
    """deepspeech_amd.train from dummy audio on the CPU, tiny model, 3 steps; the loss of the last
    step (step 2, which depends on both steps before it) is compared: the flag changes it, and a
    run stopped after step 1 and resumed from its checkpoint reproduces the uninterrupted run's
    step 2 bitwise (the same batch under the same ratios at the same global step)."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    flag = ["--speed_perturb", "0.9,1.0,1.1"]
    runs = {"plain": (3, []), "aug": (3, flag), "head": (2, flag)}
    procs = {k: subprocess.Popen(_train_cmd(str(tmp_path / k), n, extra), env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for k, (n, extra) in runs.items()}
    outs = {}
    for k, p in procs.items():
        outs[k] = p.communicate(timeout=600)[0]
        assert p.returncode == 0, outs[k][-3000:]
    loss = {k: _last_loss(str(tmp_path / k), runs[k][0] - 1) for k in runs}
    print(loss)
    assert "speed_perturb:  0.9,1,1.1" in outs["aug"] and "speed_perturb" not in outs["plain"]
    assert math.isfinite(loss["aug"]) and loss["aug"] != loss["plain"]
    d = str(tmp_path / "head")
    r = subprocess.run(_train_cmd(d, 3, flag + ["--checkpoint", d]), env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "has checkpoint" in r.stdout
    assert _last_loss(d, 2) == loss["aug"]
