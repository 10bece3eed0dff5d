"""The noise-augmentation kernels (csrc/waveaug.hip) against the fp64 / integer oracle of
ops/reference.py, the audio front end on the GPU, and a small training run from dummy audio.

Bounds: a segment's fp32 sum passes every (non-negative) term through at most 30 additions and
the partials are added in fp64, so Ex and En are within (1 + u)^31 - 1 < 32 u, u = 2^-24, of the
oracle; k = sqrt(Ex / (En c)) takes half of each plus its own rounding: 34 u."""
import functools

import numpy as np
import pytest
import torch

from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops import waveaug as WA

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LENS = [8200, 4097, 4096, 4095, 1, 0]
CLIPS = (160, 1000, 5000, 20000)
POL = WA.WaveAugPolicy.parse("p=0.7,snr=0:30")


def _bank():
    rng = np.random.default_rng(17)
    return WA.NoiseBank([(rng.standard_normal(n) * (0.5 + i)).astype(np.float32) for i, n in enumerate(CLIPS)])


BANK = _bank()


@functools.lru_cache(maxsize=None)
def _select(S):
    """The first (seed, step = 3) whose plan, by the CPU reference, uses every clip, leaves a
    non-empty row off, and has an on row whose clip is longer than the utterance and still wraps."""
    lens = torch.tensor(LENS, dtype=torch.int32)
    n = lens.clamp(0, S).long()
    for seed in range(4000):
        plan = R.waveaug_plan_ref(lens, len(LENS), S, BANK.length, POL, seed, 3).long()
        length = BANK.length.long()[plan[:, 1]]
        on = plan[:, 0] != 0
        wraps = on & (plan[:, 2] + n > length)
        if (sorted(set(plan[:, 1].tolist())) == list(range(len(CLIPS))) and bool((wraps & (length > n)).any())
                and bool((~on & (n > 0)).any()) and int(on.sum()) >= 3):
            return seed, 3, plan
    raise AssertionError("no seed gives the wanted plan")


def _x(S, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = len(LENS)
    if dtype == torch.int16:
        x = (torch.randn(B, S, generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    else:
        x = torch.randn(B, S, generator=g) * 0.3 + 0.01
        x[0, 0] = -0.0
    return x


_runs = {}


def run(cuda, S, dtype):
    """One kernel call per (S, dtype), shared by the tests: inputs, planted NaN in the tails (fp32),
    the reference and the kernel's tensors on the host."""
    key = (S, dtype)
    if key not in _runs:
        seed, step, want_plan = _select(S)
        x = _x(S, dtype)
        lens = torch.tensor(LENS, dtype=torch.int32)
        n = lens.clamp(0, S)
        if dtype == torch.float32:
            for b in range(len(LENS)):
                x[b, int(n[b]):] = float("nan")
        xd = x.to(cuda)
        assert WA.kernels_cover(xd)
        aug = WA.WaveAugment(POL, BANK, seed)
        y = aug(xd, lens.to(cuda), step)
        ref = R.waveaug_ref(x, lens, BANK, POL, seed, step)
        _runs[key] = dict(x=x, lens=lens, n=n, seed=seed, step=step, y=y.cpu(), plan=aug.plan.cpu(),
                          energy=aug.energy.cpu(), coef=aug.coef.cpu(), ref=ref, want_plan=want_plan)
        torch.cuda.synchronize()
    return _runs[key]


CASES = [(8200, torch.float32), (8200, torch.int16), (8, torch.float32), (8, torch.int16)]
IDS = ["S8200-f32", "S8200-i16", "S8-f32", "S8-i16"]


def test_case_selection():
    for S in (8200, 8):
        seed, step, plan = _select(S)
        n = torch.tensor(LENS).clamp(0, S)
        length = BANK.length.long()[plan[:, 1]]
        print("S", S, "seed", seed, "plan", plan.tolist())
        assert set(plan[:, 1].tolist()) == {0, 1, 2, 3}
        assert bool(((plan[:, 0] != 0) & (plan[:, 2] + n > length) & (length > n)).any())


@pytest.mark.parametrize("S,dtype", CASES, ids=IDS)
def test_plan_equals_reference(cuda, S, dtype):
    r = run(cuda, S, dtype)
    assert r["plan"].dtype == torch.int32 and torch.equal(r["plan"], r["ref"][1])
    assert torch.equal(r["plan"].long(), r["want_plan"])


@pytest.mark.parametrize("S,dtype", CASES, ids=IDS)
def test_energies_and_coefficient(cuda, S, dtype):
    r = run(cuda, S, dtype)
    e, eo = r["energy"], r["ref"][2]
    assert e.dtype == torch.float64 and e.shape == (len(LENS), 2)
    rel = ((e - eo).abs() / eo.clamp(min=1e-300)).max(0).values
    print("max relative error of Ex %.3g, En %.3g (bound %.3g)" % (float(rel[0]), float(rel[1]), 32 * U))
    assert bool(((e - eo).abs() <= 32 * U * eo).all())
    k, ko = r["coef"].double(), r["ref"][3].double()
    print("max relative error of k %.3g (bound %.3g)" % (float(((k - ko).abs() / ko.clamp(min=1e-300)).max()), 34 * U))
    assert bool(((k - ko).abs() <= 34 * U * ko).all())
    on = r["plan"][:, 0] != 0
    assert bool((k[~on] == 0).all()) and bool((k[on & (r["n"] > 0)] > 0).all())
    assert float(e[5, 0]) == 0.0 and float(e[5, 1]) == 0.0 and float(k[5]) == 0.0          # n == 0


@pytest.mark.parametrize("S,dtype", CASES, ids=IDS)
def test_output(cuda, S, dtype):
    r = run(cuda, S, dtype)
    x, y, plan = r["x"], r["y"], r["plan"]
    assert y.dtype == torch.float32 and y.shape == x.shape
    z = R.waveaug_noise_ref(plan, BANK.data, BANK.start, BANK.length, S)
    want = R.waveaug_mix_ref(x, r["lens"], plan, z, r["coef"])          # x + k * z in fp32 from the kernel's own k
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    xf = x.to(torch.float32)
    changed = False
    for b in range(len(LENS)):
        n = int(r["n"][b])
        assert bool((y[b, n:].view(torch.int32) == 0).all())            # +0 over the planted NaN
        if int(plan[b, 0]) == 0:
            assert torch.equal(y[b, :n].view(torch.int32), xf[b, :n].view(torch.int32))    # a bit copy
        elif n > 0:
            changed = changed or not torch.equal(y[b, :n], xf[b, :n])
    assert changed
    # against the whole reference: its k differs from the kernel's by at most 34 u, each product
    # rounds once (u of itself) and each sum rounds once (u of itself)
    yo = r["ref"][0]
    kz = (r["coef"][:, None] * z).abs().double()
    big = torch.maximum(y.abs(), yo.abs()).double()
    assert bool(((y.double() - yo.double()).abs() <= 37 * U * kz + 2.1 * U * big).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
def test_energy_and_k_do_not_depend_on_the_batch_or_the_row(cuda, dtype):
    S = 8200
    r = run(cuda, S, dtype)
    others = _x(S, dtype, seed=5)
    for b in range(len(LENS)):
        xb, lb = r["x"][b:b + 1], r["lens"][b:b + 1]
        aug = WA.WaveAugment(POL, BANK, r["seed"])
        y1 = aug(xb.contiguous().to(cuda), lb.to(cuda), r["step"], first_utt=b)
        assert torch.equal(aug.plan.cpu()[0], r["plan"][b])
        assert torch.equal(aug.energy.cpu()[0].view(torch.int64), r["energy"][b].view(torch.int64))
        assert torch.equal(aug.coef.cpu().view(torch.int32), r["coef"][b:b + 1].view(torch.int32))
        assert torch.equal(y1.cpu().view(torch.int32), r["y"][b:b + 1].view(torch.int32))
        # as row 2 of another batch, the same global utterance index
        x3 = torch.cat([others[:2], xb, others[2:3]], 0).contiguous()
        l3 = torch.tensor([S, 100, int(lb[0]), 4096], dtype=torch.int32)
        y3 = aug(x3.to(cuda), l3.to(cuda), r["step"], first_utt=(b - 2) & 0xffffffff)
        assert torch.equal(aug.plan.cpu()[2], r["plan"][b])
        assert torch.equal(aug.energy.cpu()[2].view(torch.int64), r["energy"][b].view(torch.int64))
        assert torch.equal(aug.coef.cpu()[2:3].view(torch.int32), r["coef"][b:b + 1].view(torch.int32))
        assert torch.equal(y3.cpu()[2:3].view(torch.int32), r["y"][b:b + 1].view(torch.int32))


def test_int16_is_the_fp32_of_the_same_samples(cuda):
    r = run(cuda, 8200, torch.int16)
    aug = WA.WaveAugment(POL, BANK, r["seed"])
    y = aug(r["x"].to(torch.float32).to(cuda), r["lens"].to(cuda), r["step"])
    assert torch.equal(y.cpu(), r["y"]) and torch.equal(aug.energy.cpu(), r["energy"])


def test_lens_none_is_the_whole_row(cuda):
    x = _x(4104, torch.float32)
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=5:25"), BANK, 21)
    y = aug(x.to(cuda), None, 9)
    e, k = aug.energy.cpu(), aug.coef.cpu()
    y2 = aug(x.to(cuda), torch.full((len(LENS),), 4104, dtype=torch.int32, device=cuda), 9)
    assert torch.equal(y.cpu(), y2.cpu()) and torch.equal(e, aug.energy.cpu()) and torch.equal(k, aug.coef.cpu())
    yo, plan, eo, ko = R.waveaug_ref(x, None, BANK, aug.policy, 21, 9)
    assert torch.equal(aug.plan.cpu(), plan)
    assert bool(((e - eo).abs() <= 32 * U * eo).all()) and bool(((k - ko).abs().double() <= 34 * U * ko.double()).all())


@pytest.mark.parametrize("how", ["S % 8 != 0", "strided view", "column slice"])
def test_uncovered_inputs_take_the_composite(cuda, how):
    S = 8197 if how == "S % 8 != 0" else 8200
    base = _x(2 * 8200 + 8, torch.float32, seed=3).to(cuda)
    xd = {"S % 8 != 0": base[:, :S], "strided view": base[:, :2 * S:2], "column slice": base[:, 4:4 + S]}[how]
    if how == "S % 8 != 0":
        xd = xd.contiguous()
    assert not WA.kernels_cover(xd) and xd.shape == (len(LENS), S)
    lens = torch.tensor(LENS, dtype=torch.int32)
    aug = WA.WaveAugment(POL, BANK, 12)
    y = aug(xd, lens.to(cuda), 4, first_utt=7).cpu()
    x = xd.cpu().contiguous()
    yo, plan, eo, ko = R.waveaug_ref(x, lens, BANK, POL, 12, 4, first_utt=7)
    assert torch.equal(aug.plan.cpu(), plan)
    e, k = aug.energy.cpu(), aug.coef.cpu()
    assert bool(((e - eo).abs() <= 32 * U * eo).all()) and bool(((k - ko).abs().double() <= 34 * U * ko.double()).all())
    z = R.waveaug_noise_ref(plan, BANK.data, BANK.start, BANK.length, S)
    assert torch.equal(y.view(torch.int32), R.waveaug_mix_ref(x, lens, plan, z, k).view(torch.int32))


def test_front_end_equals_the_featurizer(cuda):
    from deepspeech_amd.data.audio_batch import AudioFrontEnd
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.ops.featurize import AudioFeaturizer
    b = to_device(FixedShapeBatches(4, 60, seed=1, pool=1, audio=True).next(), cuda)
    N, Rr, _ = b["feats"].shape
    pcm, lens = b["feats"].reshape(N, Rr * 160), (b["seq_lens"] * 160).to(torch.int32)
    for kind in ("mfcc", "spectrogram"):
        out = AudioFrontEnd(kind, cuda)(b, step=5, training=True)       # no augmentation configured
        feats, frames = AudioFeaturizer(kind, device=cuda, normalize="utterance")(pcm, lens)
        assert torch.equal(out["feats"], feats) and torch.equal(out["seq_lens"], frames)
        assert out["seq_lens"].cpu().tolist() == (b["seq_lens"].cpu() - 1).tolist() and feats.shape == (N, Rr - 1, 161)
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=10:10"), BANK, 2)
    front = AudioFrontEnd("mfcc", cuda, wave_aug=aug)
    noisy = front(b, step=5, first_utt=4, training=True)
    want, _ = AudioFeaturizer("mfcc", device=cuda, normalize="utterance")(aug(pcm, lens, 5, first_utt=4), lens)
    assert torch.equal(noisy["feats"], want) and not torch.equal(noisy["feats"], front(b, step=5)["feats"])


def _three_steps(cuda):
    from deepspeech_amd.data.audio_batch import AudioFrontEnd
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.trainer import LRSchedule, Trainer
    torch.manual_seed(0)
    model = DeepSpeech2(num_filters=32, num_hidden=256, num_rnn_layers=2, cell="gru").to(cuda)
    model.set_engine("hip", torch.bfloat16)
    tr = Trainer(model, LRSchedule(1e-4, 1000, 0.9))
    src = FixedShapeBatches(8, max_frames=120, seed=0, pool=2, audio=True)
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=0.5,snr=5:20"), WA.NoiseBank.synthetic(0), 1234)
    front = AudioFrontEnd("mfcc", cuda, wave_aug=aug)
    losses, plans = [], []
    for step in range(3):
        batch = front(to_device(src.next(), cuda), step, first_utt=0, training=True)
        losses.append(tr.step(batch).detach().clone())
        plans.append(aug.plan.cpu())
    tr.flush()
    torch.cuda.synchronize()
    RNN.check_errors()
    return torch.stack([l.reshape(()) for l in losses]).cpu(), plans


def test_training_from_dummy_audio_is_finite_and_repeatable(cuda):
    a, plans = _three_steps(cuda)
    b, _ = _three_steps(cuda)
    print("losses", a.tolist())
    assert bool(torch.isfinite(a).all()) and bool((a > 0).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert any(int(p[:, 0].sum()) > 0 for p in plans) and not torch.equal(plans[0], plans[1])
