"""Additive noise at a random SNR on the waveform: the definition (ops/reference.py), the parser
and the CPU path of ops/waveaug.py, which is the reference itself."""
import numpy as np
import pytest
import torch

from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops import waveaug as WA

BANK = WA.NoiseBank.synthetic(3)
POL = WA.WaveAugPolicy.parse("noise=synthetic,p=0.4,snr=10:30")


def _plan(lens, B, S, pol=POL, seed=0, step=0, first_utt=0, bank=BANK):
    return R.waveaug_plan_ref(lens, B, S, bank.length, pol, seed, step, first_utt)


# ---------------------------------------------------------------------------------------- plan
def test_plan_row_is_a_function_of_the_utterance_alone():
    g = torch.Generator().manual_seed(1)
    B, S = 12, 50000
    lens = torch.randint(0, S + 1, (B,), generator=g).to(torch.int32)
    for seed, step in ((7, 3), (2 ** 40 + 5, 2 ** 33 + 9)):
        full = _plan(lens, B, S, seed=seed, step=step, first_utt=10)
        for b in range(B):
            alone = _plan(lens[b:b + 1], 1, S, seed=seed, step=step, first_utt=10 + b)
            assert torch.equal(alone[0], full[b])
        assert torch.equal(_plan(lens[3:], B - 3, S, seed=seed, step=step, first_utt=13), full[3:])
    assert not torch.equal(_plan(lens, B, S, seed=7, step=3), _plan(lens, B, S, seed=7, step=4))
    assert not torch.equal(_plan(lens, B, S, seed=7, step=3), _plan(lens, B, S, seed=7, step=3 + 2 ** 32))


def test_plan_stream_is_apart_from_specaug_and_dropout():
    # bit 30 of the last counter word: set here, clear for SpecAugment; bit 31 set for dropout
    assert R.WAVEAUG_STREAM == 1 << 30
    u = np.arange(4, dtype=np.uint64)
    ours = R.philox4x32((np.uint64(0), u, np.uint64(5), np.uint64(R.WAVEAUG_STREAM)), (np.uint64(9), np.uint64(0)))
    spec = R.philox4x32((np.uint64(0), u, np.uint64(5), np.uint64(0)), (np.uint64(9), np.uint64(0)))
    assert not np.array_equal(ours[0], spec[0])
    lens = torch.full((4,), 100, dtype=torch.int32)
    plan = _plan(lens, 4, 100, WA.WaveAugPolicy(p_ppm=500000, snr_lo_cdb=0, snr_hi_cdb=0), seed=9, step=5)
    assert plan[:, 0].tolist() == [int((int(w) * 1000000) >> 32 < 500000) for w in ours[0]]


def test_plan_statistics_seed0_step0():
    B, S = 4096, 16000
    lens = torch.full((B,), S, dtype=torch.int32)
    plan = _plan(lens, B, S)
    share = float(plan[:, 0].float().mean())
    print("share of on rows: %.4f" % share)
    assert 0.36 <= share <= 0.44                       # 5 sigma of the binomial around p = 0.4
    C = len(BANK)
    assert int(plan[:, 1].min()) >= 0 and int(plan[:, 1].max()) < C
    assert sorted(set(plan[:, 1].tolist())) == list(range(C))
    assert bool((plan[:, 2] >= 0).all()) and bool((plan[:, 2] < BANK.length[plan[:, 1].long()]).all())
    # p = 1: every row is on, and over those rows snr=10:30 reaches both of its ends
    p1 = _plan(lens, B, S, WA.WaveAugPolicy.parse("p=1,snr=10:30"))
    assert bool((p1[:, 0] == 1).all())
    print("snr range over the rows of p = 1: %d .. %d" % (int(p1[:, 3].min()), int(p1[:, 3].max())))
    assert int(p1[:, 3].min()) == 1000 and int(p1[:, 3].max()) == 3000
    assert torch.equal(p1[:, 1:], plan[:, 1:])


def test_plan_p0_none_p1_every_nonempty_row():
    B, S = 4096, 16000
    lens = torch.full((B,), S, dtype=torch.int32)
    lens[::7] = 0
    lens[1::7] = -5
    p0 = _plan(lens, B, S, WA.WaveAugPolicy.parse("p=0,snr=10:30"))
    p1 = _plan(lens, B, S, WA.WaveAugPolicy.parse("p=1,snr=10:30"))
    assert int(p0[:, 0].sum()) == 0
    assert torch.equal(p1[:, 0] != 0, lens > 0)
    assert torch.equal(p0[:, 1:], p1[:, 1:])           # clip, off and snr are filled whatever on is


def test_plan_lens_none_means_whole_rows():
    assert torch.equal(_plan(None, 5, 800), _plan(torch.full((5,), 800), 5, 800))
    assert torch.equal(_plan(None, 5, 800), _plan(torch.full((5,), 10 ** 6), 5, 800))


# ----------------------------------------------------------------------------------------- mix
def _signal(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S, dtype=torch.float64)
    x = torch.sin(t[None, :] * (0.01 + 0.003 * torch.arange(B, dtype=torch.float64)[:, None]))
    return (x * 0.3 + 0.05 * torch.randn(B, S, generator=g, dtype=torch.float64)).to(torch.float32)


def test_achieved_snr():
    B, S = 6, 8200
    x = _signal(B, S)
    lens = torch.tensor([8200, 4097, 4096, 4095, 161, 1], dtype=torch.int32)
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=-5:30"), BANK, seed=4)
    y = aug(x, lens, step=2)
    assert y.dtype == torch.float32 and y.shape == x.shape
    assert bool((aug.plan[:, 0] != 0).all())
    for b in range(B):
        n = int(lens[b])
        xd, yd = x[b, :n].double(), y[b, :n].double()
        ex, ed = float((xd ** 2).sum()), float(((yd - xd) ** 2).sum())
        got = 10 * np.log10(ex / ed)
        print("row %d n %d: snr %.5f dB, asked %.2f" % (b, n, got, int(aug.plan[b, 3]) / 100.0))
        assert abs(got - int(aug.plan[b, 3]) / 100.0) < 1e-3
        assert abs(float(aug.energy[b, 0]) - ex) <= 1e-12 * ex


def test_p0_returns_the_input_bit_for_bit():
    B, S = 3, 333
    x = _signal(B, S)
    x[0, 5] = -0.0
    x[1, 7] = float("inf")
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=0"), BANK, seed=1)
    y = aug(x, None, step=0)
    assert torch.equal(y.view(torch.int32), x.view(torch.int32))
    assert bool((aug.coef == 0).all())
    xi = torch.randint(-32768, 32768, (B, S), generator=torch.Generator().manual_seed(2)).to(torch.int16)
    xi[0, 0], xi[0, 1] = -32768, 32767
    yi = aug(xi, None, step=0)
    assert yi.dtype == torch.float32 and torch.equal(yi, xi.to(torch.float32))     # no 1/32768


def test_tail_is_plus_zero_over_nan():
    B, S = 4, 1000
    x = _signal(B, S)
    lens = torch.tensor([1000, 640, 1, 0], dtype=torch.int32)
    for b in range(B):
        x[b, int(lens[b]):] = float("nan")
    for spec in ("p=1,snr=10:20", "p=0"):
        aug = WA.WaveAugment(WA.WaveAugPolicy.parse(spec), BANK, seed=3)
        y = aug(x, lens, step=1)
        for b in range(B):
            tail = y[b, int(lens[b]):]
            assert bool((tail.view(torch.int32) == 0).all())                       # +0, not -0, not NaN
            assert bool(torch.isfinite(y[b, :int(lens[b])]).all())
        assert bool(torch.isfinite(aug.energy).all()) and bool(torch.isfinite(aug.coef).all())
        assert float(aug.coef[3]) == 0.0 and int(aug.plan[3, 0]) == 0              # n == 0 is never on


def test_silence_and_silent_noise_give_k_zero():
    S = 800
    x = torch.zeros(2, S)
    x[1] = _signal(1, S)[0]
    bank = WA.NoiseBank([np.zeros(160, np.float32)])
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=10:10"), BANK, seed=0)
    aug(x, None, step=0)
    assert float(aug.coef[0]) == 0.0 and float(aug.coef[1]) > 0.0                  # Ex == 0
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=10:10"), bank, seed=0)
    y = aug(x, None, step=0)
    assert bool((aug.coef == 0).all()) and torch.equal(y, x)                       # En == 0


def test_short_clip_wraps_with_its_period():
    S = n = 8200
    x = _signal(1, S)
    clip = np.random.default_rng(5).standard_normal(160).astype(np.float32)
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=5:5"), WA.NoiseBank([clip]), seed=8)
    y = aug(x, torch.tensor([n], dtype=torch.int32), step=0)
    d = y[0].double() - x[0].double()
    # y = fl32(x + fl32(k z)): y - x is k z up to half an ulp of y, and z has period 160
    slack = 2.0 ** -24 * (y[0, :-160].abs().double() + y[0, 160:].abs().double())
    assert bool(((d[:-160] - d[160:]).abs() <= slack).all())
    assert float(d.abs().max()) > 0
    k, off = float(aug.coef[0]), int(aug.plan[0, 2])
    want = torch.from_numpy(clip[(off + np.arange(S)) % 160]) * aug.coef[0]
    assert torch.equal(y[0], x[0] + want) and k > 0


def test_reference_pieces_compose():
    B, S = 3, 4000
    x = _signal(B, S)
    lens = torch.tensor([4000, 2000, 17], dtype=torch.int32)
    y, plan, energy, coef = R.waveaug_ref(x, lens, BANK, POL, seed=11, step=5, first_utt=2)
    z = R.waveaug_noise_ref(plan, BANK.data, BANK.start, BANK.length, S)
    assert torch.equal(R.waveaug_mix_ref(x, lens, plan, z, coef), y)
    assert torch.equal(R.waveaug_coef_ref(plan, energy), coef)
    comp, e2, c2 = WA.waveaug_composite(x, lens, plan, BANK)                       # the torch composite, on the CPU
    assert torch.equal(comp, y) and torch.equal(c2, coef)
    assert torch.allclose(e2, energy, rtol=1e-13, atol=0)


# -------------------------------------------------------------------------------- parser, bank
def test_parser():
    p = WA.WaveAugPolicy.parse("noise=/some/dir, p=0.4, snr=10:30")
    assert (p.noise, p.p_ppm, p.snr_lo_cdb, p.snr_hi_cdb) == ("/some/dir", 400000, 1000, 3000)
    assert WA.WaveAugPolicy.parse("snr=12.5").snr_lo_cdb == WA.WaveAugPolicy.parse("snr=12.5").snr_hi_cdb == 1250
    assert WA.WaveAugPolicy.parse("snr=-5:7.25") == WA.WaveAugPolicy(snr_lo_cdb=-500, snr_hi_cdb=725)
    assert WA.WaveAugPolicy.parse(str(p)) == p
    for bad in ("gain=3", "p=0.4,p=0.5", "p", "snr=30:10", "p=1.5", "p=-0.1", "snr=a:b", "noise=", "snr=10:99999"):
        with pytest.raises(ValueError):
            WA.WaveAugPolicy.parse(bad)


def test_noise_bank(tmp_path):
    with pytest.raises(ValueError):
        WA.NoiseBank([])
    with pytest.raises(ValueError):
        WA.NoiseBank([np.zeros(159, np.float32)])
    with pytest.raises(ValueError):
        WA.NoiseBank([np.full(200, np.nan, np.float32)])
    a, b = WA.NoiseBank.synthetic(1), WA.NoiseBank.synthetic(1)
    assert torch.equal(a.data, b.data) and not torch.equal(a.data, WA.NoiseBank.synthetic(2).data)
    assert len(set(a.length.tolist())) == len(a) >= 3
    assert a.start.tolist() == (np.cumsum(a.length.numpy()) - a.length.numpy()).tolist()
    assert int(a.start[-1] + a.length[-1]) == a.data.numel()
    rng = np.random.default_rng(0)
    np.save(tmp_path / "b.npy", rng.standard_normal(500))
    np.save(tmp_path / "a.npy", rng.standard_normal(300))
    bank = WA.NoiseBank.from_dir(str(tmp_path))
    assert bank.length.tolist() == [300, 500]                                      # sorted file order
    np.save(tmp_path / "c.npy", rng.standard_normal(20))
    with pytest.raises(ValueError):
        WA.NoiseBank.from_dir(str(tmp_path))


def test_wave_aug_is_a_training_hyper_parameter():
    from deepspeech_amd import config as C
    assert "wave_aug" not in C.RESUME_KEYS and "wave_aug" not in C.EVAL_KEYS
    assert "audio_features" in C.RESUME_KEYS and "audio_features" in C.EVAL_KEYS
    a = C.build_train_parser().parse_args([])
    assert a.wave_aug == "" and a.audio_features == "mfcc" and a.dummy_audio is False
