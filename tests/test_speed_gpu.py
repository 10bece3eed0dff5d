"""The speed-perturbation kernels (csrc/speed.hip) against the integer / fp64 oracle of
ops/reference.py and, bit for bit, against the resampling kernel run on each row alone; the audio
front end on the GPU; a small training run from dummy audio.

Bound, for every output with A = sum_k |h[ph, k] x[.]| taken from the oracle:
|y - y64| <= (2K + 2) 2^-24 A, the bound of tests/test_resample_gpu.py (a K-term fp32 fma chain
with a once-rounded table); an identity row is exact. The torch composite rounds the product and
the sum of every tap, so it gets twice that. No element is left out.

Shapes: B <= 6 rows of S = 2400 samples (15 hops): three output tiles at 90 %, and row lengths
whose last output sits one before, on and one after the first and the second tile boundary."""
import functools

import numpy as np
import pytest
import torch

from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops import resample as RS
from deepspeech_amd.ops import speed as SP

pytestmark = pytest.mark.gpu

S = 2400
POL = SP.SpeedPolicy.parse("0.9,1.0,1.1")
LENS = [2400, 1843, 1127, 921, 2253, 1]
MIN_OUT = [0, 0, 0, 0, 2300, 0]               # row 4 may not speed up: N_110(2253) = 2049
# one before, on and one after 1024 and 2048 outputs, then the ends
EDGES = {90: ([920, 921, 922, 1842, 1843, 1844], [0, 1, S]), 110: ([1125, 1126, 1127, 2251, 2252, 2253], [0, 1, S])}
K_OF = {90: 48, 100: 0, 110: 54}


@functools.lru_cache(maxsize=None)
def _select():
    """The first (seed, step = 3) whose plan, by the CPU reference, holds every variant, a row
    that the min_out guard sends back to the identity, a slowed-down row of two whole tiles, a sped-up row one
    output into its second tile and a whole-width row that is not slowed down (so the tight output width is below the worst case)."""
    for seed in range(4000):
        free = R.speed_plan_ref(LENS, len(LENS), S, POL, seed, 3, first_utt=2)
        plan = R.speed_plan_ref(LENS, len(LENS), S, POL, seed, 3, first_utt=2, min_out=MIN_OUT)
        if (set(plan[:, 0].tolist()) == set(POL.pcts) and free[4].tolist() == [110, 2049] and
                plan[4].tolist() == [100, 2253] and plan[0, 0] != 90 and plan[1].tolist() == [90, 2048] and
                plan[2].tolist() == [110, 1025]):
            return seed, 3, plan
    raise AssertionError("no seed gives the wanted plan")


def _x(B, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S) / 16000.0
    x = torch.stack([9000.0 * torch.sin(2 * np.pi * (200 + 300 * (b + 1) * t) * t) for b in range(B)])
    x = x + 300.0 * torch.randn(B, S, generator=g)
    return x.round().clamp(-32768, 32767).to(torch.int16) if dtype == torch.int16 else x


def planted(x, lens):
    """A copy with NaN (fp32) or full-scale garbage (int16) at and past each row's length."""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n:] = float("nan") if x.dtype.is_floating_point else 32767
    return x


def check_bound(y, y64, a64, plan, factor=1):
    y = y.double().cpu().numpy()
    K = np.array([K_OF[p] for p in plan[:, 0].tolist()], np.float64)[:, None]
    bound = factor * np.where(K > 0, (2 * K + 2) * 2.0 ** -24 * a64, 0.0)       # identity rows: exact
    err = np.abs(y - y64)
    if (bound > 0).any():
        print("max error / bound = %.4f" % float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.isfinite(y).all()
    assert (err <= bound).all()
    assert not y[a64 == 0].any()


def check_tail(y, out_lens):
    y = y.cpu()
    for b, n in enumerate(out_lens.tolist()):
        assert bool((y[b, n:].view(torch.int32) == 0).all())                   # +0: not -0, not NaN


_runs = {}


def run(cuda, dtype):
    """One call of the main case per dtype, shared by the tests: inputs with planted tails, the
    kernel's tensors on the host and the fp64 reference (left unchanged)."""
    if dtype not in _runs:
        seed, step, want = _select()
        x = _x(len(LENS), dtype)
        lens = torch.tensor(LENS, dtype=torch.int32)
        sp = SP.SpeedPerturb(POL, seed)
        xd = planted(x, LENS).to(cuda)
        y, out_lens = sp(xd, lens.to(cuda), step, first_utt=2, min_out=torch.tensor(MIN_OUT, dtype=torch.int32))
        y64, a64, n64 = R.speed_ref(x, lens, want, SP.speed_out_width(S, POL), return_abs=True)
        for a in (y64, a64):
            a.setflags(write=False)
        _runs[dtype] = dict(seed=seed, step=step, want=want, x=x, xd=xd, lens=lens, y=y.cpu(), out_lens=out_lens.cpu(),
                            plan=sp.plan.cpu(), y64=y64, a64=a64, n64=n64)
    return _runs[dtype]


# ------------------------------------------------------------------------------------- the plan
def test_selected_case_holds_every_variant_and_a_fallback():
    seed, step, plan = _select()
    assert sorted(set(plan[:, 0].tolist())) == [90, 100, 110]
    free = R.speed_plan_ref(LENS, len(LENS), S, POL, seed, step, first_utt=2)
    assert free[4, 0] == 110 and plan[4].tolist() == [100, LENS[4]]             # the guard's fallback
    assert int(plan[:, 1].max()) > 2 * RS.TILE_OUT                               # three tiles


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_plan_equals_the_reference(cuda, dtype):
    r = run(cuda, dtype)
    assert r["plan"].dtype == torch.int32 and torch.equal(r["plan"], r["want"])
    sp = SP.SpeedPerturb(POL, r["seed"])
    sp(r["xd"], r["lens"].to(cuda), r["step"], first_utt=2)                      # no min_out
    assert torch.equal(sp.plan.cpu(), R.speed_plan_ref(LENS, len(LENS), S, POL, r["seed"], r["step"], first_utt=2))
    assert not torch.equal(sp.plan.cpu(), r["want"])
    big = (5 << 32) + 7                                                         # both words of seed and step
    lens = torch.tensor([5, 2400, 0, 99999, -3, 1200], dtype=torch.int32)
    for kw in (dict(), dict(min_out=torch.tensor([0, 2401, 0, 0, 0, 1100], dtype=torch.int32)), dict(max_out=2400),
               dict(min_out=torch.tensor([6, 0, 0, 0, 0, 0], dtype=torch.int32), max_out=1300)):
        got = SP.speed_plan(lens.to(cuda), 6, S, POL, big, big + 1, first_utt=0xfffffffe, device=cuda, **kw)
        assert torch.equal(got.cpu(), R.speed_plan_ref(lens, 6, S, POL, big, big + 1, first_utt=0xfffffffe, **kw))
    for pol in (SP.SpeedPolicy((100,)), SP.SpeedPolicy((50, 200, 101, 199, 150, 75, 100, 133))):
        got = SP.speed_plan(None, 70, S, pol, 3, 4, first_utt=9, device=cuda)   # lens None: whole rows; two workgroups
        assert torch.equal(got.cpu(), R.speed_plan_ref(None, 70, S, pol, 3, 4, first_utt=9))


# ----------------------------------------------------------------------------------- the output
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_every_row_is_the_resampling_kernel_on_that_row_alone(cuda, dtype):
    r = run(cuda, dtype)
    y, plan = r["y"], r["plan"]
    assert y.dtype == torch.float32 and y.shape == (len(LENS), 2720) and torch.equal(r["out_lens"], plan[:, 1])
    for b, (pct, n_out) in enumerate(plan.tolist()):
        if pct == 100:
            assert n_out == LENS[b]
            assert torch.equal(y[b, :n_out].view(torch.int32), r["x"][b, :n_out].to(torch.float32).view(torch.int32))
            continue
        rs = RS.Resampler(pct, 100, device=cuda)
        assert rs.use_kernel
        yr, nr = rs(r["xd"][b:b + 1], r["lens"][b:b + 1])
        assert nr.tolist() == [n_out]
        assert torch.equal(y[b, :n_out].view(torch.int32), yr[0, :n_out].cpu().view(torch.int32))
    check_tail(y, r["out_lens"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_every_element_against_the_oracle(cuda, dtype):
    r = run(cuda, dtype)
    assert r["out_lens"].tolist() == r["n64"].tolist()
    check_bound(r["y"], r["y64"], r["a64"], r["plan"])


@pytest.mark.parametrize("pct", [90, 110])
def test_tile_boundaries_and_ends(cuda, pct):
    pol = SP.SpeedPolicy((pct,))
    sp = SP.SpeedPerturb(pol, 0)
    rs = RS.Resampler(pct, 100, device=cuda)
    for lens in EDGES[pct]:
        B = len(lens)
        x = _x(B, torch.float32, seed=pct)
        xd, ln = planted(x, lens).to(cuda), torch.tensor(lens, dtype=torch.int32)
        y, out_lens = sp(xd, ln.to(cuda), 0)
        counts = [R.speed_out_len(n, pct) if n > 0 else 0 for n in lens]
        assert out_lens.tolist() == counts and sp.plan.cpu().tolist() == [[pct if n else 100, c] for n, c in zip(lens, counts)]
        if B == 6:
            T = RS.TILE_OUT
            assert counts == [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
        y64, a64, _ = R.speed_ref(x, ln, sp.plan.cpu(), y.shape[1], return_abs=True)
        check_bound(y, y64, a64, sp.plan.cpu())
        check_tail(y, out_lens)
        for b in range(B):
            if lens[b] > 0:
                yr, _ = rs(xd[b:b + 1], ln[b:b + 1])
                assert torch.equal(y[b, :counts[b]].view(torch.int32), yr[0, :counts[b]].view(torch.int32))


def test_lens_none_means_whole_rows(cuda):
    r = run(cuda, torch.float32)
    x = r["x"].to(cuda)
    sp = SP.SpeedPerturb(POL, r["seed"])
    y, out_lens = sp(x, None, r["step"], first_utt=2)
    y2, l2 = sp(x, torch.full((len(LENS),), S, dtype=torch.int32, device=cuda), r["step"], first_utt=2)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(out_lens, l2)
    assert out_lens.tolist() == [R.speed_out_len(S, p) for p in sp.plan[:, 0].tolist()]
    y64, a64, _ = R.speed_ref(r["x"], None, sp.plan.cpu(), y.shape[1], return_abs=True)
    check_bound(y, y64, a64, sp.plan.cpu())


def test_int16_equals_the_fp32_of_the_same_samples(cuda):
    r = run(cuda, torch.int16)
    sp = SP.SpeedPerturb(POL, r["seed"])
    xf = planted(r["x"].to(torch.float32), LENS).to(cuda)
    y, out_lens = sp(xf, r["lens"].to(cuda), r["step"], first_utt=2, min_out=torch.tensor(MIN_OUT, dtype=torch.int32))
    assert torch.equal(y.cpu().view(torch.int32), r["y"].view(torch.int32)) and torch.equal(out_lens.cpu(), r["out_lens"])


def test_a_row_does_not_depend_on_the_batch_the_row_or_the_width(cuda):
    r = run(cuda, torch.float32)
    sp = SP.SpeedPerturb(POL, r["seed"])
    tight = sp.tight_width(r["lens"], len(LENS), S, r["step"], 2, MIN_OUT)
    assert tight == R.speed_round_width(int(r["out_lens"].max())) < r["y"].shape[1]
    yt, lt = sp(r["xd"], r["lens"].to(cuda), r["step"], first_utt=2, min_out=torch.tensor(MIN_OUT, dtype=torch.int32),
                out_width=tight)
    assert torch.equal(lt.cpu(), r["out_lens"]) and torch.equal(yt.cpu().view(torch.int32), r["y"][:, :tight].view(torch.int32))
    assert not r["y"][:, tight:].any()
    for b in range(len(LENS)):
        n_out = int(r["out_lens"][b])
        alone, la = sp(r["xd"][b:b + 1].clone(), r["lens"][b:b + 1].to(cuda), r["step"], first_utt=2 + b,
                       min_out=torch.tensor(MIN_OUT[b:b + 1], dtype=torch.int32))
        assert la.tolist() == [n_out] and torch.equal(sp.plan.cpu()[0], r["plan"][b])
        assert torch.equal(alone[0].cpu().view(torch.int32), r["y"][b].view(torch.int32))   # valid columns and zeros
        # row 2 of another batch, behind rows of other content and lengths
        other = torch.stack([r["xd"][(b + 1) % 6], r["xd"][(b + 2) % 6], r["xd"][b]])
        ol = torch.tensor([LENS[(b + 1) % 6], 7, LENS[b]], dtype=torch.int32)
        moved, lm = sp(other, ol.to(cuda), r["step"], first_utt=b, min_out=torch.tensor([0, 0, MIN_OUT[b]], dtype=torch.int32))
        assert int(lm[2]) == n_out and torch.equal(moved[2].cpu().view(torch.int32), r["y"][b].view(torch.int32))


def test_odd_width_rows_take_the_scalar_staging(cuda):
    """S = 2399: rows 1, 3 and 5 of a contiguous buffer are not 16-byte aligned; every row still
    equals the resampling kernel on that row alone, and the oracle's bound holds."""
    r = run(cuda, torch.float32)
    S1 = S - 1
    lens = [min(n, S1) for n in LENS]
    x = r["x"][:, :S1].contiguous()
    xd, ln = planted(x, lens).to(cuda), torch.tensor(lens, dtype=torch.int32)
    assert SP.kernels_cover(xd)
    sp = SP.SpeedPerturb(POL, r["seed"])
    y, out_lens = sp(xd, ln.to(cuda), r["step"], first_utt=2)
    plan = sp.plan.cpu()
    assert torch.equal(plan, R.speed_plan_ref(lens, len(lens), S1, POL, r["seed"], r["step"], first_utt=2))
    y64, a64, n64 = R.speed_ref(x, ln, plan, y.shape[1], return_abs=True)
    assert out_lens.tolist() == n64.tolist()
    check_bound(y, y64, a64, plan)
    check_tail(y, out_lens)
    for b, (pct, n_out) in enumerate(plan.tolist()):
        if pct == 100:
            assert torch.equal(y[b, :n_out].cpu().view(torch.int32), x[b, :n_out].view(torch.int32))
        else:
            yr, _ = RS.Resampler(pct, 100, device=cuda)(xd[b:b + 1].clone(), ln[b:b + 1])
            assert torch.equal(y[b, :n_out].view(torch.int32), yr[0, :n_out].view(torch.int32))


def test_other_layouts_take_the_composite(cuda):
    r = run(cuda, torch.float32)
    B = len(LENS)
    xp = planted(r["x"], LENS)
    flat = torch.empty(B * S + 1, device=cuda)
    misaligned = flat[1:].view(B, S)
    misaligned.copy_(xp)
    wide = torch.empty(B, S + 8, device=cuda)
    wide[:, :S] = xp.to(cuda)
    views = {"misaligned": misaligned, "fp64": xp.to(cuda).double(), "strided": wide[:, :S]}
    assert views["misaligned"].is_contiguous() and not views["strided"].is_contiguous()
    sp = SP.SpeedPerturb(POL, r["seed"])
    for name, v in views.items():
        assert not SP.kernels_cover(v), name
        y, out_lens = sp(v, r["lens"].to(cuda), r["step"], first_utt=2, min_out=torch.tensor(MIN_OUT, dtype=torch.int32))
        assert torch.equal(sp.plan.cpu(), r["want"]) and torch.equal(out_lens.cpu(), r["out_lens"]), name
        assert y.dtype == torch.float32 and y.shape == r["y"].shape
        check_bound(y, r["y64"], r["a64"], r["plan"], factor=2)
        check_tail(y, out_lens)
        ident = [b for b in range(B) if r["plan"][b, 0] == 100]
        assert torch.equal(y[ident].cpu().view(torch.int32), r["y"][ident].view(torch.int32))


def test_a_width_below_the_worst_case_needs_the_caller_s_word(cuda):
    from deepspeech_amd import _C
    x = torch.zeros(2, S, device=cuda)
    plan = torch.tensor([[100, S], [100, S]], dtype=torch.int32, device=cuda)
    out_lens = torch.empty(2, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="speed.apply.*worst case"):
        _C.speed.apply(x, None, plan, POL.table.to(cuda), POL.vtab, torch.empty(2, S, device=cuda), out_lens, False)
    y = torch.full((2, S), 7.0, device=cuda)
    _C.speed.apply(x, None, plan, POL.table.to(cuda), POL.vtab, y, out_lens, True)
    assert not y.any() and out_lens.tolist() == [S, S]
    # a count beyond the width the caller vouched for stops at the width
    plan[0, 1] = 5000
    y = torch.full((2, 1600), 7.0, device=cuda)
    _C.speed.apply(x, None, plan, POL.table.to(cuda), POL.vtab, y, out_lens, True)
    assert not y.any() and out_lens.tolist() == [1600, 1600]


# -------------------------------------------------------------------------------- the front end
def _audio_batch(cuda, N, frames, seed, keep):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    src = FixedShapeBatches(N, frames, seed=seed, pool=2, audio=True)

    def nxt():
        hb = src.next()
        hb.labels[:, keep:] = -1            # short labels: the CTC floor leaves room to speed up
        hb.label_lens[:] = np.minimum(hb.label_lens, keep)
        return hb, to_device(hb, cuda)
    return nxt


def test_front_end_equals_the_three_ops_one_by_one(cuda):
    from deepspeech_amd.data import audio_batch as AB
    from deepspeech_amd.ops import waveaug as WA
    from deepspeech_amd.ops.featurize import AudioFeaturizer
    hb, b = _audio_batch(cuda, 4, 60, 1, 2)()
    N, Rr, _ = b["feats"].shape
    pcm, lens = b["feats"].reshape(N, Rr * 160), (b["seq_lens"] * 160).to(torch.int32)
    min_out = AB.ctc_min_samples(b["labels"], b["label_lens"], "mfcc")
    step = next(s for s in range(100) if set(R.speed_plan_ref(lens.cpu(), N, Rr * 160, POL, 3, s, 4, min_out.cpu())[:, 0]
                                             .tolist()) == set(POL.pcts))
    bank = WA.NoiseBank.synthetic(0)
    sp, aug = SP.SpeedPerturb(POL, 3), WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=10:10"), bank, 3)
    front = AB.AudioFrontEnd("mfcc", cuda, wave_aug=aug, speed=sp, max_frames=1800)
    out = front(b, step=step, first_utt=4, training=True, host=hb)
    assert set(sp.plan[:, 0].tolist()) == set(POL.pcts)
    sp2, aug2 = SP.SpeedPerturb(POL, 3), WA.WaveAugment(aug.policy, bank, 3)
    tight = sp2.tight_width(lens.cpu(), N, Rr * 160, step, 4, min_out.cpu(), front.max_out)
    y, n_out = sp2(pcm, lens, step, first_utt=4, min_out=min_out, max_out=front.max_out, out_width=tight)
    assert tight <= SP.speed_out_width(Rr * 160, POL) and tight - 160 < int(n_out.max()) <= tight
    noisy = aug2(y, n_out, step, first_utt=4)
    feats, frames = AudioFeaturizer("mfcc", device=cuda, normalize="utterance")(noisy, n_out)
    assert torch.equal(out["feats"], feats) and torch.equal(out["seq_lens"], frames)
    assert torch.equal(sp.plan, sp2.plan) and torch.equal(aug.plan, aug2.plan)
    # without the host batch: the worst-case width, the same frames and more padding
    wide = front(b, step=step, first_utt=4, training=True)
    T = feats.shape[1]
    assert wide["feats"].shape[1] >= T and torch.equal(wide["feats"][:, :T], feats) and not wide["feats"][:, T:].any()
    assert torch.equal(wide["seq_lens"], frames)
    plain = AB.AudioFrontEnd("mfcc", cuda)(b)
    assert torch.equal(front(b, step=step, first_utt=4)["feats"], plain["feats"])           # not training


def _six_steps(cuda):
    from deepspeech_amd import config as C
    from deepspeech_amd import train as TR
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.trainer import LRSchedule, Trainer
    torch.manual_seed(0)
    model = DeepSpeech2(num_filters=32, num_hidden=256, num_rnn_layers=2, cell="gru").to(cuda)
    model.set_engine("hip", torch.bfloat16)
    tr = Trainer(model, LRSchedule(1e-4, 1000, 0.9))
    args = C.build_train_parser().parse_args(["--dummy", "True", "--dummy_audio", "True", "--speed_perturb", "0.9,1.0,1.1",
                                              "--seed", "1234"])
    front = TR.build_front_end(args, None, cuda, False)
    nxt = _audio_batch(cuda, 8, 120, 0, 6)
    losses, plans = [], []
    for step in range(6):
        hb, b = nxt()
        batch = front(b, step, first_utt=0, training=True, host=hb)
        losses.append(tr.step(batch).detach().clone())
        plans.append(front.speed.plan.cpu())
    tr.flush()
    torch.cuda.synchronize()
    RNN.check_errors()
    return torch.stack([l.reshape(()) for l in losses]).cpu(), plans


def test_training_from_dummy_audio_is_finite_and_repeatable(cuda):
    a, plans = _six_steps(cuda)
    b, _ = _six_steps(cuda)
    print("losses", a.tolist())
    assert bool(torch.isfinite(a).all()) and bool((a > 0).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert set(torch.cat(plans)[:, 0].tolist()) == set(POL.pcts) and not torch.equal(plans[0], plans[1])
