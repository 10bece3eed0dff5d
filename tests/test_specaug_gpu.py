"""SpecAugment kernels (csrc/specaug.hip) against the oracle of tests/specaug_cases.py, per
element on every grid case, and one Trainer step on an augmented batch."""
import copy

import pytest
import torch

import specaug_cases as SC
from deepspeech_amd.ops import reference as R

pytestmark = pytest.mark.gpu

_dev = {}


def on_device(idx, cuda):
    """(x, lens, kernel plan, kernel mean, fill, kernel output) of grid case idx, computed once."""
    if idx not in _dev:
        from deepspeech_amd.ops import specaug as SA
        c = SC.CASES[idx]
        x, lens = SC.inputs(idx)
        xd, ld = x.to(cuda), lens.to(cuda)
        assert SA.kernels_cover(xd)
        pol = SA.SpecAugPolicy(nF=c.nF, Fw=c.Fw, nT=c.nT, Tw=c.Tw, p_ppm=c.p_ppm, W=c.W, fill=c.fill)
        plan = SA.specaug_plan(ld, c.T, c.F, pol, c.seed, c.step, c.first_utt)
        mean = SA.specaug_mean(xd, ld)
        fill = mean if c.fill == "mean" else None
        out = SA.specaug_apply(xd, ld, plan, fill, c.nF)
        _dev[idx] = (xd, ld, plan, mean, fill, out)
    return _dev[idx]


@pytest.mark.parametrize("idx", range(len(SC.CASES)), ids=SC.IDS)
def test_plan_kernel_equals_oracle(cuda, idx):
    plan = on_device(idx, cuda)[2]
    assert plan.dtype == torch.int32 and torch.equal(plan.cpu(), SC.oracle_plan(idx))


@pytest.mark.parametrize("idx", range(len(SC.CASES)), ids=SC.IDS)
def test_mean_kernel(cuda, idx):
    x, lens = SC.inputs(idx)
    SC.check_mean(on_device(idx, cuda)[3], x, lens)


def test_mean_is_bitwise_independent_of_the_batch(cuda):
    from deepspeech_amd.ops import specaug as SA
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(33, 130, 161, generator=g) * 2 + 0.5).to(cuda)
    lens = torch.randint(0, 134, (33,), generator=g, dtype=torch.int32).to(cuda)
    whole = SA.specaug_mean(x, lens)
    for u in range(33):
        alone = SA.specaug_mean(x[u:u + 1].contiguous(), lens[u:u + 1].contiguous())
        assert torch.equal(SC.bits(alone), SC.bits(whole[u:u + 1])), u


@pytest.mark.parametrize("idx", range(len(SC.CASES)), ids=SC.IDS)
def test_apply_kernel(cuda, idx):
    """Given the kernel's own plan and mean: noise (with data in the padding), a ramp x = t (the
    output is the source position) and a time-constant input (any warp is the bitwise identity);
    frames >= L are bit copies; a second call gives the same bits."""
    from deepspeech_amd.ops import specaug as SA
    c = SC.CASES[idx]
    x, lens = SC.inputs(idx)
    xd, ld, plan, _, fill, out = on_device(idx, cuda)
    print("APPLY", c.id, SC.check_apply(out, x, lens, plan, fill, c.nF))
    pad = torch.arange(c.T)[None, :] >= lens.long().clamp(0, c.T)[:, None]
    assert bool((x[pad] != 0).all()) and torch.equal(SC.bits(out.cpu())[pad], SC.bits(x)[pad])
    assert torch.equal(SC.bits(SA.specaug_apply(xd, ld, plan, fill, c.nF)), SC.bits(out))
    assert torch.equal(xd.cpu(), x)                                        # the input is left alone

    rp = SC.ramp(c)
    rd = rp.to(cuda)
    rfill = SA.specaug_mean(rd, ld) if c.fill == "mean" else None
    SC.check_apply(SA.specaug_apply(rd, ld, plan, rfill, c.nF), rp, lens, plan, rfill, c.nF)

    tc = SC.time_constant(c)
    got = SA.specaug_apply(tc.to(cuda), ld, plan, None, c.nF).cpu()
    tm, fm = R.specaug_masks(lens, plan.cpu(), c.T, c.F, c.nF)
    free = ~(tm[:, :, None] | fm[:, None, :])
    assert torch.equal(SC.bits(got)[free], SC.bits(tc)[free])
    assert bool((got[~free & ~pad[:, :, None]] == 0).all())


W0 = [i for i, c in enumerate(SC.CASES) if c.W == 0 and c.nF + c.nT > 0]


@pytest.mark.parametrize("idx", W0, ids=[SC.IDS[i] for i in W0])
def test_masked_cells_hold_the_fill_and_inplace_equals_out_of_place(cuda, idx):
    """+-inf and NaN under the masks (the fill is that of the clean input): masked cells hold
    exactly the fill, every other cell its input bits; in place gives the same bits."""
    from deepspeech_amd.ops import specaug as SA
    c = SC.CASES[idx]
    x, lens = SC.inputs(idx)
    _, ld, plan, _, fill, _ = on_device(idx, cuda)
    tm, fm = R.specaug_masks(lens, plan.cpu(), c.T, c.F, c.nF)
    valid = torch.arange(c.T)[None, :] < lens.long().clamp(0, c.T)[:, None]
    masked = (tm[:, :, None] | fm[:, None, :]) & valid[:, :, None]
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(x.numel()) % 3].view_as(x)
    xp = torch.where(masked, poison, x)
    xd = xp.to(cuda)
    out = SA.specaug_apply(xd, ld, plan, fill, c.nF)
    want = torch.where(masked, (torch.zeros(c.B, c.F) if fill is None else fill.cpu())[:, None, :].expand_as(x), x)
    assert torch.equal(SC.bits(out.cpu()), SC.bits(want))
    y = xd.clone()
    assert SA.specaug_apply(y, ld, plan, fill, c.nF, inplace=True) is y
    assert torch.equal(SC.bits(y), SC.bits(out))


def test_out_of_contract_inputs_take_the_composite(cuda):
    from deepspeech_amd.ops import specaug as SA
    g = torch.Generator().manual_seed(4)
    lens = torch.tensor([67, 40, 0, 13, 70], dtype=torch.int32)
    ld = lens.to(cuda)
    wide = torch.randn(5, 67, 64, generator=g)
    x = wide[:, :, ::2]                                             # non-contiguous fp32
    xd = wide.to(cuda)[:, :, ::2]
    assert not SA.kernels_cover(xd) and not SA.kernels_cover(wide.to(cuda).bfloat16())
    for spec in ("W=5,F=9,nF=2,T=20,nT=2,fill=zero", "W=5,F=9,nF=2,T=20,nT=2,fill=mean"):
        pol = SA.SpecAugPolicy.parse(spec)
        out, plan = SA.SpecAugment(pol, 11)(xd, ld, 3, return_plan=True)
        assert torch.equal(plan.cpu(), R.specaug_plan_ref(lens, 67, 32, pol, 11, 3))
        fill = None
        if pol.fill == "mean":
            fill = SA.specaug_mean(xd, ld)
            SC.check_mean(fill, x.contiguous(), lens)
        SC.check_apply(out, x.contiguous(), lens, plan, fill, pol.nF)
    pol = SA.SpecAugPolicy.parse("W=5,F=9,nF=2,T=20,nT=2,fill=zero")
    xb = wide.bfloat16()
    out = SA.SpecAugment(pol, 11)(xb.to(cuda), ld, 3)
    assert out.dtype == torch.bfloat16
    want = R.specaug_apply_ref(xb, lens, R.specaug_plan_ref(lens, 67, 64, pol, 11, 3), None, pol.nF)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_no_host_synchronisation(cuda):
    from deepspeech_amd.ops import specaug as SA
    x = torch.randn(4, 130, 161, device=cuda)
    lens = torch.tensor([130, 99, 0, 7], dtype=torch.int32, device=cuda)
    augs = [SA.SpecAugment(SA.SpecAugPolicy.parse(s), 1234) for s in ("ls", "F=27,nF=2,T=40,nT=2,fill=zero")]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = augs[0](x, lens, 5)
        b = augs[1](x, lens, 5, inplace=False)
        y = x.clone()
        augs[1](y, lens, 5, inplace=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(y, b) and not torch.equal(a, x)


@pytest.mark.parametrize("kw", [dict(), dict(step_graphs=True, graph_warmup=1)], ids=["eager", "step-graphs"])
def test_trainer_steps_on_augmented_batches(cuda, kw):
    """Three Trainer steps of a tiny HIP model on batches augmented by the kernels (W = 0): the
    losses are bitwise those of the same trainer state fed the oracle-augmented tensors."""
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.ops import specaug as SA
    from deepspeech_amd.trainer import LRSchedule, Trainer
    torch.manual_seed(21)
    m0 = DeepSpeech2(num_filters=32, num_hidden=128, num_rnn_layers=2, cell="gru", bidirectional=False).to(cuda)
    m1 = copy.deepcopy(m0)
    feed = FixedShapeBatches(6, max_frames=260, seed=3, pool=3)
    host = [feed.next() for _ in range(3)]
    aug = SA.SpecAugment(SA.SpecAugPolicy.parse("F=27,nF=2,T=40,nT=2,p=1.0"), 1234)
    losses = []
    for m, oracle in ((m0, False), (m1, True)):
        tr = Trainer(m.set_engine("hip", torch.bfloat16), LRSchedule(1e-3, 2, 0.5), **kw)
        run = []
        for step, hb in enumerate(host):
            b = to_device(hb, cuda)
            feats, plan = aug(b["feats"], b["seq_lens"], step, return_plan=True)
            if oracle:
                x, lens = torch.from_numpy(hb.feats), torch.from_numpy(hb.seq_lens)
                assert torch.equal(plan.cpu(), R.specaug_plan_ref(lens, x.shape[1], x.shape[2], aug.policy, 1234, step))
                want = R.specaug_apply_ref(x, lens, plan.cpu(), SA.specaug_mean(b["feats"], b["seq_lens"]).cpu(), 2)
                assert not torch.equal(want, x)
                feats = want.to(cuda)
            run.append(float(tr.step(dict(b, feats=feats))))
        tr.flush()
        torch.cuda.synchronize()
        losses.append(run)
    assert losses[0] == losses[1] and all(l == l for l in losses[0]), losses
