"""Model-level semantics of the reference graph (CPU, engine=ref)."""
import math
import os

import numpy as np
import pytest
import torch

from deepspeech_amd import NUM_CLASSES
from deepspeech_amd.config import get_rnn_seqlen_py
from deepspeech_amd.models import DeepSpeech2, conv_out_len, freq_out
from deepspeech_amd.ops import reference as R


def test_get_rnn_seqlen_matches_conv_output():
    # T2 = ceil((ceil((T-19)/2)-9)/2) equals the VALID conv output length
    for T in [39, 40, 100, 101, 999, 1000, 1500, 1800]:
        t1, t2 = conv_out_len(T)
        assert int(R.get_rnn_seqlen(torch.tensor([T]))[0]) == t2 == get_rnn_seqlen_py(T)
    assert conv_out_len(1000) == (491, 241)
    assert conv_out_len(1500) == (741, 366)
    assert freq_out(161) == (79, 75)


@pytest.mark.parametrize("cell", ["rnn_relu", "gru"])
def test_forward_shapes(cell):
    m = DeepSpeech2(num_filters=4, num_hidden=16, num_rnn_layers=3, cell=cell)
    x = torch.randn(3, 120, 161)
    logits, lens = m(x, torch.tensor([120, 100, 80], dtype=torch.int32))
    assert logits.shape == (conv_out_len(120)[1], 3, NUM_CLASSES)
    assert lens.tolist() == [get_rnn_seqlen_py(t) for t in (120, 100, 80)]


def test_param_shapes_follow_reference():
    m = DeepSpeech2(num_filters=32, num_hidden=64, num_rnn_layers=2, cell="rnn_relu")
    assert tuple(m.conv1.weight.shape) == (32, 1, 20, 5)
    assert tuple(m.conv2.weight.shape) == (32, 32, 10, 5)
    assert torch.allclose(m.conv1.bias, torch.full((32,), -0.05))
    assert tuple(m.rnn[0].fw.W.shape) == (64, 2400)      # W [H, 75*C]
    assert tuple(m.rnn[1].fw.W.shape) == (64, 64)        # correctly stacked (Q1 fix)
    assert tuple(m.fc_weight.shape) == (NUM_CLASSES, 64)
    # quirk Q1 reproduction: every layer consumes the conv output
    q = DeepSpeech2(num_filters=32, num_hidden=64, num_rnn_layers=2, stack_fix=False)
    assert tuple(q.rnn[1].fw.W.shape) == (64, 2400)


def test_reverse_sequence_semantics():
    x = torch.arange(5).view(5, 1, 1).repeat(1, 2, 1).float()
    y = R.reverse_sequence(x, torch.tensor([3, 5]))
    assert y[:, 0, 0].tolist() == [2, 1, 0, 3, 4]       # reversed within length, tail kept
    assert y[:, 1, 0].tolist() == [4, 3, 2, 1, 0]


def test_outputs_zero_past_length_and_bw_direction():
    torch.manual_seed(0)
    T, N, H = 6, 2, 4
    gx = torch.randn(T, N, H)
    U = torch.randn(H, H) * 0.3
    lens = torch.tensor([4, 6])
    y, _ = R.rnn_relu_scan(gx, U, lens)
    assert float(y[4:, 0].abs().sum()) == 0.0
    # bw direction of a length-4 utterance == fw scan of its time-reversed prefix
    yb = R.birnn_ref("rnn_relu", torch.zeros_like(gx), gx, torch.zeros(H, H), U, None, None, lens)
    ref, _ = R.rnn_relu_scan(gx[:4, :1].flip(0), U, torch.tensor([4]))
    y_f0, _ = R.rnn_relu_scan(torch.zeros(T, N, H), torch.zeros(H, H), lens)
    assert torch.allclose(yb[:4, 0] - y_f0[:4, 0], ref.flip(0)[:, 0], atol=1e-6)


def test_clipped_relu_cap():
    x = torch.tensor([-1.0, 0.5, 25.0])
    assert R.clipped_relu(x).tolist() == [0.0, 0.5, 20.0]


def test_frozen_seq_bn_is_constant_scale():
    y = torch.randn(5, 3, 7)
    out = R.seq_batch_norm(y, torch.tensor([5, 5, 5]), "frozen", torch.zeros(7), torch.ones(7))
    assert torch.allclose(out, y / math.sqrt(1 + 1e-5))


def test_batch_seq_bn_uses_valid_positions_only():
    y = torch.randn(4, 2, 3)
    lens = torch.tensor([4, 2])
    y[2:, 1] = 1000.0            # padding garbage must not affect the statistics
    out = R.seq_batch_norm(y, lens, "batch", torch.zeros(3), torch.ones(3), training=True)
    valid = torch.cat([y[:, 0], y[:2, 1]], 0)
    ref = (valid - valid.mean(0)) / torch.sqrt(valid.var(0, unbiased=False) + 1e-5)
    assert torch.allclose(torch.cat([out[:, 0], out[:2, 1]], 0), ref, atol=1e-5)


def test_gru_matches_torch_gru_cell():
    torch.manual_seed(0)
    H, I, N, T = 8, 5, 3, 4
    cell = torch.nn.GRUCell(I, H)
    x = torch.randn(T, N, I)
    gx = x @ cell.weight_ih.t() + cell.bias_ih
    y, _ = R.gru_scan(gx, cell.weight_hh, cell.bias_hh, torch.tensor([T] * N))
    h = torch.zeros(N, H)
    for t in range(T):
        h = cell(x[t], h)
    assert torch.allclose(y[-1], h, atol=1e-5)


def test_ctc_ref_mean_over_batch_not_normalised_by_label_length():
    torch.manual_seed(0)
    logits = torch.randn(20, 2, NUM_CLASSES)
    labels = torch.tensor([[1, 2, 3], [4, 5, 0]], dtype=torch.int32)
    per = R.ctc_loss_ref(logits, labels, torch.tensor([20, 15]), torch.tensor([3, 2]))
    m = DeepSpeech2(num_filters=4, num_hidden=8, num_rnn_layers=1)
    mean = m.loss(logits, torch.tensor([20, 15], dtype=torch.int32), labels, torch.tensor([3, 2]))
    assert torch.allclose(mean, per.mean())


@pytest.mark.parametrize("cell", ["rnn_relu", "gru"])
def test_overfits_one_batch(cell):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.trainer import LRSchedule, Trainer
    torch.manual_seed(0)
    m = DeepSpeech2(num_filters=4, num_hidden=32, num_rnn_layers=1, cell=cell)
    tr = Trainer(m, LRSchedule(3e-3, 10 ** 6, 0.9), moving_avg_decay=0.9999)
    b = to_device(FixedShapeBatches(2, max_frames=160, seed=0, pool=1, chars_per_sec=5).next(), torch.device("cpu"))
    first = float(tr.step(b))
    for _ in range(25):
        last = float(tr.step(b))
    assert last < first * 0.8, (first, last)


def test_flops_positive_and_gru_heavier():
    a = DeepSpeech2(num_filters=32, num_hidden=800, num_rnn_layers=5, cell="gru").flops_per_step(32, 1000)
    b = DeepSpeech2(num_filters=32, num_hidden=800, num_rnn_layers=5, cell="rnn_relu").flops_per_step(32, 1000)
    assert a > b > 0


def test_weight_gradient_scheduling_is_per_arena():
    """Two models / trainers in one process keep their own weight-gradient scheduling
    (side stream, deferral switch, pending queues): VERDICT r1 weak item 12."""
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.ops.optim import ParamArena
    a = ParamArena(DeepSpeech2(num_filters=4, num_hidden=32, num_rnn_layers=1))
    b = ParamArena(DeepSpeech2(num_filters=4, num_hidden=32, num_rnn_layers=1))
    assert a.wgrad is not b.wgrad
    a.wgrad.set_deferral(True)
    b.wgrad.set_deferral(False)        # e.g. a data-parallel trainer created second
    assert a.wgrad.defer_input and not b.wgrad.defer_input
    ran = []
    a.wgrad.deferred.append(lambda: ran.append("a"))
    assert RNN.pending_deferred(a) == 1 and RNN.pending_deferred(b) == 0
    b.wgrad.discard()                  # b's step start must not drop a's pending work
    assert RNN.pending_deferred(a) == 1
    a.wgrad.flush()
    assert ran == ["a"] and RNN.pending_deferred(a) == 0
    assert RNN.wgrad_stream(torch.device("cpu"), a) is None      # no side stream off-GPU


def test_xcd_plans_for_wide_and_deferral_rule():
    """Plan geometry of the XCD recurrence kernels (no GPU needed): one-gate layers wider than
    an XCD at 32 units per workgroup get 64-unit workgroups (ceil(H/64) per group, 8 groups of
    <= 8 rows on one XCD each); the weight gradients of a layer are deferred to the grouped tail
    launch only when its BPTT leaves fewer than 96 CUs idle."""
    from deepspeech_amd.ops import rnn as RNN
    p = RNN.make_xcd_plan(32, 1760, "rnn_relu", 2, 256)
    assert p is not None and p.kind == "xcd" and (p.BG, p.R, p.NP, p.xcd_map) == (4, 8, 32, 1)
    C, relu, gru = RNN._ext.ext(), RNN.CELL_CODE["rnn_relu"], RNN.CELL_CODE["gru"]
    assert C.rnnx_members(1760, relu) == 28 and RNN._bptt_cus(p) == 224
    assert RNN.make_xcd_plan(64, 1760, "rnn_relu", 2, 256) is None          # R = 16 > 8
    assert C.rnnx_fwd_family(1760, gru, 0) != 6 and C.rnnx_fwd_family(1024, relu, 0) != 6
    assert C.rnnx_fwd_family(1056, relu, 0) == 6 and C.rnnx_fwd_family(1824, relu, 0) != 6
    head = RNN.make_xcd_plan(32, 800, "gru", 2, 256)                        # headline: 200 CUs
    c5 = RNN.make_xcd_plan(32, 1280, "gru", 2, 256)                         # config 5: 160 CUs
    assert RNN._bptt_cus(head) == 200 and RNN._bptt_cus(c5) == 160
    assert 256 - RNN._bptt_cus(head) < RNN._BESIDE_MIN_IDLE_CUS <= 256 - RNN._bptt_cus(c5)


def test_partial_deferral_rule(monkeypatch):
    """Which layers' weight gradients join the grouped tail launch (no GPU: the host rule of
    ops/rnn.py _defer_layers). Headline (56 idle CUs): only layer 0's, and only for sequences of
    >= _PARTIAL_MIN_T recurrence steps (the 10-s batch has 241); shorter buckets defer every
    layer's. ReLU-1760 (32 idle CUs) defers everything; config 5 (96 idle) defers nothing."""
    from deepspeech_amd.ops import rnn as RNN
    monkeypatch.setenv("DS2_NUM_CUS", "256")
    monkeypatch.setattr(RNN, "_DEFER_LAYERS", -1)
    cuda = torch.device("cuda", 0)
    head = RNN.make_xcd_plan(32, 800, "gru", 2, 256)
    relu = RNN.make_xcd_plan(32, 1760, "rnn_relu", 2, 256)
    c5 = RNN.make_xcd_plan(32, 1280, "gru", 2, 256)
    assert RNN._PARTIAL_MIN_T <= 241
    assert RNN._defer_wgrad(head, cuda) and RNN._defer_layers(head, cuda, 241) == 1
    assert [RNN._defer_layer(head, cuda, i, 241) for i in range(5)] == [True] + [False] * 4
    assert RNN._upper_trigger(head, cuda, 241) == 1
    short = RNN._PARTIAL_MIN_T - 1
    assert all(RNN._defer_layer(head, cuda, i, short) for i in range(5))
    assert RNN._upper_trigger(head, cuda, short) >= 5
    assert all(RNN._defer_layer(relu, cuda, i, 241) for i in range(7))
    assert not RNN._defer_wgrad(c5, cuda) and RNN._upper_trigger(c5, cuda, 241) == 1
    assert not any(RNN._defer_layer(c5, cuda, i, 241) for i in range(7))
    assert RNN._defer_layers(head, torch.device("cpu"), 241) >= 5          # CPU: all deferred


def test_recurrence_kernel_family_map():
    """Which kernel family every bf16 plan launches (no GPU: the host dispatch functions of
    csrc/rnn_xcd.hip that the launches branch on). Every family on this map is reachable by a
    geometry someone can configure, and tests/test_engine_gpu.py runs each one at T = 241 and
    batch 32 against the fp32 reference."""
    from deepspeech_amd.ops import rnn as RNN
    want = {("gru", 800, "auto"): "rnne_fwd", ("gru", 256, "auto"): "rnne_fwd",
            ("gru", 1280, "auto"): "rnnq_fwd", ("rnn_relu", 800, "auto"): "rnnq_fwd",
            ("rnn_relu", 1760, "auto"): "rnnw_fwd", ("gru", 1056, "auto"): "rnnx_fwd",
            ("gru", 1344, "auto"): "rnnx_fwd", ("rnn_relu", 2048, "auto"): "rnn_fwd (gen 1, persistent)",
            ("gru", 800, "step"): "rnn_fwd (gen 1, step"}
    for (cell, H, mode), fam in want.items():
        fw, bw = RNN.kernel_families(RNN.make_plan(32, H, cell, 2, 256, mode))
        assert fw.startswith(fam), (cell, H, mode, fw)
        assert bw.startswith({"rnnw_fwd": "rnnw_bwd"}.get(fam, "rnn_bwd" if fam.startswith("rnn_fwd") else "rnnrs_bwd"))
    # the timing-only knob bits never reach the family choice, the selector bit 256 does
    p = RNN.make_plan(32, 800, "gru", 2, 256)
    assert int(RNN._ext.ext().rnnx_fwd_family(800, 1, 256)) == 2
    assert RNN.kernel_families(p)[0].startswith("rnne_fwd")


def test_xcd_plans_agree_with_the_extension():
    """make_xcd_plan builds its plans from what csrc/rnn_xcd.hip reports (rnnx_members,
    rnnx_fwd_family, rnnx_bwd_family): over both cells, 1 / 2 directions, 128 / 256 / 304 CUs,
    H = 32..2048 in steps of 32 and 12 batch sizes, every plan it returns is one the dispatch
    accepts, fits the chip with the grid the launch will use, and is wide exactly where the
    kernels use 64-unit groups (no GPU needed)."""
    from deepspeech_amd.ops import rnn as RNN
    C = RNN._ext.ext()
    plans = 0
    for cell, code in RNN.CELL_CODE.items():
        for H in range(32, 2049, 32):
            P = int(C.rnnx_members(H, code))
            for ndir in (1, 2):
                for cus in (128, 256, 304):
                    for N in (1, 2, 3, 5, 8, 12, 16, 24, 32, 48, 64, 128):
                        p = RNN.make_xcd_plan(N, H, cell, ndir, cus)
                        if p is None:
                            continue
                        plans += 1
                        fam = int(C.rnnx_fwd_family(H, code, RNN._kernel_knobs(p)))
                        assert fam != 0 and int(C.rnnx_bwd_family(H, code, p.R)) != 0, p
                        ngroups = ndir * p.BG
                        grid = int(C.rnnx_grid(H, code, ngroups, p.xcd_map))
                        assert grid == (8 * P if p.xcd_map and ngroups <= 8 else ngroups * P), p
                        assert 0 < grid <= cus, p
                        assert p.NP == p.BG * p.R >= N and p.mt == 1, p
                        assert (fam == 6) == (P == -(-H // 64) != H // 32), p
    assert plans > 5000


@pytest.mark.parametrize("name,N,H,cell,T,dp,fp8,want", [
    # headline 5 x BiGRU-800, batch 32, 10 s (T = 241): 200 CUs, layer 0 deferred, beside GEMMs on 40 of
    # the 56 idle CUs (5 per XCD), carried optimizer chunks on 56 blocks
    ("headline", 32, 800, "gru", 241, False, False,
     dict(bptt_cus=200, idle_cus=56, defer_wgrad=True, defer_layers=1, upper_trigger=1, beside_grid=40,
          carry_grid=56, group_cap=192)),
    # the short SortaGrad buckets (< 200 recurrence steps): every layer deferred
    ("headline-short", 32, 800, "gru", 116, False, False,
     dict(defer_wgrad=True, defer_layers=1 << 30, upper_trigger=1 << 30)),
    # data parallel: same plan, beside grids capped for the collectives' sake
    ("headline-dp", 32, 800, "gru", 241, True, False, dict(beside_grid=56)),
    # config 5, 7 x BiGRU-1280: 160 CUs, 96 idle: nothing deferred, bf16 beside GEMMs uncapped,
    # the fp8 BPTT's capped (10 of each XCD's 12 idle CUs on one device, all 12 with DP)
    ("config5-bf16", 32, 1280, "gru", 241, False, False,
     dict(bptt_cus=160, idle_cus=96, defer_wgrad=False, upper_trigger=1, beside_grid=0, carry_grid=96)),
    ("config5-fp8", 32, 1280, "gru", 241, False, True, dict(beside_grid=80)),
    ("config5-fp8-dp", 32, 1280, "gru", 241, True, True, dict(beside_grid=96)),
    # reference headline 7 x bi-ReLU-1760: 224 CUs, everything deferred (32 idle < 56)
    ("relu1760", 32, 1760, "rnn_relu", 241, False, False,
     dict(bptt_cus=224, idle_cus=32, defer_wgrad=True, defer_layers=1 << 30, beside_grid=32, carry_grid=32)),
])
def test_schedule_for_shipped_configs(name, N, H, cell, T, dp, fp8, want):
    """ops/rnn.py schedule_for: the one place every weight-gradient / optimizer placement
    threshold is decided, pinned for each shipped configuration on a
    256-CU MI355X (no GPU needed)."""
    from deepspeech_amd.ops import rnn as RNN
    plan = RNN.make_xcd_plan(N, H, cell, 2, 256)
    s = RNN.schedule_for(plan, T, dp, fp8, 256)
    for k, v in want.items():
        assert getattr(s, k) == v, (name, k, getattr(s, k), v)
    cpu = RNN.schedule_for(plan, T, dp, fp8, 0)
    assert cpu.defer_wgrad and cpu.defer_layers >= 5 and cpu.beside_grid == 0


def test_env_knobs_are_few():
    """A/B-only environment switches whose decision is recorded are gone;
    fewer than 20 distinct DS2_* variables are read anywhere in the package."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepspeech_amd")
    names = set()
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                names |= set(re.findall(r"DS2_[A-Z0-9_]+", open(os.path.join(d, f)).read()))
    assert len(names) < 20, sorted(names)


def test_recurrence_poll_timing_knob_defaults(monkeypatch):
    """The persistent recurrences' poll timing (ops/rnn.py POLL_DEFAULT: forward pre-poll sleep
    4, BPTT pre-gather sleep 4, profiles/r6_recurrence_poll.md) reaches every launch unless
    DS2_RNNX_KNOBS sets a poll-timing bit; bit 23 alone asks for no sleep at all."""
    from deepspeech_amd.ops import rnn as RNN
    monkeypatch.delenv("DS2_TIMING_ONLY", raising=False)
    monkeypatch.setattr(RNN, "RNNX_KNOBS", 0)
    assert RNN._kernel_knobs() == RNN.POLL_DEFAULT
    assert (RNN.POLL_DEFAULT >> 17) & 7 == 4 and (RNN.POLL_DEFAULT >> 20) & 7 == 4
    monkeypatch.setattr(RNN, "RNNX_KNOBS", 16384)
    assert RNN._kernel_knobs() == 16384 | RNN.POLL_DEFAULT
    monkeypatch.setattr(RNN, "RNNX_KNOBS", 6 << 17)
    assert RNN._kernel_knobs() == 6 << 17
    monkeypatch.setattr(RNN, "RNNX_KNOBS", RNN.POLL_EXPLICIT)
    assert RNN._kernel_knobs() & RNN.POLL_MASK == RNN.POLL_EXPLICIT
    monkeypatch.setattr(RNN, "RNNX_KNOBS", 1 << 24)          # stamp-wave selection: not a poll bit
    assert RNN._kernel_knobs() == (1 << 24) | RNN.POLL_DEFAULT
    # GRU wider than 1024 (config 5 bf16, cross-XCD groups): the wide poll timing
    from types import SimpleNamespace
    monkeypatch.setattr(RNN, "RNNX_KNOBS", 0)
    assert RNN._kernel_knobs(SimpleNamespace(cell="gru", H=1280)) == RNN.POLL_WIDE
    assert RNN._kernel_knobs(SimpleNamespace(cell="gru", H=800)) == RNN.POLL_DEFAULT
    assert RNN._kernel_knobs(SimpleNamespace(cell="rnn_relu", H=1760)) == RNN.POLL_RELU
