"""Every tensor slot of every tensor-taking binding refuses a wrong dtype and a tensor one element
short, before anything is launched (csrc/bind_args.h).

A proxy for ``_ext.ext()`` records every call as (name, args) and then really launches it, while a
handful of tiny scenarios run through the public ``ops`` wrappers. Afterwards each recorded call
is repeated with one tensor slot replaced at a time: by zeros of float64 in the same shape (at
least as many bytes, on the same device, all-zero bits: were a check missing, a kernel would read
zeros as lengths, labels and indices and never form an out-of-range index), and by
``good.flatten()[:-1]`` (a view of the full allocation: nothing can be overrun). Each must raise a
RuntimeError that names the op, and leave every tensor of the call bit-identical."""
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32

# Slots whose helper call says "or more" (at_least in csrc/bindings.cpp), by positional index,
# each with the comment of the binding that makes it so. Exempt from the one-element-short case.
OR_MORE = {
    # "bf16 [T, N, row] ... (or more: the projection's output may be the larger buffer of a longer
    # batch)"; "saved state of the forward ... or more (a longer launch's buffers)"; flags / census
    # / err are word buffers shared between launches
    "rnn_fwd": {4: "gx", 11: "hx", 12: "hs", 13: "gates", 14: "flags", 15: "err"},
    "rnn_bwd": {4: "dy", 8: "hs", 9: "gates", 11: "dgx", 15: "flags", 16: "err"},
    "rnnx_fwd": {1: "gx", 8: "ysum", 9: "hx", 10: "hs", 11: "gates", 12: "census", 13: "err"},
    # "dgh is a plain output (or more: the exchange of a longer launch), ... ring [ndir, ds2_rnnx_ring_floats or more]"
    "rnnx_bwd": {1: "dy", 5: "hs", 6: "gates", 7: "dgh", 8: "dgx", 11: "census", 12: "err", 13: "ring"},
    # "uexp = E8M0 exponent per direction on the device, int32 [ndir or more]"
    "rnnf8_fwd": {1: "gx", 4: "uexp", 12: "census", 13: "err"},
    # "ring [ndir, ring_words or more]"
    "rnnf8_bwd": {4: "uexp", 5: "hs", 6: "gates", 11: "census", 12: "err", 13: "ring"},
    # "uexp / amax int32 [1 or more]"
    "fp8_quant_pow2": {2: "uexp", 3: "amax"}, "fp8_quant_pow2_t": {2: "uexp", 3: "amax"},
    # "uexp int32 [ndir or more], part fp32 [ndir * 256 or more] scratch"
    "fp8_quant_u": {4: "uexp", 5: "part"},
    # "ws fp32 [ctc_ws_floats or more]"; "ws uint8 [ctc_align_ws_bytes or more]"
    "ctc_fused": {6: "ws"}, "ctc_align": {9: "ws"}, "head_ctc": {8: "ws"},
    # "hyper fp32 {lr_t, ema_keep} [2 or more]"; "fp32 [ds2_clip_state_words() or more]"; skip is a flag word
    "adam_ema": {12: "skip", 14: "hyper", 16: "clip"}, "adam_ema_ranges": {13: "hyper", 14: "clip"},
    # "part fp32 [1 or more]: as many block partials as it has elements"
    "grad_norm": {2: "part"}, "clip_finalize": {2: "state"},
    # "part buffers are fp32 workspaces of the stated size or more"; "optional int64 [8 * 16 * 6 or more]"
    "conv1_fwd": {4: "part"}, "conv2_fwd": {4: "part", 6: "trace"}, "conv2_dgrad": {9: "part", 10: "trace"},
    "conv2_wgrad": {2: "part"}, "conv1_wgrad": {2: "part"}, "bn_cl_finalize": {0: "part"}, "bn_cl_bwd": {6: "part"},
    # "labels int32 [N, T or more] (first counts[n] valid)"
    "ctc_greedy": {2: "labels"},
    # "sdst (fp32 [ns or more])"
    "multi_copy": {2: "sdst"},
    # "scale a device fp32 scalar": one fp32 scalar on the device is [1 or more]
    "fc_bias_grad": {2: "scale"},
    "ctc_beam": {12: "err"}, "ctc_beam_lm": {12: "err"},
    # "scales ... fp32 [2 or more]. part: fp32 [2 * fp8_quant_blocks or more]"
    "fp8_quant2": {5: "part", 6: "scales"},
    # "split-K through ... one fp32 workspace (S * batch * M * N floats or more ...) and one zeroed
    # int32 counter buffer (tiles or more; one buffer per stream)"
    "gemm8": {6: "alpha_dev", 7: "alpha_dev2", 11: "ws", 12: "cnt"}, "gemm8_group": {7: "ws", 8: "cnt"},
    "seq_dropout": {2: "ctr"},
    # "part fp32 [hist_blocks(n), 6 or more]"; "done (int32 [1 or more])"
    "hist_stats": {2: "part"}, "spin": {4: "done"},
}
# Slots whose own length is the problem size n, with no second argument that fixes it: a shorter
# view is a valid, smaller call. Exempt from the one-element-short case.
DEFINES_N = {
    "grad_norm": {0}, "grad_sumsq": {0}, "clip_finalize": {0}, "hist_stats": {0},
    "multi_fill": {0}, "gemm": {16}, "gemm8": {14},           # fill regions
    "multi_copy": {0, 1},                                    # 1-D pairs: src <= dst is all that is asked
}
# "contiguous tensor of any dtype": fill regions are bytes. Exempt from the wrong-dtype case.
ANY_DTYPE = {"multi_fill": {0}, "gemm": {16}, "gemm8": {14}}
# No public wrapper reaches these; each is driven by a direct call with hand-built arguments.
DIRECT = {
    "spin": "a test aid (tools/coresidency.py)",
    "fp8_quant_pow2": "superseded in ops/rnn.py by fp8_quant_u; kept as its per-tensor oracle",
    "fp8_quant_pow2_t": "superseded in ops/rnn.py by fp8_quant_u; kept as its per-tensor oracle",
    "adam_ema_ranges": "issued by the data-parallel bucketer only",
}


class Recording:
    """Stands in for the extension: every tensor-taking binding is recorded, then launched."""

    def __init__(self, C, names):
        self._C, self._names, self.calls = C, names, []

    def __getattr__(self, attr):
        f = getattr(self._C, attr)
        if attr not in self._names:
            return f

        def call(*args, **kw):
            self.calls.append((attr, list(args), dict(kw)))
            return f(*args, **kw)
        return call


# ------------------------------------------------------------------------------ the scenarios
def s_recurrence(dev, family):
    from deepspeech_amd.ops import rnn as RNN
    N, H, T = (8, 256, 4) if family == "fp8" else (5, 64, 4)
    plan = RNN.make_plan(N, H, "gru", 2, 256, "step" if family == "v1" else "auto")
    lens = torch.tensor([T] + [T - 1] * (N - 1), dtype=I32, device=dev)
    gx = (torch.randn(T, N, 6 * H) * 0.5).bfloat16().to(dev)
    dy = torch.randn(T, N, H).bfloat16().to(dev)
    U = [(torch.randn(3 * H, H) / math.sqrt(H)).bfloat16().to(dev) for _ in range(2)]
    bh = [(torch.randn(3 * H) * 0.1).to(dev) for _ in range(2)]
    fuse, RNN._FUSE_DIRSUM = RNN._FUSE_DIRSUM, False              # y as the stacked direction pair
    try:
        if family == "fp8":
            _, (hx, hs, gates) = RNN._run_fwd_fp8(gx, lens, U, bh, plan)
            RNN._run_bwd_fp8(dy, lens, U, hs, gates, plan, 6 * H)
        else:
            _, (hx, hs, gates) = RNN._run_fwd(gx, lens, U, bh, plan)
            RNN._run_bwd(dy, lens, U, hx, hs, gates, plan, 6 * H)
    finally:
        RNN._FUSE_DIRSUM = fuse


def s_train_step(dev):
    """the conv front-end, the projections, the fused head and the optimizer of one training step"""
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.trainer import LRSchedule, Trainer
    model = DeepSpeech2(num_filters=32, num_hidden=256, num_rnn_layers=2, cell="gru").to(dev)
    model.set_engine("hip", torch.bfloat16)
    tr = Trainer(model, LRSchedule(1e-4, 1000, 0.9))
    tr.step(to_device(FixedShapeBatches(8, max_frames=300, seed=0, pool=1).next(), dev))


def s_ctc(dev):
    from deepspeech_amd.lm import CharNgramLM, synthetic_corpus
    from deepspeech_amd.ops import align, ctc, decode
    T, N, K = 12, 3, 29
    logits = torch.randn(T, N, K, device=dev)
    lens = torch.tensor([T, T - 1, T - 3], dtype=I32, device=dev)
    labels = torch.randint(0, K - 1, (N, 4), dtype=I32, device=dev)
    label_lens = torch.tensor([4, 3, 2], dtype=I32, device=dev)
    ctc.ctc_loss_hip(logits, lens, labels, label_lens)
    decode.greedy_decode(logits, lens)
    decode.beam_decode(logits, lens, 4)
    decode.beam_decode(logits, lens, 4, lm=CharNgramLM.train(synthetic_corpus(150, seed=3), 2))
    align.ctc_forced_align(logits, lens, labels, label_lens)


def s_bn(dev):
    from deepspeech_amd.ops.frontend import BNClip
    N, C, T, F = 2, 3, 5, 7
    y = torch.randn(N, C, T, F, device=dev, requires_grad=True)
    g, b = torch.ones(C, device=dev, requires_grad=True), torch.zeros(C, device=dev, requires_grad=True)
    out = BNClip.apply(y, g, b, torch.zeros(C, device=dev), torch.ones(C, device=dev), True, 0, F32, 1)
    out.backward(torch.randn_like(out))


def s_optimizer(dev):
    from deepspeech_amd.ops.optim import FusedAdamEMA, ParamArena
    m = torch.nn.Linear(13, 7).to(dev)
    arena = ParamArena(m)
    arena.grad.normal_()
    opt = FusedAdamEMA(arena, ema_decay=0.99, bf16_copy=True, max_grad_norm=1.0)
    opt.grad_norm_and_finite(0.5)
    opt.step(lr=1e-2, global_step=0)


def s_gemm(dev):
    from deepspeech_amd.ops import gemm as G
    M, N, K = 40, 24, 256                                        # one tile with a ragged edge
    a, b = torch.randn(M, K, device=dev).to(BF), torch.randn(N, K, device=dev).to(BF)
    one = torch.ones(1, device=dev)
    G.gemm(a, b, torch.empty(M, N, device=dev, dtype=BF), M, N, K, False, False, 0, 1.0, torch.zeros(N, device=dev, dtype=BF),
           alpha_dev=one)
    G.gemm8(a, b, torch.empty(M, N, device=dev, dtype=BF), 0, 1.0, torch.zeros(N, device=dev, dtype=BF), one, one, splits=1)
    G.gemm8(a, b, torch.empty(M, N, device=dev), 1, splits=2, fill=([torch.empty(8, device=dev)], [0]))
    G.gemm8_group([(torch.randn(4000, 256, device=dev).to(BF), torch.randn(4000, 264, device=dev).to(BF),
                    torch.empty(256, 264, device=dev))])
    x, w = torch.randn(16, 136, device=dev).to(BF), torch.randn(8, 136, device=dev).to(BF)
    G.linear_fp8(x, w, None, 1.0)


def s_augment(dev):
    from deepspeech_amd.ops import dropout, lookahead, specaug
    B, T, F = 3, 16, 8
    feats = torch.randn(B, T, F, device=dev)
    lens = torch.tensor([16, 12, 9], dtype=I32, device=dev)
    specaug.SpecAugment(specaug.SpecAugPolicy(nF=2, Fw=3, nT=2, Tw=4, W=2), seed=5)(feats, lens, step=1)
    x = torch.randn(T, B, 16, device=dev).to(BF)
    dropout.seq_dropout(x, dropout.DropoutState(dev), seed=7, site=0, thr=6554)
    w16 = torch.randn(16, 3, device=dev).to(BF)
    lookahead.lookahead_fwd(x, w16, lens)
    lookahead.lookahead_bwd_data(x, w16, lens)
    lookahead.lookahead_bwd_weight(x, x.clone(), lens, 2, torch.empty(16, 3, device=dev))
    lookahead.lookahead_stream(torch.zeros(2, B, 16, device=dev, dtype=BF), x[:4].contiguous(), w16)


def s_audio(dev):
    from deepspeech_amd.ops.featurize import AudioFeaturizer
    from deepspeech_amd.ops.resample import Resampler
    pcm = torch.randn(2, 800) * 0.1
    AudioFeaturizer("mfcc", device=dev)(pcm, torch.tensor([800, 640], dtype=I32))
    Resampler(8000, 16000, device=dev)(pcm[:, :300].contiguous())


def s_stats(dev):
    from deepspeech_amd.utils.stats import NonfiniteWatch, histogram
    histogram(torch.randn(100, device=dev))
    NonfiniteWatch(dev).update(torch.ones((), device=dev))


def s_direct(dev):
    """DIRECT, and the copy kernels a training step reaches only in some configurations"""
    from deepspeech_amd.ops import _ext
    C = _ext.ext()
    x = torch.randn(64, 64, device=dev).to(BF)
    w = torch.empty(2, device=dev, dtype=I32)
    C.fp8_quant_pow2(x, torch.empty(64, 64, device=dev, dtype=torch.uint8), w[0:1], w[1:2])
    C.fp8_quant_pow2_t(x, torch.empty(64, 64, device=dev, dtype=torch.uint8), w[0:1], w[1:2])
    p = [torch.randn(256, device=dev) for _ in range(5)]
    p[3].abs_()
    C.adam_ema_ranges(*p, torch.empty(256, device=dev, dtype=BF), [0, 64, 128, 200], 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.9)
    C.spin(1000, 1, 64, 4, torch.zeros(1, device=dev, dtype=I32))
    C.transpose_bf16(x[:8, :16], torch.empty(16, 8, device=dev, dtype=BF))
    C.multi_copy([torch.empty(4, 8, device=dev), torch.empty(9, device=dev)],
                 [torch.randn(4, 6, device=dev), torch.randn(5, device=dev)], torch.empty(2, device=dev), [1.0, 2.0])
    feats = torch.randn(2, 40, 161, device=dev)
    C.prep_inputs(feats, torch.empty_like(feats, dtype=BF), torch.tensor([40, 38], dtype=I32, device=dev),
                  torch.empty(2, dtype=I32, device=dev))
    C.multi_fill([torch.empty(16, device=dev)], [0])
    C.wait_resident(torch.zeros(1, dtype=I32, device=dev), 1000)
    C.cast_bf16(p[0], torch.empty(256, device=dev, dtype=BF))
    C.col_sum([torch.randn(2, 3, 4, device=dev)], [torch.empty(8, device=dev)], [False])
    C.fc_bias_grad(torch.randn(12, 32, device=dev).to(BF), 29, torch.ones(1, device=dev), 1.0, torch.empty(29, device=dev), False)
    h, W = torch.randn(12, 64, device=dev).to(BF), torch.randn(29, 64, device=dev).to(BF)
    C.fc_logits(h, W, torch.zeros(29, device=dev, dtype=BF), torch.empty(12, 29, device=dev))


SCENARIOS = [("v1", lambda d: s_recurrence(d, "v1")), ("xcd", lambda d: s_recurrence(d, "xcd")),
             ("fp8", lambda d: s_recurrence(d, "fp8")), ("train", s_train_step), ("ctc", s_ctc), ("bn", s_bn),
             ("optimizer", s_optimizer), ("gemm", s_gemm), ("augment", s_augment), ("audio", s_audio), ("stats", s_stats),
             ("direct", s_direct)]


def tensor_bindings(C):
    return {n for n in dir(C) if not n.startswith("_") and "Tensor" in (getattr(C, n).__doc__ or "")}


def _tensors(v):
    return [v] if isinstance(v, torch.Tensor) else [t for t in v if isinstance(t, torch.Tensor)] if isinstance(v, list) else []


@pytest.fixture(scope="module")
def recorded(cuda):
    """(C, calls by binding name, scenario errors): every scenario once, under the recorder"""
    from deepspeech_amd.ops import _ext, rnn as RNN
    C = _ext.ext()
    rec = Recording(C, tensor_bindings(C))
    mp = pytest.MonkeyPatch()
    mp.setattr(_ext, "ext", lambda: rec)
    errors = {}
    try:
        torch.manual_seed(11)
        for name, run in SCENARIOS:
            try:
                run(cuda)
            except Exception as e:                       # reported by test_every_tensor_binding_is_recorded
                errors[name] = repr(e)
    finally:
        mp.undo()
    torch.cuda.synchronize()
    RNN.check_errors()
    by_name, seen = {}, set()
    for name, args, kw in rec.calls:
        # one call per binding and per pattern of which arguments are tensors, lists or None
        key = (name, tuple(type(a).__name__ for a in args), tuple(sorted(kw)))
        if key not in seen:
            seen.add(key)
            by_name.setdefault(name, []).append((args, kw))
    return C, by_name, errors


def test_every_tensor_binding_is_recorded(recorded):
    C, by_name, errors = recorded
    assert not errors, errors
    assert tensor_bindings(C) - set(by_name) == set()
    assert set(DIRECT) <= tensor_bindings(C)


def _slots(C, name, args, kw):
    """(key into args or kw, positional index, value) of every argument: a keyword argument's
    position is that of its name in the binding's docstring"""
    sig = (getattr(C, name).__doc__ or "").split("\n")[0]
    names = re.findall(r"(\w+): ", sig[sig.index("(") + 1:])
    return [(i, i, a) for i, a in enumerate(args)] + [(k, names.index(k), v) for k, v in kw.items()]


def _bits(t):
    return t.detach().clone().contiguous().reshape(-1).view(torch.uint8)


def _refused(C, name, args, kw, key, idx, bad):
    a, k = list(args), dict(kw)
    where = a if isinstance(key, int) else k
    where[key] = bad if idx is None else where[key][:idx] + [bad] + where[key][idx + 1:]
    with pytest.raises(RuntimeError) as e:
        getattr(C, name)(*a, **k)
    assert name in str(e.value) and "kernel launch failed" not in str(e.value), str(e.value)


@pytest.mark.parametrize("name", sorted(set(OR_MORE) | {
    "bn_stats", "bn_apply", "bn_bwd", "grad_sumsq", "cast_bf16", "prep_inputs", "transpose_bf16", "gemm", "multi_fill",
    "col_sum", "wait_resident", "ctc_beam_backtrack", "ctc_beam_backtrack_lm", "bn_cl_apply", "fc_logits", "lookahead",
    "lookahead_wgrad", "lookahead_stream", "specaug_plan", "specaug_mean", "specaug_apply", "audio_stats", "featurize",
    "resample", "nonfinite_watch"}))
def test_wrong_dtype_and_one_short_are_refused(recorded, name):
    C, by_name, _ = recorded
    assert name in by_name, "no scenario recorded " + name
    for args, kw in by_name[name]:
        every = [t for a in list(args) + list(kw.values()) for t in _tensors(a)]
        before = [_bits(t) for t in every]
        for key, pos, a in _slots(C, name, args, kw):
            members = [(None, a)] if isinstance(a, torch.Tensor) else [(i, t) for i, t in enumerate(a)] if _tensors(a) else []
            for idx, good in members:
                if pos not in ANY_DTYPE.get(name, ()):
                    _refused(C, name, args, kw, key, idx, torch.zeros(good.shape, dtype=torch.float64, device=good.device))
                short_exempt = pos in OR_MORE.get(name, ()) or (pos in DEFINES_N.get(name, ()) and
                                                                (name != "multi_copy" or good.dim() == 1))
                if good.numel() > 0 and not short_exempt:
                    _refused(C, name, args, kw, key, idx, good.flatten()[:-1])
        for t, b in zip(every, before):
            assert torch.equal(_bits(t), b), name + ": a refused call changed a tensor"
    torch.cuda.synchronize()


def test_the_parametrisation_names_every_binding(recorded):
    C = recorded[0]
    marks = test_wrong_dtype_and_one_short_are_refused.pytestmark
    names = {n for m in marks if m.name == "parametrize" for n in m.args[1]}
    assert names == tensor_bindings(C), sorted(names ^ tensor_bindings(C))
