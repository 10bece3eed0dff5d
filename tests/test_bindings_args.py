"""csrc/bindings.cpp turns a tensor into a pointer only through csrc/bind_args.h, whose helpers
always check the device first. Three properties, none of which needs a GPU: the source holds no
data_ptr of its own, every tensor-taking binding has a row in the argument table below, and every
row, called with correctly shaped and typed CPU tensors, is refused before any launch."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from deepspeech_amd import _C
except ImportError:          # not built: the source property still holds
    _C = None

F32, BF, I32, I64, U8, I16 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8, torch.int16
F8 = torch.float8_e4m3fn


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


# ---- the recurrences: N = 5, H = 64, T = 4, two directions, GRU (fp8: N = 8, H = 256)
T, N, H, NP1 = 4, 5, 64, 16
G1 = [T, N, NP1, H, 1, 0, T, 6 * H, 2, 0, 1, 0]          # generation 1: NP = BG * 16 * mt
GX = [T, N, N, H, 1, N, T, 6 * H, 2, 0, 1, 0]            # XCD groups of R = N rows
N8, H8 = 8, 256
G8 = [T, N8, N8, H8, 1, N8, T, 6 * H8, 2, 0, 1, 0]


def _rnn(g, h, n, np_):
    return dict(gx=z(BF, T, n, 6 * h), dy=z(BF, T, n, h), dgx=z(BF, T, n, 6 * h), lens=z(I32, n), U=z(BF, 3 * h, h),
                bh=z(F32, 3 * h), y=z(BF, 2, T, n, h), hx=z(BF, 2, T + 1, np_, h), hs=z(F32, 2, T + 1, np_, h),
                gates=z(F32, 2, T, np_, 4 * h), dgh=z(BF, 2, T, np_, 3 * h), carry=z(F32, 2, np_, h),
                parts=z(F32, 2, 2, 1, 3 * h), err=z(I32, 1))


def _rnn_fwd():
    r = _rnn(G1, H, N, NP1)
    return (G1, 4, 1, True, r["gx"], r["lens"], r["U"], r["U"], r["bh"], r["bh"], r["y"], r["hx"], r["hs"], r["gates"],
            z(I32, 2 * H // 16), r["err"], 1000, None)


def _rnn_bwd():
    r = _rnn(G1, H, N, NP1)
    return (G1, 4, 1, True, r["dy"], r["lens"], r["U"], r["U"], r["hs"], r["gates"], r["dgh"], r["dgx"], r["carry"],
            r["parts"], 1.0, z(I32, 2 * H // 16), r["err"], 1000, None)


def _rnnx_fwd():
    r = _rnn(GX, H, N, N)
    return (GX, r["gx"], r["lens"], r["U"], r["U"], r["bh"], r["bh"], r["y"], None, r["hx"], r["hs"], r["gates"],
            z(I32, 2 * H // 32), r["err"], 1000, None)


def _rnnx_bwd():
    r = _rnn(GX, H, N, N)
    ring = z(F32, 2, int(_C.rnnx_ring_floats(H, 1, N)))
    return (GX, r["dy"], r["lens"], r["U"], r["U"], r["hs"], r["gates"], r["dgh"], r["dgx"], r["parts"], 1.0,
            z(I32, 2 * H // 32), r["err"], ring, 1000, None)


def _rnnf8_fwd():
    r = _rnn(G8, H8, N8, N8)
    return (G8, r["gx"], r["lens"], z(U8, 2, 3 * H8, H8), z(I32, 2), r["bh"], r["bh"], r["y"], z(U8, 2, T + 1, N8, H8),
            r["hx"], r["hs"], r["gates"], z(I32, 2 * H8 // 64), r["err"], 1000)


def _rnnf8_bwd():
    r = _rnn(G8, H8, N8, N8)
    ring = z(I32, 2, int(_C.rnnf8_ring_words(H8, 1, N8)))
    return (G8, r["dy"], r["lens"], z(U8, 2, H8, 3 * H8), z(I32, 2), r["hs"], r["gates"], r["dgh"], r["dgx"], r["parts"],
            1.0, z(I32, 2 * H8 // 64), r["err"], ring, 1000)


# ---- CTC, alignment, beam search: T = 6, N = 2, K = 29
CT, CN, CK, CL = 6, 2, 29, 3


def _ctc():
    return z(I32, CN), z(I32, CN, CL), z(I32, CN)


def _beam(lm=False):
    B, W, cap = 2, 4, 16
    st = (z(I32, B, W), z(I32, B, W), z(I32, B, W), z(F32, B, W), z(F32, B, W), z(I32, B), z(I32, B, cap, 2), z(I32, B))
    return B, W, st


def _ctc_beam(lm):
    B, W, st = _beam()
    tail = (z(I32, 3, CK, 2), z(I32, B, W), z(I64, B, W, 2)) if lm else (z(I64, B, W, 2),)
    return (z(F32, CT, B, CK), None, 0, 1e-4) + st + (z(I32, 1),) + tail


def _ctc_backtrack(lm):
    B, W, st = _beam()
    tail = (z(I32, 3, CK, 2), z(I32, B, W), 0) if lm else ()
    return st + (z(I32, B, W, 8), z(I32, B, W), z(F32, B, W)) + tail


# ---- conv front-end: N = 1, T = 20, F0 = 161 -> T1 = 1, F1 = 79 -> T2 = 1, F2 = 38
def _vec(n=4):
    return tuple(z(F32, 32) for _ in range(n))


X0, Y1, Y2 = (1, 20, 161), (1, 1, 79, 32), (1, 1, 38, 32)

# ---- one row per tensor-taking binding: the positional arguments of a small, valid call
TABLE = {
    "rnn_fwd": _rnn_fwd, "rnn_bwd": _rnn_bwd, "rnnx_fwd": _rnnx_fwd, "rnnx_bwd": _rnnx_bwd,
    "rnnf8_fwd": _rnnf8_fwd, "rnnf8_bwd": _rnnf8_bwd,
    "fp8_quant_pow2": lambda: (z(BF, 64, 64), z(U8, 64, 64), z(I32, 1), z(I32, 1)),
    "fp8_quant_pow2_t": lambda: (z(BF, 64, 64), z(U8, 64, 64), z(I32, 1), z(I32, 1)),
    "fp8_quant_u": lambda: (z(BF, 64, 64), z(BF, 64, 64), z(U8, 2, 64, 64), z(U8, 2, 64, 64), z(I32, 2), z(F32, 512)),
    "ctc_fused": lambda: (z(F32, CT, CN, CK),) + _ctc() + (z(F32, CN), z(F32, CT, CN, CK),
                                                           z(F32, int(_C.ctc_ws_floats(CT, CN, CL))), 0, True),
    "ctc_align": lambda: (z(F32, CT, CN, CK),) + _ctc() + (z(I32, CN, CT), z(I32, CN, CL), z(I32, CN, CL), z(F32, CN, CL),
                                                           z(F32, CN), z(U8, int(_C.ctc_align_ws_bytes(CT, CN, CL))), 0, False),
    "bn_stats": lambda: (z(F32, 2, 3, 4, 5), z(F32, 3 * int(_C.bn_chunks(2, 4, 5)) * 2), 1e-5, z(F32, 3), z(F32, 3),
                         None, None, 0.1),
    "bn_apply": lambda: (z(F32, 2, 3, 4, 5), z(F32, 3), z(F32, 3), z(F32, 3), z(F32, 3), z(F32, 2, 3, 4, 5), 0),
    "bn_bwd": lambda: (z(F32, 2, 3, 4, 5), z(F32, 2, 3, 4, 5), z(F32, 3), z(F32, 3), z(F32, 3), z(F32, 3),
                       z(F32, 3 * int(_C.bn_chunks(2, 4, 5)) * 2), z(F32, 3), z(F32, 3), z(F32, 2, 3, 4, 5), 0),
    "adam_ema": lambda: (z(F32, 64), z(F32, 64), z(F32, 64), z(F32, 64), z(F32, 64), z(BF, 64), 1e-3, 0.9, 0.999, 1e-8,
                         1.0, 0.99, None, 0),
    "adam_ema_ranges": lambda: (z(F32, 64), z(F32, 64), z(F32, 64), z(F32, 64), None, None, [0, 32], 1e-3, 0.9, 0.999,
                                1e-8, 1.0, 0.99),
    "grad_norm": lambda: (z(F32, 64), 1.0, z(F32, int(_C.grad_norm_blocks(64))), z(I32, 1)),
    "grad_sumsq": lambda: (z(F32, 64), 1.0, z(F32, 1)),
    "clip_finalize": lambda: (z(F32, 1), 1.0, z(F32, 8)),
    "cast_bf16": lambda: (z(F32, 64), z(BF, 64)),
    "prep_inputs": lambda: (z(F32, 2, 40, 161), z(BF, 2, 40, 161), z(I32, 2), z(I32, 2)),
    "multi_copy": lambda: ([z(F32, 4, 8)], [z(F32, 4, 6)]),
    "fp8_quant2": lambda: (z(BF, 16, 64), z(BF, 8, 64), 1.0, z(F8, 16, 128), z(F8, 8, 128),
                           z(F32, 2 * int(_C.fp8_quant_blocks(16 * 128, 8 * 128))), z(F32, 2)),
    "transpose_bf16": lambda: (z(BF, 4, 8), z(BF, 8, 4)),
    "gemm8": lambda: (z(BF, 16, 64), z(BF, 8, 64), z(F32, 16, 8), None, 1),
    "gemm8_group": lambda: ([z(BF, 16, 64)], [z(BF, 8, 64)], [z(F32, 16, 8)], [1], [1], False, False, None, None, 0),
    "gemm": lambda: (z(BF, 16, 16), z(BF, 8, 16), z(F32, 16, 8), None, 16, 8, 16, False, False, 1, 1.0, 3),
    "multi_fill": lambda: ([z(F32, 16)], [0]),
    "col_sum": lambda: ([z(F32, 2, 3, 4)], [z(F32, 8)], [False]),
    "wait_resident": lambda: (z(I32, 1), 1000),
    "fc_bias_grad": lambda: (z(BF, 12, 32), 29, z(F32, 1), 1.0, z(F32, 29), False),
    "ctc_beam": lambda: _ctc_beam(False), "ctc_beam_lm": lambda: _ctc_beam(True),
    "ctc_beam_backtrack": lambda: _ctc_backtrack(False), "ctc_beam_backtrack_lm": lambda: _ctc_backtrack(True),
    "ctc_greedy": lambda: (z(F32, CT, CN, CK), z(I32, CN), z(I32, CN, CT), z(I32, CN), 0, z(F32, CN)),
    "conv1_fwd": lambda: (z(BF, *X0), z(BF, 32, 1, 20, 5), z(F32, 32), z(BF, *Y1), z(F32, int(_C.conv1_fwd_grid(1, 1)) * 64)),
    "conv2_fwd": lambda: (z(BF, *Y1), z(BF, 32, 32, 10, 5), z(F32, 32), z(BF, *Y2), z(F32, 2 * 64), 2),
    "conv2_dgrad": lambda: (z(BF, *Y2), z(BF, 32, 32, 10, 5), z(BF, *Y1), 2, z(BF, *Y1)) + _vec() + (z(F32, 2 * 64),),
    "conv2_wgrad": lambda: (z(BF, *Y2), z(BF, *Y1), z(F32, int(_C.conv2_wgrad_part_floats(2))), z(F32, 32, 32, 10, 5), 2),
    "conv1_wgrad": lambda: (z(BF, *Y1), z(BF, *X0), z(F32, int(_C.conv1_wgrad_part_floats(2))), z(F32, 32, 1, 20, 5), 2,
                            z(BF, *Y1)) + _vec(6),
    "bn_cl_finalize": lambda: (z(F32, 2 * 64), 2, 79.0, 1e-5) + _vec(2) + (z(F32, 32), z(F32, 32), 0.1),
    "bn_cl_apply": lambda: (z(BF, *Y1),) + _vec() + (z(BF, *Y1), False),
    "bn_cl_bwd": lambda: (z(BF, *Y1), z(BF, *Y1)) + _vec() + (z(F32, 2 * 64), 2) + _vec(2) + (z(BF, *Y1), False),
    "head_ctc": lambda: (z(BF, CT, CN, 64), z(BF, CK, 64), z(BF, CK)) + _ctc() + (
        z(F32, CN), z(BF, CT * CN, 32), z(F32, int(_C.ctc_ws_floats(CT, CN, CL))), 0, True),
    "fc_logits": lambda: (z(BF, 12, 64), z(BF, CK, 64), z(BF, CK), z(F32, 12, CK)),
    "lookahead": lambda: (z(BF, 8, 2, 16), z(BF, 16, 3), z(I32, 2), z(BF, 8, 2, 16), False),
    "lookahead_wgrad": lambda: (z(BF, 8, 2, 16), z(BF, 8, 2, 16), z(I32, 2),
                                z(F32, int(_C.lookahead_wgrad_parts(8, 2, 16)), 16 * 3), 2),
    "lookahead_stream": lambda: (z(BF, 2, 2, 16), z(BF, 4, 2, 16), z(BF, 16, 3), z(BF, 4, 2, 16)),
    "specaug_plan": lambda: (z(I32, 2), z(I32, 2, 2 + 2 * 2 + 2 * 2), 16, 8, 2, 3, 2, 4, 200000, 2, 1, 2, 3, 4, 5),
    "specaug_mean": lambda: (z(F32, 2, 16, 8), z(I32, 2), z(F32, 2, 8)),
    "specaug_apply": lambda: (z(F32, 2, 16, 8), z(I32, 2), z(I32, 2, 10), z(F32, 2, 8), z(F32, 2, 16, 8), 2, 2, False),
    "seq_dropout": lambda: (z(BF, 4, 2, 16), z(BF, 4, 2, 16), z(I32, 2), 1, 2, 0, 6554, 1.1, False),
    "audio_stats": lambda: (z(F32, 2, 800), z(I32, 2), z(F32, 2), z(F32, 2)),
    "featurize": lambda: (z(I16, 2, 800), None, z(F32, 2), z(F32, 2), z(F32, 320, 320), None, None, None, None, 1, 0, 0,
                          z(F32, 2, 4, 161), z(I32, 2)),
    "resample": lambda: (z(F32, 2, 300), None, z(F32, 2, 16), 2, 1, -7, 0, True, z(F32, 2, 600), z(I32, 2)),
    "hist_stats": lambda: (z(F32, 100), z(I32, int(_C.hist_nbucket())), z(F32, int(_C.hist_blocks(100)), 6)),
    "nonfinite_watch": lambda: (z(F32, 1), z(I32, 1), z(I32, 1)),
    "spin": lambda: (1000, 1, 64, 4, z(I32, 1)),
}


def test_bindings_source_holds_no_data_ptr():
    with open(os.path.join(ROOT, "deepspeech_amd", "csrc", "bindings.cpp")) as f:
        text = f.read()
    assert "data_ptr" not in text, "a tensor must become a pointer through csrc/bind_args.h only"
    with open(os.path.join(ROOT, "deepspeech_amd", "csrc", "bind_args.h")) as f:
        assert "data_ptr" in f.read()


def tensor_bindings():
    return {n for n in dir(_C) if not n.startswith("_") and "Tensor" in (getattr(_C, n).__doc__ or "")}


@pytest.mark.skipif(_C is None, reason="the extension is not built")
def test_every_tensor_binding_has_a_row():
    names = tensor_bindings()          # 59 of the 94 entry points
    assert names == set(TABLE), (sorted(names - set(TABLE)), sorted(set(TABLE) - names))


@pytest.mark.skipif(_C is None, reason="the extension is not built")
@pytest.mark.skipif(torch.cuda.is_available(), reason="meant for machines where a launch cannot happen")
@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_refused_before_any_launch(name):
    args = TABLE[name]()
    assert any(isinstance(a, torch.Tensor) or (isinstance(a, list) and a and isinstance(a[0], torch.Tensor)) for a in args)
    with pytest.raises(RuntimeError) as e:
        getattr(_C, name)(*args)
    msg = str(e.value)
    assert "GPU" in msg and "kernel launch failed" not in msg, msg
    assert name in msg.split("\n")[0], msg
