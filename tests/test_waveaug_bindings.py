"""The launchers of csrc/waveaug.hip live in the submodule ``_C.waveaug`` and get the guarantees
tests/test_bindings_args.py gives the top-level entries, none of which needs a GPU: no data_ptr
outside csrc/bind_args.h (checked there for the whole file), a row in the table below for every
tensor-taking entry, and every row, called with correctly shaped and typed CPU tensors, refused
before any launch."""
import pytest
import torch

try:
    from deepspeech_amd import _C
except ImportError:          # not built
    _C = None

F32, F64, I32, I16 = torch.float32, torch.float64, torch.int32, torch.int16
B, S, C, NTOT = 2, 4104, 3, 900          # two segments per row


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


def _bank():
    return z(F32, NTOT), z(I32, C), torch.full((C,), 300, dtype=I32)


TABLE = {
    "plan": lambda: (z(I32, B), _bank()[2], z(I32, B, 4), S, 400000, 1000, 3000, 1, 2, 3, 4, 5),
    "energy": lambda: (z(F32, B, S), z(I32, B), z(I32, B, 4)) + _bank() + (z(F32, B, 2, 2),),
    "coef": lambda: (z(I32, B), z(I32, B, 4), z(F32, B, 2, 2), z(F64, B, 2), z(F32, B), S),
    "apply": lambda: (z(I16, B, S), None, z(I32, B, 4), z(F32, B)) + _bank() + (z(F32, B, S),),
}


def tensor_bindings():
    W = _C.waveaug
    return {n for n in dir(W) if not n.startswith("_") and "Tensor" in (getattr(W, n).__doc__ or "")}


@pytest.mark.skipif(_C is None, reason="the extension is not built")
def test_the_submodule_stays_out_of_the_top_level_enumeration():
    assert hasattr(_C, "waveaug")
    assert "Tensor" not in (_C.waveaug.__doc__ or "")
    assert int(_C.waveaug.segment()) == 4096


@pytest.mark.skipif(_C is None, reason="the extension is not built")
def test_every_tensor_binding_has_a_row():
    assert tensor_bindings() == set(TABLE)


@pytest.mark.skipif(_C is None, reason="the extension is not built")
@pytest.mark.skipif(torch.cuda.is_available(), reason="meant for machines where a launch cannot happen")
@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_refused_before_any_launch(name):
    args = TABLE[name]()
    assert any(isinstance(a, torch.Tensor) for a in args)
    with pytest.raises(RuntimeError) as e:
        getattr(_C.waveaug, name)(*args)
    msg = str(e.value)
    assert "GPU" in msg and "kernel launch failed" not in msg, msg
    assert name in msg.split("\n")[0] and "waveaug" in msg.split("\n")[0], msg


@pytest.mark.skipif(_C is None, reason="the extension is not built")
@pytest.mark.parametrize("name,slot,bad", [
    ("energy", 0, z(F32, B, S + 4)),                 # S % 8 != 0
    ("energy", 0, z(F64, B, S)),                     # dtype
    ("apply", 0, z(F32, B * S)),                     # not [B, S]
    ("plan", 4, 1000001),                            # p_ppm
    ("plan", 5, 3001),                               # snr_lo > snr_hi
    ("plan", 11, -1),                                # first_utt is a 32-bit word
    ("coef", 5, S + 1),
])
def test_contract_violations_name_the_op(name, slot, bad):
    args = list(TABLE[name]())
    args[slot] = bad
    with pytest.raises((RuntimeError, TypeError)) as e:
        getattr(_C.waveaug, name)(*args)
    assert "kernel launch failed" not in str(e.value)
    assert "waveaug." + name in str(e.value), str(e.value)
