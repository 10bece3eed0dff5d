"""The launchers of csrc/speed.hip live in the submodule ``_C.speed`` and get the guarantees
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
B, S, W = 2, 2400, 2720                  # W: the worst case of (90, 100, 110) at S
VTAB = [90, 10, 9, 48, 0, 100, 1, 1, 0, 0, 110, 10, 11, 54, 480]
H = 480 + 540


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


TABLE = {
    "plan": lambda: (z(I32, B), z(I32, B), z(I32, B, 2), S, 0, list(VTAB), 1, 2, 3, 4, 5),
    "apply": lambda: (z(I16, B, S), None, z(I32, B, 2), z(F32, H), list(VTAB), z(F32, B, W), z(I32, B), False),
}


def tensor_bindings():
    P = _C.speed
    return {n for n in dir(P) if not n.startswith("_") and "Tensor" in (getattr(P, n).__doc__ or "")}


@pytest.mark.skipif(_C is None, reason="the extension is not built")
def test_the_submodule_stays_out_of_the_top_level_enumeration():
    assert hasattr(_C, "speed")
    assert "Tensor" not in (_C.speed.__doc__ or "")
    assert not any(n.startswith("speed") and "Tensor" in (getattr(_C, n).__doc__ or "") for n in dir(_C))
    assert not any("speed" in n for n in dir(_C.waveaug))
    assert int(_C.speed.tile()) == 1024


@pytest.mark.skipif(_C is None, reason="the extension is not built")
def test_every_tensor_binding_has_a_row():
    assert tensor_bindings() == set(TABLE)


@pytest.mark.skipif(_C is None, reason="the extension is not built")
def test_supported_names_the_contract():
    ok = _C.speed.supported
    assert ok(VTAB, H) and ok([100, 1, 1, 0, 0], 0)
    assert not ok(VTAB, H - 1)                                    # the last table leaves h
    assert not ok(VTAB[:14], H) and not ok([], H) and not ok(VTAB * 3, H)
    for slot, bad in ((0, 49), (0, 110), (1, 9), (3, 47), (3, 322), (4, 2), (5, 201), (6, 2)):
        t = list(VTAB)
        t[slot] = bad
        assert not ok(t, 1 << 20), (slot, bad)
    # every percent of the range fits the LDS: the largest table is 100 x 96 words at 199 %
    for p in range(50, 201):
        if p != 100:
            from math import gcd
            L, M = 100 // gcd(p, 100), p // gcd(p, 100)
            K = 2 * -((-24 * max(L, M)) // L)
            assert ok([p, L, M, K, 0], L * K), p


@pytest.mark.skipif(_C is None, reason="the extension is not built")
@pytest.mark.skipif(torch.cuda.is_available(), reason="meant for machines where a launch cannot happen")
@pytest.mark.parametrize("name", sorted(TABLE))
def test_cpu_tensors_are_refused_before_any_launch(name):
    args = TABLE[name]()
    assert any(isinstance(a, torch.Tensor) for a in args)
    with pytest.raises(RuntimeError) as e:
        getattr(_C.speed, name)(*args)
    msg = str(e.value)
    assert "GPU" in msg and "kernel launch failed" not in msg, msg
    assert name in msg.split("\n")[0] and "speed" in msg.split("\n")[0], msg


@pytest.mark.skipif(_C is None, reason="the extension is not built")
@pytest.mark.parametrize("name,slot,bad", [
    ("apply", 0, z(F64, B, S)),                      # dtype
    ("apply", 0, z(F32, B * S)),                     # not [B, S]
    ("apply", 5, z(F32, B, W - 160)),                # narrower than the worst case, and not vouched for
    ("apply", 5, z(F32, B + 1, W)),
    ("apply", 3, z(F32, H - 4)),                     # a table outside h
    ("apply", 4, VTAB[:10] + [110, 10, 11, 54, 482]),    # a table off its 16-byte boundary
    ("plan", 5, VTAB + VTAB[:5]),                    # a repeated percent
    ("plan", 5, [100, 1, 1, 0, 0] * 9),              # V > 8
    ("plan", 5, [40, 5, 2, 48, 0]),                  # 40 %
    ("plan", 2, z(I32, B, 4)),                       # plan [B, 2]
    ("plan", 3, 1 << 30),                            # S
    ("plan", 4, -1),                                 # max_out
    ("plan", 10, -1),                                # first_utt is a 32-bit word
])
def test_contract_violations_name_the_op(name, slot, bad):
    args = list(TABLE[name]())
    args[slot] = bad
    with pytest.raises((RuntimeError, TypeError)) as e:
        getattr(_C.speed, name)(*args)
    assert "kernel launch failed" not in str(e.value)
    assert "speed." + name in str(e.value), str(e.value)
