"""The streaming kernels of csrc/optim.hip, csrc/quant.hip, csrc/reduce.hip and csrc/fill.hip per
element against the oracles of tests/stream_cases.py, whose docstring holds the method and the
bounds. Every launch runs on guard-banded buffers; the drivers are the ones the CPU emulations of
tests/test_stream_oracle.py pass, here with the extension in the emulation's place.

Printed (run with -s): STREAMWORST lines, the worst err/tol per kernel, and STREAMCOUNT lines, the
launches checked. profiles/stream_oracle_coverage.md records them.
"""
import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from deepspeech_amd.ops import _ext  # noqa: E402

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def C():
    return _ext.ext()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(SC.WORST.items()):
        print("STREAMWORST %-28s err/tol %.3f" % (k, v))
    for k, v in sorted(SC.COUNTS.items()):
        print("STREAMCOUNT %-20s %d" % (k, v))


# ------------------------------------------------------------------------------ csrc/optim.hip
@pytest.mark.parametrize("n", SC.ADAM_GS_N)
def test_adam_grid_strided(C, n):
    """max_grid = 3: a stride of 768 float4 groups; n4 below it, one past it, 2, 2 + 5 / 768 and
    5 + 17 / 768 strides, tails of 0..3 elements; n = 1, 3, 4, 5"""
    SC.run_adam(C, DEV, dict(n=n, max_grid=3))


@pytest.mark.parametrize("n,max_grid", SC.ADAM_CHUNK)
def test_adam_block_contiguous(C, n, max_grid):
    """the block-contiguous launch against the oracle, and bitwise the grid-strided one"""
    SC.same_forms("n=%d" % n, SC.run_adam(C, DEV, dict(n=n, max_grid=3)), SC.run_adam(C, DEV, dict(n=n, max_grid=max_grid)))


@pytest.mark.parametrize("n", SC.ADAM_LDS_N)
def test_adam_lds_reserve_is_bitwise_the_plain_launch(C, n):
    a = SC.run_adam(C, DEV, dict(n=n, lds=0))
    SC.same_forms("n=%d lds_reserve" % n, a, SC.run_adam(C, DEV, dict(n=n, lds=32768)))
    SC.same_forms("n=%d lds_reserve, max_grid 3" % n, a, SC.run_adam(C, DEV, dict(n=n, lds=32768, max_grid=3)))


@pytest.mark.parametrize("opt", SC.ADAM_OPTIONS, ids=lambda o: "-".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in o.items()))
def test_adam_options(C, opt):
    """ema / p16 absent, gscale, the skip word, the device hyper pair (the scalar lr_t and ema_keep
    are NaN then): grid-strided and block-contiguous, bitwise each other"""
    a = SC.run_adam(C, DEV, dict(n=SC.ADAM_OPT_N, max_grid=3, **opt))
    SC.same_forms(str(opt), a, SC.run_adam(C, DEV, dict(n=SC.ADAM_OPT_N, max_grid=-7, **opt)))


@pytest.mark.parametrize("key", list(SC.ADAM_RANGES))
def test_adam_ranges(C, key):
    """0, 1 and 64 ranges (empty, adjacent, at both arena ends, unsorted): the oracle inside, bit-
    unchanged between them, and bitwise the single launch where the ranges cover the arena"""
    got = SC.run_adam(C, DEV, dict(n=SC.ARENA), ranges=key)
    SC.run_adam(C, DEV, dict(n=SC.ARENA, hyper=True, ema=False, gscale=SC.GSCALES[1]), ranges=key)
    whole = SC.run_adam(C, DEV, dict(n=SC.ARENA, max_grid=3))
    mask = torch.zeros(SC.ARENA, dtype=torch.bool)
    for lo, hi in SC.ADAM_RANGES[key]:
        mask[lo:hi] = True
    for k in got:
        SC.check_bits("ranges %s: %s against the single launch" % (key, k), got[k][mask], whole[k][mask])


@pytest.mark.parametrize("n", SC.GN_N)
def test_grad_norm(C, n):
    for parts in SC.GN_PARTS:
        for gs in (1.0, 0.5):
            SC.run_grad_norm(C, DEV, n, parts, gs)
    SC.run_grad_norm(C, DEV, n, None, 1.0, flag0=1)          # a flag already 1 stays 1


@pytest.mark.parametrize("n", SC.GN_N)
def test_grad_norm_flags_non_finite(C, n):
    """NaN, +-inf, a finite g whose scaled value overflows, inf * 0: first, middle, last element"""
    for val, gs in SC.GN_POISON:
        for where in sorted({0, n // 2, n - 1}):
            SC.run_grad_norm(C, DEV, n, None, gs, val, where)


@pytest.mark.parametrize("n", SC.CAST_N)
def test_cast_bf16(C, n):
    for first in range(len(SC.CAST_SPECIALS) if n == 1 else 1):
        SC.run_cast(C, DEV, n, first)


# ------------------------------------------------------------------------------ csrc/quant.hip
_QID = lambda s: "x".join(map(str, s))      # noqa: E731


@pytest.mark.parametrize("sh", SC.Q_SHAPES, ids=_QID)
def test_quant(C, sh):
    """bitwise the fp32 steps, within half an e4m3 step in fp64, zero padding, the amax element at
    either end with either sign, an all-zero operand, the direction-sum form"""
    for variant in SC.Q_VARIANTS:
        SC.run_quant(C, DEV, sh, variant)


@pytest.mark.parametrize("sh", SC.Q_SHAPES, ids=_QID)
def test_quant_direction_sum_is_the_unfused_call(C, sh):
    a, b, a2 = SC.quant_operands(sh, "sum")
    a8, b8, sc, asum = SC.run_quant(C, DEV, sh, "sum")
    s = torch.add(a, a2)
    SC.check_bits("asum", asum, s.view(torch.int16).reshape(-1))
    u8, v8, usc, _ = SC.run_quant(C, DEV, sh, "sum, unfused", ops=(s, b, None))
    for k, x, y in (("a8", a8, u8), ("b8", b8, v8), ("scales", sc, usc)):
        SC.check_bits("direction sum against the unfused call: " + k, x, y)


@pytest.mark.parametrize("variant", SC.Q_NONFINITE)
@pytest.mark.parametrize("sh", SC.Q_SHAPES, ids=_QID)
def test_quant_non_finite(C, sh, variant):
    """A NaN element is stored as an e4m3 NaN byte, everything else and the scale as if it were
    zero; an infinite element does not dequantise to a finite value. Before the select in
    quant2_kernel the first of these failed with
      fp8_quant2 1x8, 1x8 -> Kp 8, nan a: a: the NaN at [0, 4] was stored as byte 0xFE (-448,
      dequantised -3.5), want an e4m3 NaN"""
    SC.run_quant(C, DEV, sh, variant)


# ------------------------------------------------------------------------------ csrc/reduce.hip
@pytest.mark.parametrize("jobs", SC.CS_CASES, ids=lambda j: "+".join("%dx%dx%d%s" % (x[0], x[1], x[2], "a" if x[3] else "") for x in j))
def test_col_sum(C, jobs):
    SC.run_col_sum(C, DEV, jobs)


@pytest.mark.parametrize("M", SC.FC_M)
def test_fc_bias_grad(C, M):
    for m, K, ldg, acc in SC.fc_cases():
        if m == M:
            SC.run_fc_bias(C, DEV, M, K, ldg, acc)


# ------------------------------------------------------------------------------ csrc/fill.hip
def test_multi_fill(C):
    for regs in SC.mf_cases():
        SC.run_multi_fill(C, DEV, regs)


def test_multi_copy(C):
    for pairs, ns in SC.MC_CASES:
        SC.run_multi_copy(C, DEV, pairs, ns)


@pytest.mark.parametrize("n", SC.PREP_N)
def test_prep_inputs(C, n):
    SC.run_prep(C, DEV, n, 3)
    SC.run_prep(C, DEV, n, len(SC.PREP_LENS))


@pytest.mark.parametrize("nl", SC.PREP_NL)
def test_prep_inputs_more_lengths_than_feature_groups(C, nl):
    """n = 8 features: a grid sized from n / 4 alone has 256 threads and left lens_out[256:]
    unwritten"""
    SC.run_prep(C, DEV, 8, nl)


@pytest.mark.parametrize("R", SC.TR_SIZES)
def test_transpose_bf16(C, R):
    for Cc in SC.TR_SIZES:
        SC.run_transpose(C, DEV, R, Cc)


# ------------------------------------------------------------------------------ host refusals
def test_host_refusals(C):
    """every call the bindings must refuse raises before anything is launched: the buffers are
    bit-identical afterwards"""
    for name, thunk, bufs in SC.refusals(C, DEV):
        SC.run_refusal(name, thunk, bufs)
    torch.cuda.synchronize()
