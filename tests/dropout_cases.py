"""Shared cases and helpers of tests/test_dropout.py (CPU) and tests/test_dropout_gpu.py.

The definition under test is the docstring of deepspeech_amd/ops/dropout.py; the oracle is
ops/reference.py seq_dropout_mask_ref / seq_dropout_ref (vectorised numpy over philox4x32), itself
checked against ``scalar_keep`` below, a pure-Python evaluation of the definition one element at
a time.

SHAPES: the smallest [T, N, H] that exercise a single group (1, 1, 8), rows that are not 64-byte
multiples (3, 2, 40), several workgroups per row (5, 2, 1280 and 2, 1, 2048: 160 and 256 groups
against 256 lanes per workgroup), the headline row width (67, 3, 800) and a group count that is
no multiple of the workgroup size (33, 5, 264: 5445 groups).

PARAMS: the full cross of thr {1, 13107, 32768, 65535}, both modes, sites {0, 9}, steps
{0, 7, 2^31 + 5} and first_utt {0, 0xfffffffe (wraps inside a batch)}: 96 launches per shape,
each a few microseconds against a numpy oracle of at most 20100 Philox blocks.

COUNTS: dropped counts of the oracle at seed 1234, step 7, first_utt 0, site 2; the test bound
is 4 sigma of the binomial n * p * (1 - p) around n * thr / 65536.
"""
import torch

from deepspeech_amd.ops import reference as R

SEED = 1234
SHAPES = [(1, 1, 8), (3, 2, 40), (5, 2, 1280), (67, 3, 800), (2, 1, 2048), (33, 5, 264)]
THRS = [1, 13107, 32768, 65535]
# (thr, locked, site, step, first_utt)
PARAMS = [(thr, locked, site, step, fu) for thr in THRS for locked in (False, True) for site in (0, 9)
          for step in (0, 7, 2 ** 31 + 5) for fu in (0, 0xfffffffe)]
COUNTS = [((16, 4, 64), 16384, 1054), ((67, 3, 800), 13107, 32434), ((5, 2, 40), 32768, 219),
          ((241, 32, 800), 6554, 617209)]
KNOWN = ((0, 1, 2, 0x80020003), (1234, 0), (3005091373, 1805019942, 3854824497, 3968262615))


def ident(p):
    return "-".join(str(int(v)) for v in p)


def scalar_keep(t, b, i, seed, step, first_utt, site, thr, locked):
    """The definition for one element, Python integers only."""
    g, e = i >> 3, i & 7
    ctr = (0 if locked else t, (first_utt + b) % 2 ** 32, step % 2 ** 32,
           0x80000000 | (int(locked) << 30) | (site << 16) | g)
    x = R.philox4x32(ctr, (seed & 0xffffffff, seed >> 32))
    return ((x[e >> 1] >> (16 * (e & 1))) & 0xffff) >= thr


def inputs(shape, seed=0, dtype=torch.bfloat16):
    """Values of every magnitude a hidden state takes, some exactly zero, both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 5, shape, generator=g).float())
    x[torch.rand(shape, generator=g) < 0.05] = 0.0
    return x.to(dtype)


def oracle(x, thr, locked, site, step, first_utt, seed=SEED):
    """seq_dropout_ref on the CPU, in x's dtype."""
    return R.seq_dropout_ref(x.detach().cpu(), seed, step, first_utt, site, thr, locked)


def same_bits(a, b):
    """Bitwise equality (NaNs included) of two tensors of one dtype."""
    ity = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().contiguous().view(ity),
                                                                     b.cpu().contiguous().view(ity))
