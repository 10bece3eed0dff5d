"""CTC forced alignment on the GPU (csrc/align.hip) against the oracle
(ops/reference.py ctc_viterbi_ref): bitwise scores and identical paths / spans on log-prob
inputs for every register-tile width, forced ties, bf16, logits input, infeasible rows, graph
capture and the streaming recogniser's finish_timed()."""
import math

import numpy as np
import pytest
import torch

from align_cases import collapse, labels_no_repeat, pad_labels, path_score, quantised_lp, random_lp

from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops.align import Alignment, ctc_forced_align

pytestmark = pytest.mark.gpu

K, BLANK = 29, 28

# Logits input: the bound is 4x the largest difference observed on the inputs of
# test_logits_input (profiles/align.md). Observed: 0 for the score and for the rescored path, fp32
# and bf16, i.e. below what an fp32 score resolves; so "observed" is taken as that resolution, one
# ulp of the score (2^-23 relative), and the bound is 4 ulp of the oracle's score. That is 1 / 200
# of the rtol = atol = 1e-4 tests/test_kernels_gpu.py grants the same log-softmax arithmetic.
LOGITS_RTOL = 4 * 2.0 ** -23


def _rows(seed):
    """Label rows of lengths [20, 2, 1, 0, 33, 5]: the 33 without adjacent repeats (it fills its
    33 frames: no blank fits), the 5 with adjacent repeats."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, BLANK, size=20).tolist(), [3, 7], [11], [], labels_no_repeat(rng, 33, K, BLANK),
            [4, 4, 9, 9, 9]]
    return rows


LENS = [70, 65, 64, 1, 33, 70]


def _same(got: Alignment, want: Alignment, paths: bool = True):
    g = Alignment(*[t.cpu() for t in got])
    assert g.score.numpy().tobytes() == want.score.numpy().tobytes(), (g.score, want.score)
    if paths:
        assert torch.equal(g.path, want.path)
        assert torch.equal(g.tok_start, want.tok_start) and torch.equal(g.tok_end, want.tok_end)
        torch.testing.assert_close(g.tok_score, want.tok_score, rtol=1e-5, atol=0.0)


def _both(lp_dev_input, lp_oracle, lens, rows, log_probs=True):
    lab, ll = pad_labels(rows)
    lens = torch.tensor(lens, dtype=torch.int32)
    want = Alignment(*R.ctc_viterbi_ref(lp_oracle, lens, lab, ll, BLANK))
    got = ctc_forced_align(lp_dev_input, lens.to(lp_dev_input.device), lab.to(lp_dev_input.device),
                           ll.to(lp_dev_input.device), BLANK, log_probs=log_probs)
    assert all(t.device == lp_dev_input.device for t in got)
    return got, want


def test_exact_against_oracle(cuda):
    """Crosses a lane boundary (2L+1 = 41 and 67 > SPL = 4), the 64-frame staging boundary (65
    against 64), len < T, the empty lattice (L = 0 in one frame) and the no-blank lattice."""
    lp = random_lp(70, 6, K, seed=1)
    rows = _rows(0)
    got, want = _both(lp.to(cuda), lp, LENS, rows)
    _same(got, want)
    w = want
    assert all(math.isfinite(s) for s in w.score.tolist())
    assert w.path[3].tolist() == [BLANK] + [-1] * 69
    assert BLANK not in w.path[4, :33].tolist() and collapse(w.path[4, :33].tolist(), BLANK) == rows[4]
    assert collapse(w.path[5].tolist(), BLANK) == rows[5]


@pytest.mark.parametrize("L,spl", [(127, 4), (159, 5), (191, 6), (255, 8), (383, 12), (511, 16), (1023, 32)])
def test_every_register_tile_width(cuda, L, spl):
    """2L+1 = 255 .. 2047 states: one case per instantiated SPL (csrc/align.hip align_spl); the
    last one packs its back-pointers into two words per lane and frame."""
    assert (2 * L + 1 + 63) // 64 <= spl
    rng = np.random.default_rng(L)
    T = L + 8
    rows = [labels_no_repeat(rng, L, K, BLANK), rng.integers(0, BLANK, size=L // 2).tolist()]
    lp = random_lp(T, 2, K, seed=L, sharp=1.0)
    got, want = _both(lp.to(cuda), lp, [T, T - 3], rows)
    assert all(math.isfinite(s) for s in want.score.tolist())
    _same(got, want)


def test_forced_ties(cuda):
    lp = quantised_lp(70, 6, K, seed=3)
    rows = _rows(1)
    got, want = _both(lp.to(cuda), lp, LENS, rows)
    _same(got, want)
    # and the hand-written case of tests/test_align.py
    flat = torch.full((5, 1, 3), -0.5)
    lab, ll = pad_labels([[0, 1]])
    a = ctc_forced_align(flat.to(cuda), torch.tensor([5], dtype=torch.int32), lab, ll, 2, log_probs=True)
    assert a.path.cpu()[0].tolist() == [0, 1, 2, 2, 2] and a.score.item() == -2.5


def test_bf16_log_probs(cuda):
    lp16 = random_lp(70, 6, K, seed=4).to(torch.bfloat16)
    got, want = _both(lp16.to(cuda), lp16.float(), LENS, _rows(2))
    _same(got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logits_input(cuda, dtype):
    g = torch.Generator().manual_seed(6)
    x = (3.0 * torch.randn(70, 6, K, generator=g)).to(dtype)
    lp = torch.log_softmax(x.float(), -1)
    rows = _rows(3)
    got, want = _both(x.to(cuda), lp, LENS, rows, log_probs=False)
    gs, ws = got.score.cpu().double(), want.score.double()
    path = got.path.cpu()
    # the kernel's own path scored with the torch log-probs, in the recursion's fp32 order
    rescored = torch.tensor([float(path_score(lp[:, b].numpy(), path[b, : LENS[b]].tolist())) for b in range(6)],
                            dtype=torch.float64)
    print("align logits %s: max |score - oracle| = %.3e (%.3e relative), max |rescored path - oracle| = %.3e, "
          "paths equal %s, scores %s"
          % (dtype, (gs - ws).abs().max().item(), ((gs - ws).abs() / ws.abs()).max().item(),
             (rescored - ws).abs().max().item(), torch.equal(path, want.path), ws.tolist()))
    for b in range(6):
        assert collapse(path[b, : LENS[b]].tolist(), BLANK) == rows[b]
        assert (path[b, LENS[b]:] == -1).all()
    np.testing.assert_allclose(gs.numpy(), ws.numpy(), rtol=LOGITS_RTOL, atol=0.0)
    np.testing.assert_allclose(rescored.numpy(), ws.numpy(), rtol=LOGITS_RTOL, atol=0.0)


def _raw_call(cuda, lp, lens, rows, margin=0, fill=0x5A, width=0):
    """The binding on output views cut out of sentinel-filled buffers with a margin either side."""
    from deepspeech_amd.ops import _ext
    C = _ext.ext()
    T, N, _ = lp.shape
    lab, ll = pad_labels(rows, width)
    Lmax = lab.shape[1]

    def buf(n, dtype):
        b = torch.full((n + 2 * margin,), fill, dtype=torch.uint8, device=cuda).repeat_interleave(4).view(dtype)
        return b, b[margin: margin + n]

    bufs = [buf(N * T, torch.int32), buf(N * Lmax, torch.int32), buf(N * Lmax, torch.int32),
            buf(N * Lmax, torch.float32), buf(N, torch.float32)]
    shapes = [(N, T), (N, Lmax), (N, Lmax), (N, Lmax), (N,)]
    views = [v.view(s) for (_, v), s in zip(bufs, shapes)]
    ws = torch.empty(int(C.ctc_align_ws_bytes(T, N, Lmax)), device=cuda, dtype=torch.uint8)
    C.ctc_align(lp.to(cuda).contiguous(), torch.tensor(lens, dtype=torch.int32, device=cuda), lab.to(cuda),
                ll.to(cuda), *views, ws, BLANK, True)
    torch.cuda.synchronize()
    return Alignment(*[v.cpu().clone() for v in views]), [b for b, _ in bufs]


def test_infeasible_rows_inside_a_feasible_batch(cuda):
    lp = random_lp(70, 5, K, seed=7)
    rows = [_rows(4)[0], [5, 5, 6], _rows(4)[4], [1, 2, 3], [8]]
    lens = [70, 3, 20, 0, 44]      # row 1: 3 labels + 1 repeat in 3 frames; row 2: 33 labels in 20; row 3: no frames
    margin = 64
    got, bufs = _raw_call(cuda, lp, lens, rows, margin)
    for b in (1, 2, 3):
        assert got.score[b] == -math.inf
        assert (got.path[b] == -1).all() and (got.tok_start[b] == -1).all() and (got.tok_end[b] == -1).all()
    want = Alignment(*R.ctc_viterbi_ref(lp, torch.tensor(lens), *pad_labels(rows), BLANK))
    _same(got, want)
    # the feasible neighbours alone give the same outputs (same padded label width)
    keep = [0, 4]
    alone, _ = _raw_call(cuda, lp[:, keep], [lens[i] for i in keep], [rows[i] for i in keep], width=33)
    for i, b in enumerate(keep):
        for f in range(5):
            assert alone[f][i].numpy().tobytes() == got[f][b].numpy().tobytes(), (b, Alignment._fields[f])
    # canary margins untouched
    for big in bufs:
        raw = big.view(torch.uint8).cpu()
        assert (raw[: 4 * margin] == 0x5A).all() and (raw[-4 * margin:] == 0x5A).all()


def test_nan_frame_gives_nan_score(cuda):
    """A NaN inside an utterance's valid frames makes its score NaN (as it makes the CTC loss NaN)
    and leaves no path; a NaN past the length, or in a neighbour, changes nothing."""
    lp = random_lp(70, 3, K, seed=11)
    clean = lp.clone()
    lp[40, 1, 5] = float("nan")
    lp[69, 2, 0] = float("nan")
    rows, lens = [[1, 2, 3], [4, 5], [6, 6]], [70, 70, 60]
    got, want = _both(lp.to(cuda), lp, lens, rows)
    ref, _ = _both(clean.to(cuda), clean, lens, rows)
    g, r = Alignment(*[t.cpu() for t in got]), Alignment(*[t.cpu() for t in ref])
    assert math.isnan(g.score[1]) and math.isnan(want.score[1])
    assert (g.path[1] == -1).all() and (g.tok_start[1] == -1).all() and (g.tok_end[1] == -1).all()
    for b in (0, 2):
        for f in range(5):
            assert g[f][b].numpy().tobytes() == r[f][b].numpy().tobytes(), (b, Alignment._fields[f])
            if f != 3:
                assert g[f][b].numpy().tobytes() == want[f][b].numpy().tobytes(), (b, Alignment._fields[f])


def test_graph_capture(cuda):
    rows_a, rows_b = _rows(5), _rows(6)
    lp_a, lp_b = random_lp(70, 6, K, seed=8), random_lp(70, 6, K, seed=9)
    lens_a, lens_b = LENS, [64, 70, 2, 5, 40, 66]
    s_lp = torch.empty(70, 6, K, device=cuda)
    s_lens = torch.empty(6, dtype=torch.int32, device=cuda)
    lab0, ll0 = pad_labels(rows_a)
    s_lab, s_ll = torch.empty_like(lab0, device=cuda), torch.empty_like(ll0, device=cuda)

    def load(lp, lens, rows):
        lab, ll = pad_labels(rows)
        s_lp.copy_(lp); s_lens.copy_(torch.tensor(lens, dtype=torch.int32)); s_lab.copy_(lab); s_ll.copy_(ll)

    load(lp_a, lens_a, rows_a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctc_forced_align(s_lp, s_lens, s_lab, s_ll, BLANK, log_probs=True)      # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ctc_forced_align(s_lp, s_lens, s_lab, s_ll, BLANK, log_probs=True)
    for lp, lens, rows in ((lp_b, lens_b, rows_b), (lp_a, lens_a, rows_a)):
        load(lp, lens, rows)
        graph.replay()
        torch.cuda.synchronize()
        replayed = Alignment(*[t.cpu().clone() for t in out])
        eager = ctc_forced_align(lp.to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda),
                                 *[t.to(cuda) for t in pad_labels(rows)], BLANK, log_probs=True)
        for f in range(5):
            assert replayed[f].numpy().tobytes() == eager[f].cpu().numpy().tobytes(), Alignment._fields[f]
        _same(replayed, Alignment(*R.ctc_viterbi_ref(lp, torch.tensor(lens), *pad_labels(rows), BLANK)))


@pytest.mark.parametrize("decoder", ["beam", "greedy"])
def test_finish_timed_on_the_hip_engine(cuda, decoder):
    from deepspeech_amd import align as A
    from deepspeech_amd.infer import StreamingRecognizer
    from deepspeech_amd.models import DeepSpeech2
    torch.manual_seed(0)
    m = DeepSpeech2(num_filters=32, num_hidden=128, num_rnn_layers=2, cell="gru", bidirectional=False).to(cuda)
    m.set_engine("hip", torch.bfloat16)
    rec = StreamingRecognizer(m, decoder=decoder, beam_width=16, batch=2)
    feats = torch.randn(2, 50 * 6 + 38, m.freq_bins, device=cuda)
    for i in range(0, feats.shape[1], 50):
        rec.accept(feats[:, i:i + 50])
    hyp = rec.finish()
    words = rec.finish_timed()
    assert all(len(h) > 0 for h in hyp)
    assert rec.alignment.path.device.type == "cuda"
    for b in range(2):
        assert "".join(w.text for w in words[b]) == A.ids_to_text(hyp[b]).replace(" ", "")
        t = 0.0
        for w in words[b]:
            assert 0.0 <= t <= w.start_s <= w.end_s <= feats.shape[1] * 0.01
            t = w.end_s
    lp = torch.cat(rec.logprobs, 0)                                   # [T2, B, K]
    path = rec.alignment.path.t().long()                              # [T2, B]
    assert math.isfinite(rec.alignment.score.sum().item())
    if decoder == "greedy":
        # the aligned path is the frame-wise argmax path: it reaches every frame's maximum, and
        # is the argmax itself wherever that is unique
        top2 = lp.topk(2, -1).values
        assert torch.equal(lp.gather(-1, path.unsqueeze(-1)).squeeze(-1), top2[..., 0])
        unique = top2[..., 0] > top2[..., 1]
        assert torch.equal(path[unique], lp.argmax(-1)[unique])
