"""Shallow LM fusion in the GPU prefix beam search (csrc/beam.hip ctc_beam_kernel<true>) against
the native host decoder with the same LM (runtime/decoder.cpp, itself checked against a brute-force
path sum in tests/test_beam_lm.py): same hypotheses and scores in both final modes, chunked
feeding bitwise equal to whole feeding, and the streaming recogniser end to end."""
import numpy as np
import pytest
import torch

from deepspeech_amd.lm import CharNgramLM, synthetic_corpus

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.8, 0.5
_LMS = {}


def _lm(order):
    if order not in _LMS:
        _LMS[order] = CharNgramLM.train(synthetic_corpus(150, seed=3), order)
    return _LMS[order]


def _lp(T, B, K, sharp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(sharp * torch.randn(T, B, K, generator=g), -1)


def _host(lp, lens, W, blank, prune, lm, final):
    from deepspeech_amd.ops.decode import host_lm
    from deepspeech_amd.runtime import native
    N = native.load()
    L = host_lm(lm, ALPHA, BETA, blank)
    out = []
    for b in range(lp.shape[1]):
        bs = N.PrefixBeamSearch(W, blank, prune, L)
        bs.feed(lp[: int(lens[b]), b].contiguous().numpy())
        out.append(bs.results(final))
    return out


def _same(got, want, B):
    for b in range(B):
        assert len(got[b]) == len(want[b]), b
        assert got[b][0][0] == want[b][0][0], (b, got[b][0], want[b][0])
        g = sorted(s for _, s in got[b])
        h = sorted(s for _, s in want[b])
        np.testing.assert_allclose(g, h, rtol=2e-5, atol=2e-5)
        assert {tuple(p) for p, _ in got[b]} == {tuple(p) for p, _ in want[b]}


@pytest.mark.parametrize("order", [1, 3, 6])
@pytest.mark.parametrize("W", [1, 8, 16, 32])
def test_gpu_lm_beam_matches_host(cuda, W, order):
    from deepspeech_amd.ops.decode import GpuBeamSearch
    T, B, K, blank = 60, 6, 29, 28
    lm = _lm(order)
    lp = _lp(T, B, K, 2.0, seed=100 * order + W)
    lens = torch.tensor([60, 41, 1, 60, 17, 33], dtype=torch.int32)
    gs = GpuBeamSearch(B, W, blank, -10.0, cuda, frames_hint=8, lm=lm, lm_weight=ALPHA, label_bonus=BETA)
    gs.feed(lp.to(cuda), lens.to(cuda))
    for final in (False, True):
        got = gs.results(final)
        for r in got:
            assert [s for _, s in r] == sorted((s for _, s in r), reverse=True)
        _same(got, _host(lp, lens, W, blank, -10.0, lm, final), B)


def test_gpu_lm_beam_small_alphabet_blank_zero(cuda):
    from deepspeech_amd.ops.decode import GpuBeamSearch
    T, B, K, blank = 30, 3, 5, 0
    rng = np.random.default_rng(4)
    data = [rng.integers(1, K, size=int(rng.integers(1, 10))).tolist() for _ in range(60)]
    lm = CharNgramLM.train(data, 3, alphabet="ABCD", blank=0)
    lp = _lp(T, B, K, 2.0, seed=9)
    lens = torch.tensor([30, 1, 19], dtype=torch.int32)
    gs = GpuBeamSearch(B, 8, blank, -10.0, cuda, frames_hint=8, lm=lm, lm_weight=ALPHA, label_bonus=BETA)
    gs.feed(lp.to(cuda), lens.to(cuda))
    for final in (False, True):
        _same(gs.results(final), _host(lp, lens, 8, blank, -10.0, lm, final), B)


def test_gpu_lm_beam_chunked_equals_whole(cuda):
    """Streaming: the LM state is carried between launches like the rest of the beam state."""
    from deepspeech_amd.ops.decode import GpuBeamSearch
    T, B, K, blank = 80, 4, 29, 28
    lm = _lm(3)
    kw = dict(lm=lm, lm_weight=ALPHA, label_bonus=BETA)
    lp = _lp(T, B, K, 2.0, seed=7).to(cuda)
    whole = GpuBeamSearch(B, 16, blank, -10.0, cuda, frames_hint=T, **kw)
    whole.feed(lp)
    parts = GpuBeamSearch(B, 16, blank, -10.0, cuda, frames_hint=4, **kw)
    t = 0
    for n in (1, 13, 7, 13, 13, 2, 13, 13, 5):
        parts.feed(lp[t:t + n])
        t += n
    assert t == T
    assert whole.results() == parts.results()
    assert whole.results(final=True) == parts.results(final=True)
    assert torch.equal(whole.lmstate, parts.lmstate)
    plain = GpuBeamSearch(B, 16, blank, -10.0, cuda, frames_hint=T)
    plain.feed(lp)
    assert plain.best() != whole.best()                      # the LM is not a no-op here
    assert plain.results(final=True) == plain.results()      # and no LM has no final term
    parts.reset()
    parts.feed(lp)
    assert parts.best() == whole.best()
    assert parts.best(final=True) == whole.best(final=True)


def test_streaming_recognizer_with_lm(cuda):
    """finish() is beam_decode over the stream's stored log-probs with the same LM (both use the
    end-of-sentence term), and finish_timed() aligns that transcript into words."""
    from deepspeech_amd.infer import StreamingRecognizer
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.ops.decode import beam_decode
    torch.manual_seed(0)
    m = DeepSpeech2(num_filters=32, num_hidden=128, num_rnn_layers=2, cell="gru", bidirectional=False).to(cuda)
    m.set_engine("hip", torch.bfloat16)
    lm = _lm(3)
    rec = StreamingRecognizer(m, decoder="beam", beam_width=16, batch=2, lm=lm, lm_weight=ALPHA, label_bonus=BETA)
    assert rec.gbeams is not None and rec.gbeams.lm is not None
    feats = torch.randn(2, 50 * 6 + 38, m.freq_bins, device=cuda)
    for i in range(0, feats.shape[1], 50):
        rec.accept(feats[:, i:i + 50])
    got = rec.finish()
    lp = torch.cat(rec.logprobs, 0)
    lens = torch.full((2,), lp.shape[0], dtype=torch.int32)
    assert got == beam_decode(lp, lens, 16, lm=lm, lm_weight=ALPHA, label_bonus=BETA)
    assert got == rec.gbeams.best(final=True)
    assert all(len(g) > 0 for g in got)
    words = rec.finish_timed()
    assert len(words) == 2 and all(len(w) > 0 for w in words)
