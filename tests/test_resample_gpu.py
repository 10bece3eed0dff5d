"""The resampling kernel (csrc/resample.hip) per element against the fp64 oracle
(ops/reference.py resample_ref), its edges, its bitwise invariances, graph capture, and the
wiring through AudioFeaturizer, StreamingRecognizer and Aligner.

Bound, for every output with A = sum_k |h[ph, k] x[.]| taken from the oracle:
|y - y64| <= (2K + 2) 2^-24 A, the standard forward bound of a K-term fp32 dot product with a
once-rounded table (tests/test_resample.py derives it); where A is 0 the output is exactly 0.
No element is left out. Shapes are the smallest that reach every path: B = 3, rows up to three
tiles of TILE_OUT outputs, row lengths at the filter's half width and at the tile edges, an
odd buffer width so that row 0 takes the 16-byte staging and rows 1 and 2 the scalar one.
"""
import functools

import numpy as np
import pytest
import torch

from deepspeech_amd.ops import featurize as FZ
from deepspeech_amd.ops import reference as REF
from deepspeech_amd.ops import resample as RS

pytestmark = pytest.mark.gpu

RATES = [8000, 24000, 22050, 44100, 48000]
DTYPES = ["fp32", "int16"]


def samples_for(n_out, L, M):
    """A row length whose output count is n_out (the next reachable count when upsampling)."""
    return ((n_out - 1) * M) // L + 1


def wave(B, S, seed, rate):
    rng = np.random.RandomState(seed)
    t = np.arange(S) / float(rate)
    return np.stack([9000.0 * np.sin(2 * np.pi * (200 + 700 * (b + 1) * t) * t) + 300.0 * rng.randn(S)
                     for b in range(B)])


@functools.lru_cache(maxsize=None)
def case(rate, dtype):
    """Nine rows of one buffer width (three calls of B = 3), their lengths and the oracle,
    computed once and shared: (x [9, S], lens, y64, a64, L, M, K)."""
    L, M, K, _ = REF.resample_table(rate, 16000)
    T = RS.TILE_OUT
    S = samples_for(2 * T + 77, L, M) | 1                       # three tiles, odd width
    lens = [S, 1, K // 2 - 1,
            K // 2, samples_for(T - 1, L, M), K // 2 + 1,
            samples_for(T, L, M), samples_for(T + 1, L, M), S - 1]
    x = wave(9, S, rate, rate)
    x = np.round(x).astype(np.int16) if dtype == "int16" else x.astype(np.float32)
    y64, a64 = REF.resample_ref(x, rate, 16000, lens=lens, return_abs=True)
    for a in (y64, a64):                                        # shared: left unchanged
        a.setflags(write=False)
    return x, lens, y64, a64, L, M, K


def check_bound(y, y64, a64, K):
    y = y.double().cpu().numpy()
    bound = (2 * K + 2) * 2.0 ** -24 * a64
    err = np.abs(y - y64)
    if (bound > 0).any():
        print("max error / bound = %.4f" % float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.isfinite(y).all()
    assert (err <= bound).all()
    assert not y[bound == 0].any()


def planted(x, lens, dtype, dev):
    """x on the device with NaN (fp32) or full-scale garbage (int16) at and past each row's length."""
    t = torch.from_numpy(x.copy())
    for b, n in enumerate(lens):
        t[b, n:] = float("nan") if dtype == "fp32" else 32767
    return t.to(dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rate", RATES)
def test_every_element_against_the_oracle(cuda, rate, dtype):
    x, lens, y64, a64, L, M, K = case(rate, dtype)
    rs = RS.Resampler(rate, device=cuda)
    assert rs.use_kernel
    S = x.shape[1]
    for g in range(0, 9, 3):
        ln = lens[g:g + 3]
        y, out_lens = rs(planted(x[g:g + 3], ln, dtype, cuda), torch.tensor(ln, dtype=torch.int32))
        assert y.dtype == torch.float32 and y.shape == (3, REF.resample_out_len(S, L, M))
        assert y.shape[1] > 2 * RS.TILE_OUT                     # three tiles
        counts = [REF.resample_out_len(n, L, M) for n in ln]
        assert out_lens.dtype == torch.int32 and out_lens.tolist() == counts
        check_bound(y, y64[g:g + 3], a64[g:g + 3], K)
        for b, n in enumerate(counts):
            assert not y[b, n:].any()                           # padding columns: exact zeros
            assert not torch.signbit(y[b, n:]).any()
    # the lengths put a row's last output one before, on and one after the first tile boundary
    ends = [REF.resample_out_len(lens[i], L, M) for i in (4, 6, 7)]
    assert ends[0] <= RS.TILE_OUT <= ends[1] < ends[2] <= RS.TILE_OUT + L


@pytest.mark.parametrize("rate", RATES)
def test_no_lens_is_the_full_width(cuda, rate):
    x, lens, y64, a64, L, M, K = case(rate, "fp32")
    y, out_lens = RS.Resampler(rate, device=cuda)(torch.from_numpy(x[:1]).to(cuda))
    assert out_lens.tolist() == [y.shape[1]]
    check_bound(y, y64[:1], a64[:1], K)                         # row 0 is a full row


@pytest.mark.parametrize("rate", RATES)
def test_a_row_alone_equals_the_row_in_a_batch(cuda, rate):
    x, lens, *_ = case(rate, "fp32")
    rs = RS.Resampler(rate, device=cuda)
    xb = torch.from_numpy(x[6:9]).to(cuda)
    ln = torch.tensor(lens[6:9], dtype=torch.int32)
    y, n = rs(xb, ln)
    for b in range(3):
        y1, n1 = rs(xb[b:b + 1].clone(), ln[b:b + 1])
        assert torch.equal(y1[0], y[b]) and int(n1[0]) == int(n[b])


@pytest.mark.parametrize("rate", RATES)
def test_int16_equals_the_same_values_as_fp32(cuda, rate):
    x, lens, *_ = case(rate, "int16")
    rs = RS.Resampler(rate, device=cuda)
    ln = torch.tensor(lens[:3], dtype=torch.int32)
    xi = torch.from_numpy(x[:3]).to(cuda)
    yi, ni = rs(xi, ln)
    yf, nf = rs(xi.float(), ln)
    assert torch.equal(yi, yf) and torch.equal(ni, nf)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rate", RATES)
def test_stream_is_bitwise_the_whole_call(cuda, rate, dtype):
    L, M, K, _ = REF.resample_table(rate, 16000)
    rs = RS.Resampler(rate, device=cuda)
    sizes = (1, 7, K // 2, 441, 1023, 2048)
    head = sum(sizes)
    end = [600, 333, 1]                                         # valid samples of the last push
    x = wave(3, head + 600, rate + 1, rate)
    xt = torch.from_numpy(np.round(x).astype(np.int16) if dtype == "int16" else x.astype(np.float32)).to(cuda)
    whole, whole_lens = rs(xt, torch.tensor([head + e for e in end], dtype=torch.int32))
    st, got, at = rs.stream(3), [], 0
    for n in sizes:
        got.append(st.push(xt[:, at:at + n]))
        at += n
        assert st.emitted == REF.resample_emitted(at, L, M, K) == sum(g.shape[1] for g in got)
    before = st.emitted
    got.append(st.push(xt[:, at:], final=True, lens=end))
    got = torch.cat(got, 1)
    assert got.shape == whole.shape and torch.equal(got, whole)
    assert torch.equal(st.last_lens, whole_lens - before)


@pytest.mark.parametrize("rate", RATES)
def test_kernel_and_composite_agree_within_the_bound(cuda, rate):
    """The composite rounds each product and each sum (torch.mul, torch.add), the kernel once per
    fma, so they are not bitwise equal by construction: both lie within the bound of the oracle,
    hence within twice the bound of each other."""
    x, lens, y64, a64, L, M, K = case(rate, "fp32")
    rs = RS.Resampler(rate, device=cuda)
    xt = torch.from_numpy(x[3:6]).to(cuda)
    ln = torch.tensor(lens[3:6], dtype=torch.int32, device=cuda)
    y, n = rs(xt, ln)
    yc, nc = RS.resample_composite(xt, ln, rs.h, L, M, -(K // 2 - 1), 0, y.shape[1], True)
    assert torch.equal(n, nc)
    check_bound(yc, y64[3:6], a64[3:6], K)
    bound = torch.from_numpy(2 * (2 * K + 2) * 2.0 ** -24 * a64[3:6]).to(cuda)
    assert ((y.double() - yc.double()).abs() <= bound).all()


def test_out_of_contract_rate_takes_the_composite(cuda):
    for rate in (8000, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000):
        assert RS.Resampler(rate, device=cuda).use_kernel
    rs = RS.Resampler(11025, device=cuda)                       # L K = 30720 table words
    assert not rs.use_kernel
    x = wave(2, 1500, 4, 11025).astype(np.float32)
    y, n = rs(x, [1500, 700])
    y64, a64 = REF.resample_ref(x, 11025, 16000, lens=[1500, 700], return_abs=True)
    assert y.device.type == "cuda" and n.tolist() == [REF.resample_out_len(s, rs.L, rs.M) for s in (1500, 700)]
    check_bound(y, y64, a64, rs.K)


def test_graph_capture_replays_on_new_audio(cuda):
    x, lens, *_ = case(48000, "fp32")
    rs = RS.Resampler(48000, device=cuda)
    first = torch.from_numpy(x[:2]).to(cuda)
    other = torch.from_numpy(x[7:9]).to(cuda)
    ln = torch.tensor([x.shape[1], 3000], dtype=torch.int32, device=cuda)
    rs(first, ln)                                               # warm: table uploaded, kernel loaded
    static = first.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, out_lens = rs(static, ln)
    static.copy_(other)
    g.replay()
    want, want_lens = rs(other, ln)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out_lens, want_lens)
    assert out_lens.tolist() == [REF.resample_out_len(x.shape[1], 1, 3), 1000]
    assert not out[1, 1000:].any()


@pytest.mark.parametrize("normalize", ["utterance", "fixed"])
@pytest.mark.parametrize("kind", ["mfcc", "spectrogram"])
def test_featurizer_input_rate_is_resample_then_featurize(cuda, kind, normalize):
    x, *_ = case(48000, "int16")
    pcm = torch.from_numpy(x[:2])
    lens = [x.shape[1], 4000]
    got, frames = FZ.AudioFeaturizer(kind, device=cuda, normalize=normalize, input_rate=48000)(pcm, lens)
    # the default fixed gain follows the int16 input; the resampled signal is fp32
    fz = FZ.AudioFeaturizer(kind, device=cuda, normalize=normalize, gain=1.0 / 32768.0)
    want, want_frames = fz(*RS.Resampler(48000, device=cuda)(pcm, lens))
    assert torch.equal(got, want) and torch.equal(frames, want_frames)
    assert frames.tolist() == [FZ.num_frames(REF.resample_out_len(n, 1, 3), kind) for n in lens]
    assert got.abs().max() > 1


@pytest.mark.parametrize("kind", ["mfcc", "spectrogram"])
def test_feature_stream_with_input_rate_equals_its_whole_call(cuda, kind):
    x, *_ = case(48000, "int16")
    pcm = torch.from_numpy(x[:2])
    fz = FZ.AudioFeaturizer(kind, device=cuda, normalize="fixed", input_rate=48000)
    whole, frames = fz(pcm)
    st, got, at = fz.stream(2), [], 0
    for n in (1, 71, 72, 1500, 2999):
        got.append(st.push(pcm[:, at:at + n]))
        at += n
    got.append(st.push(pcm[:, at:], final=True))
    got = torch.cat(got, 1)
    assert got.shape == whole.shape and torch.equal(got, whole)


def small_model(cuda):
    from deepspeech_amd.models import DeepSpeech2
    torch.manual_seed(3)
    m = DeepSpeech2(num_filters=32, num_hidden=256, num_rnn_layers=2, cell="gru", bidirectional=False).to(cuda)
    m.set_engine("hip", torch.bfloat16)
    return m.eval()


def test_recognizer_accepts_48k_audio(cuda):
    from deepspeech_amd.infer import StreamingRecognizer
    from deepspeech_amd.ops import rnn as RNN
    m = small_model(cuda)
    B, n, step = 2, 72000, 24000                                # 1.5 s in 0.5 s chunks
    pcm = torch.from_numpy(np.round(wave(B, n, 60, 48000)).astype(np.int16))
    feats, frames = FZ.AudioFeaturizer("mfcc", device=cuda, normalize="fixed", input_rate=48000)(pcm)
    assert frames.tolist() == [FZ.num_frames(n // 3)] * B
    a = StreamingRecognizer(m, batch=B, audio_rate=48000)
    b = StreamingRecognizer(m, batch=B)
    done = 0
    for s in range(0, n, step):
        a.accept_audio(pcm[:, s:s + step], final=s + step >= n)
        new = a.total - done
        b.accept(feats[:, done:done + new])
        done += new
    assert done == feats.shape[1]
    RNN.check_errors()
    got, want = torch.cat(a.logprobs, 0), torch.cat(b.logprobs, 0)
    assert got.shape == want.shape and got.shape[0] > 0
    assert torch.allclose(got, want, atol=2e-4), (got - want).abs().max()
    assert a.finish() == b.finish()


def test_align_audio_resamples_8k(cuda):
    from deepspeech_amd.align import Aligner
    m = small_model(cuda)
    n = 12000                                                   # 1.5 s at 8 kHz
    pcm = torch.from_numpy(np.round(wave(2, n, 80, 8000)).astype(np.int16))
    texts = ["ab c", "hello world"]
    got = Aligner(m).align_audio(pcm, texts, sample_rate=8000, resample=True)
    feats, frames = FZ.AudioFeaturizer("mfcc", device=cuda)(*RS.Resampler(8000, device=cuda)(pcm))
    assert frames.tolist() == [FZ.num_frames(2 * n)] * 2
    want = Aligner(m).align(feats.float(), frames, texts, durations=[n / 8000.0] * 2)
    assert len(got) == 2 and all(u.feasible for u in got)
    for g, w in zip(got, want):
        assert g.score == w.score and g.frames == w.frames
        assert g.words == w.words                               # text, start_s, end_s, confidence
        assert g.words and g.words[-1].end_s <= n / 8000.0 + 1e-9
