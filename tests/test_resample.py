"""Resampling on the CPU: the definition's geometry and emission count, the quality of the fp64
oracle (ops/reference.py resample_ref), the torch composite against it, stream = whole call,
and the wiring through AudioFeaturizer and preprocessing.

Per-element bound of a fp32 evaluation against the oracle, for an output with
A = sum_k |h[ph, k] x[.]|: |y - y64| <= (2K + 2) 2^-24 A. It is the standard forward bound of a
K-term fp32 dot product: each coefficient is rounded to fp32 once (relative 2^-24), each product
once, each of the K - 1 sums once, so a term carries at most K + 1 roundings of 2^-24 and
(K + 1) 2^-24 (1 + o(1)) A bounds the error; 2K + 2 leaves the factor of two that covers the
second-order terms and the composite's separate product and sum. Where A is 0 every term is a
signed zero and the output must be exactly 0.
"""
import numpy as np
import pytest
import torch

from deepspeech_amd.ops import featurize as FZ
from deepspeech_amd.ops import reference as REF
from deepspeech_amd.ops import resample as RS

GEOMETRY = {8000: (2, 1, 48), 12000: (4, 3, 48), 22050: (320, 441, 68), 24000: (2, 3, 72),
            32000: (1, 2, 96), 44100: (160, 441, 134), 48000: (1, 3, 144), 88200: (80, 441, 266),
            96000: (1, 6, 288), 11025: (640, 441, 48)}


def pcm(B, S, seed, rate):
    """Chirp plus noise, amplitude about 0.3, float64 [B, S]."""
    rng = np.random.RandomState(seed)
    t = np.arange(S) / float(rate)
    return np.stack([0.3 * np.sin(2 * np.pi * (200 + 700 * (b + 1) * t) * t) + 0.01 * rng.randn(S) for b in range(B)])


def assert_within_bound(y, y64, a64, K):
    y = np.asarray(y, np.float64)
    bound = (2 * K + 2) * 2.0 ** -24 * a64
    err = np.abs(y - y64)
    worst = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    print("max error / bound = %.4f" % worst)
    assert (err <= bound).all(), worst
    assert not y[bound == 0].any()


@pytest.mark.parametrize("rate", sorted(GEOMETRY))
def test_geometry(rate):
    L, M, K, h = REF.resample_table(rate, 16000)
    assert (L, M, K) == GEOMETRY[rate]
    assert h.shape == (L, K) and h.dtype == np.float64
    assert K % 2 == 0
    for table in (h, h.astype(np.float32).astype(np.float64)):     # DC gain of every phase
        assert np.abs(table.sum(1) - 1).max() <= 3e-5


@pytest.mark.parametrize("rate", sorted(GEOMETRY))
def test_emitted_count_against_brute_force(rate):
    L, M, K, _ = REF.resample_table(rate, 16000)
    for P in (0, 1, K // 2 - 1, K // 2, K // 2 + 1, 1000):
        n = 0                                        # outputs whose last tap i + K/2 is below P
        while (n * M) // L + K // 2 <= P - 1:
            n += 1
        assert REF.resample_emitted(P, L, M, K) == n, P
    for S in (1, 2, 7, 441, 1000):
        assert REF.resample_out_len(S, L, M) == int(np.ceil(S * L / float(M)))


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_oracle_quality(rate):
    S = rate // 2
    t = np.arange(S) / float(rate)
    nyq = min(rate, 16000) / 2.0
    for f in (100.0, 1000.0, 3000.0, 0.6 * nyq, 0.8 * nyq):
        y = REF.resample_ref(np.sin(2 * np.pi * f * t), rate, 16000)
        want = np.sin(2 * np.pi * f * np.arange(y.size) / 16000.0)
        err = np.abs(y - want)[600:-600].max()
        print("passband %g Hz: %.3e" % (f, err))
        assert err <= 1.0e-3
    if rate > 16000:
        for ratio in (1.0, 1.05, 1.1, 1.5, 2.2):
            y = REF.resample_ref(np.sin(2 * np.pi * ratio * 8000.0 * t), rate, 16000)
            db = 20 * np.log10(np.abs(y)[600:-600].max())
            print("image of %.2f x Nyquist: %.1f dB" % (ratio, db))
            assert db <= -70.0


def test_oracle_lens_and_padding():
    x = pcm(2, 700, 1, 48000)
    x[1, 500:] = np.nan                              # nothing at or past lens may be read
    y = REF.resample_ref(x, 48000, 16000, lens=[700, 500])
    assert y.shape == (2, 234) and np.isfinite(y).all()
    assert not y[1, REF.resample_out_len(500, 1, 3):].any()
    assert np.array_equal(y[1, :167], REF.resample_ref(x[1, :500], 48000, 16000))


@pytest.mark.parametrize("rate", [8000, 11025, 22050, 24000, 44100, 48000])
@pytest.mark.parametrize("dtype", ["fp32", "int16"])
def test_composite_against_oracle(rate, dtype):
    L, M, K, _ = REF.resample_table(rate, 16000)
    S = 3000
    lens = [S, K // 2 + 1, 1777]
    x = pcm(3, S, 3, rate)
    x = np.round(x * 30000).astype(np.int16) if dtype == "int16" else x.astype(np.float32)
    xt = torch.from_numpy(x.copy())
    if dtype == "fp32":
        xt[2, 1777:] = float("nan")
    y, out_lens = RS.Resampler(rate, device="cpu")(xt, lens)
    y64, a64 = REF.resample_ref(x, rate, 16000, lens=lens, return_abs=True)
    assert y.dtype == torch.float32 and y.shape == y64.shape
    assert out_lens.tolist() == [REF.resample_out_len(n, L, M) for n in lens]
    assert_within_bound(y.numpy(), y64, a64, K)
    for b, n in enumerate(out_lens.tolist()):
        assert not y[b, n:].any()


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_stream_equals_whole_call_on_cpu(rate):
    L, M, K, _ = REF.resample_table(rate, 16000)
    rs = RS.Resampler(rate, device="cpu")
    S, B = 4000, 2
    x = torch.from_numpy(pcm(B, S, 5, rate).astype(np.float32))
    end = torch.tensor([250, 133], dtype=torch.int32)          # valid samples of the last chunk
    sizes = [1, 7, K // 2, 441, 1023, 2048]
    tail = S - sum(sizes)
    assert tail >= 250
    total = torch.tensor([S - tail + 250, S - tail + 133], dtype=torch.int32)
    whole, whole_lens = rs(x, total)
    st, got, at = rs.stream(B), [], 0
    for n in sizes:
        got.append(st.push(x[:, at:at + n]))
        at += n
        assert st.emitted == REF.resample_emitted(at, L, M, K) == sum(g.shape[1] for g in got)
    before = st.emitted
    got.append(st.push(x[:, at:], final=True, lens=end))
    got = torch.cat(got, 1)
    assert got.shape == whole.shape and torch.equal(got, whole)
    assert torch.equal(st.last_lens, whole_lens - before)
    with pytest.raises(ValueError):
        rs.stream(B).push(x[:, :10], lens=end)
    with pytest.raises(RuntimeError):
        st.push(x[:, :10])


def test_stream_rejects_mixed_dtypes():
    st = RS.Resampler(8000, device="cpu").stream(1)
    st.push(torch.zeros(1, 10))
    with pytest.raises(ValueError):
        st.push(torch.zeros(1, 10, dtype=torch.int16))


def test_identity_makes_no_launch():
    rs = RS.Resampler(16000, device="cpu")
    x = torch.from_numpy(np.round(pcm(2, 100, 7, 16000) * 30000).astype(np.int16))
    y, n = rs(x, [100, 60])
    assert rs.identity and not rs.use_kernel
    assert torch.equal(y, x.float()) and n.tolist() == [100, 60]


@pytest.mark.parametrize("kind", ["mfcc", "spectrogram"])
@pytest.mark.parametrize("normalize", ["utterance", "fixed"])
def test_featurizer_input_rate_is_resample_then_featurize(kind, normalize):
    rate, S = 8000, 2500
    x = pcm(2, S, 9, rate).astype(np.float32)
    lens = [S, 1800]
    got, frames = FZ.AudioFeaturizer(kind, device="cpu", normalize=normalize, input_rate=rate)(x, lens)
    y, out_lens = RS.Resampler(rate, device="cpu")(x, lens)
    want, want_frames = FZ.AudioFeaturizer(kind, device="cpu", normalize=normalize)(y, out_lens)
    assert torch.equal(got, want) and torch.equal(frames, want_frames)
    assert frames.tolist() == [FZ.num_frames(2 * n, kind) for n in lens]


def test_featurizer_int16_gain_follows_the_input_dtype():
    rate, S = 48000, 6000
    x = np.round(pcm(1, S, 11, rate) * 30000).astype(np.int16)
    got, _ = FZ.AudioFeaturizer("mfcc", device="cpu", normalize="fixed", input_rate=rate)(x)
    y, out_lens = RS.Resampler(rate, device="cpu")(x)
    want, _ = FZ.AudioFeaturizer("mfcc", device="cpu", normalize="fixed", gain=1.0 / 32768.0)(y, out_lens)
    assert torch.equal(got, want)


def test_feature_stream_with_input_rate_on_cpu():
    rate, S = 8000, 3000
    x = torch.from_numpy(pcm(2, S, 13, rate).astype(np.float32))
    fz = FZ.AudioFeaturizer("mfcc", device="cpu", normalize="fixed", input_rate=rate)
    whole, frames = fz(x)
    st = fz.stream(2)
    got = [st.push(x[:, :700]), st.push(x[:, 700:701]), st.push(x[:, 701:], final=True)]
    got = torch.cat(got, 1)
    assert got.shape == whole.shape and torch.equal(got, whole)


@pytest.mark.parametrize("input_rate", [None, 16000])
def test_default_input_rate_changes_nothing(input_rate):
    x = pcm(2, 3000, 15, 16000).astype(np.float32)
    for sr in (16000, 8000):
        old = FZ.AudioFeaturizer("mfcc", sample_rate=sr, device="cpu")
        new = FZ.AudioFeaturizer("mfcc", sample_rate=sr, device="cpu", input_rate=input_rate if sr == 16000 else None)
        assert new._rs is None
        a, fa = old(x, [3000, 2000])
        b, fb = new(x, [3000, 2000])
        assert torch.equal(a, b) and torch.equal(fa, fb)


def test_process_partition_resample_to(tmp_path, monkeypatch):
    """.npy audio carries no rate (read_audio reports 16 kHz), so the rates come from the file
    names here; off, a file is featurized at its own rate as before."""
    from deepspeech_amd.data import preprocess as P
    d = tmp_path / "audio" / "dev-clean" / "1" / "2"
    d.mkdir(parents=True)
    sizes = {8000: 2900, 48000: 17001}
    lines = []
    for rate, n in sizes.items():
        np.save(str(d / ("1-2-%05d.npy" % rate)), pcm(1, n, rate, rate)[0].astype(np.float32))
        lines.append("1-2-%05d HELLO WORLD" % rate)
    (d / "1-2.trans.txt").write_text("\n".join(lines) + "\n")
    read = P.read_audio
    monkeypatch.setattr(P, "read_audio", lambda path: (read(path)[0], int(path[-9:-4])))
    part = str(tmp_path / "audio" / "dev-clean")
    on = P.process_partition(part, str(tmp_path / "on"), resample_to=16000)
    want = sum(FZ.num_frames(REF.resample_out_len(n, 16000, rate)) for rate, n in sizes.items())
    assert on == {"utterances": 2, "frames": want}
    assert P.process_partition(part, str(tmp_path / "off"))["utterances"] == 2
