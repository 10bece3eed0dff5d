"""Audio featurizer, CPU side: frame counts, the tables the HIP kernels consume against the
fp64 numpy oracle (data/featurizer.py), the CPU path of AudioFeaturizer, stream state,
StreamingRecognizer.accept_audio on the reference engine, register budget, preprocessing CLI."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from deepspeech_amd.data import featurizer as F
from deepspeech_amd.data import preprocess as P
from deepspeech_amd.infer import StreamingRecognizer
from deepspeech_amd.models import DeepSpeech2
from deepspeech_amd.ops import featurize as FZ
from deepspeech_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["mfcc", "spectrogram"]
SCHEDULE = (1, 159, 160, 161, 400, 1023)


def chirp(n, seed=0):
    """Dithered chirp: every sample keeps a noise floor (a frame of digital silence has
    analytically zero bins, where the oracle itself is ill-conditioned)."""
    t = np.arange(n) / 16000.0
    rng = np.random.RandomState(seed)
    return 0.3 * np.sin(2 * np.pi * (200 + 900 * t) * t) + 0.002 * rng.randn(n)


def chunks(n, schedule=SCHEDULE):
    """[(lo, hi)] of the schedule's chunk sizes, then the rest."""
    out, lo = [], 0
    for c in schedule:
        out.append((lo, lo + c))
        lo += c
    assert lo < n
    out.append((lo, n))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_num_frames_matches_oracle(kind):
    L = FZ.FRAME_LEN[kind]
    for n in (1, 399, 400, 401, 560, 561, 16000):
        assert FZ.num_frames(n, kind) == F._frames(np.zeros(n), L, 160).shape[0], n
    for n in (L - 1, L, L + 1, L + 160, L + 161):
        assert FZ.num_frames(n, kind) == F._frames(np.zeros(n), L, 160).shape[0], n


@pytest.mark.parametrize("kind", KINDS)
def test_tables_reproduce_oracle_fp64(kind):
    sig = chirp(5437)
    want = (F.mfcc if kind == "mfcc" else F.spectrogram)(sig, 16000).astype(np.float64)
    got = FZ.features_from_tables(sig, kind, np.float64)
    assert got.shape == want.shape == (FZ.num_frames(5437, kind), 161)
    # the oracle's functions return float32, so 1e-9 is checked against the same steps kept in
    # fp64 (its own rfft / mel_filterbank / _dct2_ortho / _lifter) ...
    if kind == "mfcc":
        pre = np.append(sig[0], sig[1:] - 0.97 * sig[:-1])
        ps = np.abs(np.fft.rfft(F._frames(pre, 400, 160), 512)) ** 2 / 512
        fe = ps @ F.mel_filterbank(322, 512, 16000).T
        fe = np.where(fe == 0, np.finfo(float).eps, fe)
        o64 = F._lifter(F._dct2_ortho(np.log(fe))[:, :161], 22)
        o64[:, 0] = np.log(ps.sum(1))
    else:
        o64 = np.log(np.abs(np.fft.rfft(F._frames(sig, 320, 160) * np.hamming(320), 320)) ** 2 + 1e-14)
    assert np.array_equal(o64.astype(np.float32), want.astype(np.float32))
    assert np.abs(got - o64).max() <= 1e-9, np.abs(got - o64).max()
    # ... and the float32 it returns is the rounding of the table formulation's result
    assert np.abs(got - want).max() <= 0.5 * np.spacing(np.float32(np.abs(want).max())) + 1e-9


def test_mel_table_expands_exactly():
    idx, w = FZ.mel_table(16000)
    fb = F.mel_filterbank(322, 512, 16000)
    assert np.array_equal(FZ.expand_mel(idx, w), fb)
    assert int((idx[:, 1] == 0).sum()) == int((fb.sum(1) == 0).sum()) == 117
    assert idx[:, 1].max() <= FZ.MEL_TAPS and (idx[:, 0] + idx[:, 1]).max() <= 257


def test_dft_basis_packing():
    for kind in KINDS:
        L = FZ.FRAME_LEN[kind]
        nfft = 512 if kind == "mfcc" else L
        fr = np.random.RandomState(1).randn(3, L)
        w = np.hamming(L) if kind == "spectrogram" else 1.0
        spec = np.fft.rfft(fr * w, nfft)
        p = FZ.power_from_dft(fr @ FZ.dft_basis(kind), kind)
        want = np.abs(spec) ** 2 / (nfft if kind == "mfcc" else 1.0)
        assert np.allclose(p, want, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("int16", [False, True])
def test_cpu_featurizer_matches_compute_features(kind, int16):
    utts = [chirp(n, seed=i) for i, n in enumerate((5437, 401, 1900))]
    if int16:
        utts = [np.round(u * 20000).astype(np.int16) for u in utts]
    fz = FZ.AudioFeaturizer(kind, device="cpu")
    feats, frames = fz(utts)
    want = [F.compute_features(u, 16000, kind) for u in utts]
    assert frames.dtype == torch.int32 and frames.tolist() == [w.shape[0] for w in want]
    assert feats.shape == (3, max(w.shape[0] for w in want), 161) and feats.dtype == torch.float32
    for b, w in enumerate(want):
        assert np.array_equal(feats[b, :w.shape[0]].numpy(), w)
        assert not feats[b, w.shape[0]:].any()
    # the padded-tensor form of the same call
    pad = np.zeros((3, 5437), utts[0].dtype)
    for b, u in enumerate(utts):
        pad[b, :u.size] = u
    feats2, frames2 = fz(torch.from_numpy(pad), lens=[u.size for u in utts])
    assert torch.equal(feats2, feats) and torch.equal(frames2, frames)


def test_stream_needs_fixed_normalisation():
    with pytest.raises(ValueError):
        FZ.AudioFeaturizer("mfcc", device="cpu").stream(1)


@pytest.mark.parametrize("kind", KINDS)
def test_cpu_stream_equals_whole_call(kind):
    n, B = 4000, 2
    pcm = np.stack([chirp(n, seed=3), chirp(n, seed=4)])
    fz = FZ.AudioFeaturizer(kind, device="cpu", normalize="fixed", gain=0.5)
    whole, frames = fz(pcm)
    assert frames.tolist() == [FZ.num_frames(n, kind)] * B
    st = fz.stream(B)
    got, seen = [], 0
    parts = chunks(n)
    for i, (lo, hi) in enumerate(parts):
        final = i == len(parts) - 1
        out = st.push(pcm[:, lo:hi], final=final)
        seen = hi
        got.append(out)
        if not final:
            # only complete frames so far: the partial last frame is withheld
            L = FZ.FRAME_LEN[kind]
            done = sum(g.shape[1] for g in got)
            assert done == (0 if seen < L else 1 + (seen - L) // 160)
    got = torch.cat(got, 1)
    assert got.shape == whole.shape
    assert torch.equal(got, whole)
    with pytest.raises(RuntimeError):
        st.push(pcm[:, :10])


def test_cpu_stream_final_lens():
    """Streams that end at different samples of the last chunk."""
    n = 2000
    pcm = np.stack([chirp(n, seed=5), chirp(n, seed=6)])
    ends = [2000, 1530]
    fz = FZ.AudioFeaturizer("mfcc", device="cpu", normalize="fixed")
    st = fz.stream(2)
    a = st.push(pcm[:, :1000])
    b = st.push(pcm[:, 1000:], final=True, lens=[e - 1000 for e in ends])
    got = torch.cat([a, b], 1)
    for r, e in enumerate(ends):
        want = torch.from_numpy(F.mfcc(pcm[r, :e], 16000))
        tot = a.shape[1] + int(st.last_frames[r])
        assert tot == want.shape[0]
        assert torch.equal(got[r, :tot], want)
        assert not got[r, tot:].any()


def _model(cell="gru", H=48, L=2):
    torch.manual_seed(5)
    m = DeepSpeech2(num_filters=4, num_hidden=H, num_rnn_layers=L, cell=cell, bidirectional=False)
    # non-trivial running statistics so inference-mode BN matters
    for blk in (m.conv1, m.conv2):
        blk.running_mean.uniform_(-0.1, 0.1)
        blk.running_var.uniform_(0.5, 1.5)
    return m.eval()


def test_accept_audio_matches_accept_on_features():
    m = _model()
    B, n = 2, 40000                                           # 2.5 s
    pcm = np.stack([np.round(chirp(n, seed=7 + b) * 20000).astype(np.int16) for b in range(B)])
    step = int(0.37 * 16000)
    feats, frames = FZ.AudioFeaturizer("mfcc", device="cpu", normalize="fixed")(pcm)
    assert frames.tolist() == [FZ.num_frames(n)] * B
    a = StreamingRecognizer(m, batch=B)
    b = StreamingRecognizer(m, batch=B)
    done = 0
    for s in range(0, n, step):
        a.accept_audio(pcm[:, s:s + step], final=s + step >= n)
        new = a.total - done                                  # the frames that chunk completed
        if new:
            b.accept(feats[:, done:done + new])
        done += new
    assert done == feats.shape[1]
    got, want = torch.cat(a.logprobs, 0), torch.cat(b.logprobs, 0)
    assert got.shape == want.shape and got.shape[0] > 0
    assert torch.allclose(got, want, atol=2e-4), (got - want).abs().max()
    assert a.finish() == b.finish()
    # and the whole signal at once
    with torch.no_grad():
        logits, lens = m(feats, torch.full((B,), feats.shape[1], dtype=torch.int32))
    full = torch.log_softmax(logits.float(), -1)
    assert torch.allclose(got, full, atol=2e-4)
    assert a.finish() == R.greedy_decode(full, lens)
    # reset() starts a new audio stream
    a.reset()
    a.accept_audio(pcm[:, :step])
    assert a.total == 1 + (step - 400) // 160


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
def test_featurize_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    rows = KR.analyse(os.path.join(ROOT, "deepspeech_amd", "csrc", "featurize.hip"))
    assert len(rows) >= 10, [r["name"] for r in rows]        # 2 stats + 2 kinds x 2 inputs x 2 outputs
    bad = [r["name"] for r in rows if r.get("VGPRs Spill", 0) or r.get("ScratchSize [bytes/lane]", 0)]
    assert not bad, bad


def _fake_partition(tmp_path):
    d = tmp_path / "audio" / "dev-clean" / "1" / "2"
    d.mkdir(parents=True)
    lines = []
    for i, n in enumerate((3000, 1234, 5437)):
        np.save(str(d / ("1-2-%04d.npy" % i)), chirp(n, seed=i))
        lines.append("1-2-%04d HELLO WORLD %d" % (i, i))
    (d / "1-2.trans.txt").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "audio" / "dev-clean")


def test_preprocess_featurizer_option(tmp_path):
    part = _fake_partition(tmp_path)
    s0 = P.process_partition(part, str(tmp_path / "a"))
    s1 = P.process_partition(part, str(tmp_path / "b"), featurizer="numpy")
    assert s0 == s1 and s0["utterances"] == 3
    for ext in (".feats", ".index.npz"):
        assert (tmp_path / ("a" + ext)).read_bytes() == (tmp_path / ("b" + ext)).read_bytes()
    with pytest.raises(ValueError):
        P.process_partition(part, str(tmp_path / "c"), featurizer="fft")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            P.process_partition(part, str(tmp_path / "c"), featurizer="gpu")
        with pytest.raises(RuntimeError, match="GPU"):
            P.main(["--audio_path", str(tmp_path / "audio"), "--out_dir", str(tmp_path / "o"),
                    "--featurizer", "gpu"])
