"""Audio featurizer on the GPU (csrc/featurize.hip) against the fp64 numpy oracle
(data/featurizer.py): accuracy, the exact-zero path, the statistics kernel, bf16 output,
chunk invariance, graph capture and StreamingRecognizer.accept_audio on the HIP engine.

The accuracy bound is not a constant: the same table formulation is evaluated in fp32 torch
on the CPU and its max abs error against the oracle on the same input is the yardstick; the
kernel may be at most 4x that (another summation order in the MFMA K loop, the device log,
the fp32 normalisation). Feature magnitudes reach ~430, so this is about three orders of
magnitude below the bf16 rounding the model applies to its input.
"""
import numpy as np
import pytest
import torch

from deepspeech_amd.data import featurizer as F
from deepspeech_amd.ops import featurize as FZ

pytestmark = pytest.mark.gpu

KINDS = ["mfcc", "spectrogram"]
SCHEDULE = (1, 159, 160, 161, 400, 1023)
FACTOR = 4.0


def signal(n, seed):
    """0.3 sin(2 pi (200 + 900 t) t) (t < 0.7 dur) + 0.002 N(0, 1), one stretch scaled by 0.01.
    Every sample keeps a noise floor: a frame of digital silence is an exact constant after DC
    removal, its DFT has analytically zero bins, and there any fp32 evaluation and the fp64
    oracle disagree by tens of units in the log (ill-conditioning of the oracle)."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * (200 + 900 * t) * t) * (t < 0.7 * n / 16000.0) + 0.002 * rng.randn(n)
    x[n // 3:n // 3 + n // 5] *= 0.01
    return x


def ref32(sig, kind):
    """The kernels' formulation in fp32 torch on the CPU: frames @ fp32 basis, banded mel, log,
    DCT table, lifter (tests/test_featurize.py pins its fp64 form to the oracle)."""
    fr = torch.from_numpy(FZ.frame_signal(np.asarray(sig, np.float32), kind))
    y = (fr @ torch.from_numpy(FZ.dft_basis(kind).astype(np.float32))).numpy()
    p = torch.from_numpy(FZ.power_from_dft(y, kind))
    if kind == "spectrogram":
        return torch.log(p + 1e-14).numpy()
    eps = float(np.finfo(float).eps)
    energy = p.sum(1)
    energy = torch.where(energy == 0, torch.full_like(energy, eps), energy)
    idx, w = FZ.mel_table()
    w = torch.from_numpy(w.astype(np.float32))
    feat = torch.zeros(p.shape[0], FZ.NFILT)
    for t in range(FZ.MEL_TAPS):
        on = torch.from_numpy(idx[:, 1] > t)
        cols = torch.from_numpy(idx[:, 0].astype(np.int64) + t)[on]
        feat[:, on] += p[:, cols] * w[on, t]
    feat = torch.where(feat == 0, torch.full_like(feat, eps), feat)
    cep = (torch.log(feat) @ torch.from_numpy(FZ.dct_table().astype(np.float32)))[:, :161]
    cep = cep * torch.from_numpy(FZ.lifter_table().astype(np.float32))
    cep[:, 0] = torch.log(energy)
    return cep.numpy()


def normalised(a):
    a = np.asarray(a, np.float64)
    a = a - a.mean()
    peak = np.abs(a).max()
    return a / (peak if peak > 0 else 1.0)


@pytest.mark.parametrize("int16", [False, True], ids=["fp32", "int16"])
@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_against_fp64_oracle(cuda, kind, int16):
    lens = (1, 400, 401, 5437)                   # 1, 1, 2 and 33 frames
    utts = [signal(n, seed=10 + i) for i, n in enumerate(lens)]
    utts = [np.round(u * 30000).astype(np.int16) for u in utts] if int16 else [u.astype(np.float32) for u in utts]
    want = [F.compute_features(u, 16000, kind).astype(np.float64) for u in utts]
    assert [w.shape[0] for w in want] == [FZ.num_frames(n, kind) for n in lens]
    if kind == "mfcc":
        assert [w.shape[0] for w in want] == [1, 1, 2, 33]
    fz = FZ.AudioFeaturizer(kind, device=cuda)
    feats, frames = fz(utts)
    assert feats.shape == (4, max(w.shape[0] for w in want), 161) and feats.dtype == torch.float32
    assert frames.dtype == torch.int32 and frames.tolist() == [w.shape[0] for w in want]
    feats = feats.cpu().numpy().astype(np.float64)
    assert np.isfinite(feats).all()
    err_ref = err_k = 0.0
    for b, (u, w) in enumerate(zip(utts, want)):
        err_ref = max(err_ref, np.abs(ref32(normalised(u), kind) - w).max())
        err_k = max(err_k, np.abs(feats[b, :w.shape[0]] - w).max())
        assert not feats[b, w.shape[0]:].any()   # padding rows: exact zeros
    print("featurize %s %s: kernel max abs err %.3e, fp32 formulation %.3e (ratio %.2f), max |feature| %.1f"
          % (kind, "int16" if int16 else "fp32", err_k, err_ref, err_k / err_ref, max(np.abs(w).max() for w in want)))
    assert err_ref > 0
    assert err_k <= FACTOR * err_ref, (err_k, err_ref)
    # the padded-tensor form with lens gives the same bits
    pad = np.zeros((4, 5437), utts[0].dtype)
    for b, u in enumerate(utts):
        pad[b, :u.size] = u
    feats2, frames2 = fz(torch.from_numpy(pad).to(cuda), lens=torch.tensor(lens, dtype=torch.int32, device=cuda))
    assert np.array_equal(feats2.cpu().numpy(), feats.astype(np.float32)) and torch.equal(frames2, frames)


@pytest.mark.parametrize("kind", KINDS)
def test_exact_zero_frames(cuda, kind):
    rng = np.random.RandomState(2)
    pcm = np.zeros(1900, np.int16)
    pcm[:1000] = np.clip(np.round(3000.0 * rng.randn(1000)), -32768, 32767).astype(np.int16)
    fz = FZ.AudioFeaturizer(kind, device=cuda, normalize="fixed", gain=1.0)
    feats, frames = fz(torch.from_numpy(pcm[None]))
    want = (F.mfcc if kind == "mfcc" else F.spectrogram)(pcm.astype(np.float64), 16000).astype(np.float64)
    assert frames.tolist() == [want.shape[0]]
    got = feats[0].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    bound = FACTOR * np.abs(ref32(pcm.astype(np.float64), kind) - want).max()
    L = FZ.FRAME_LEN[kind]
    zero_rows = [t for t in range(want.shape[0]) if t * 160 > 1000]      # past the pre-emphasis tail
    assert len(zero_rows) >= 3 and not pcm[zero_rows[0] * 160 - 1:].any() and zero_rows[-1] * 160 + L > 1900
    print("featurize %s zero frames: err %.3e all frames %.3e bound %.3e"
          % (kind, np.abs(got[zero_rows] - want[zero_rows]).max(), np.abs(got - want).max(), bound))
    assert np.abs(got[zero_rows] - want[zero_rows]).max() <= bound
    assert np.abs(got - want).max() <= bound
    if kind == "mfcc":
        assert np.allclose(want[zero_rows, 0], np.log(np.finfo(float).eps))   # the eps-substituted energy


def test_stats_kernel(cuda):
    from deepspeech_amd.ops import _ext
    n = 560000                                    # 35 s
    rng = np.random.RandomState(3)
    x = np.zeros((3, n), np.float32)
    x[0] = (1000.0 + 50.0 * rng.uniform(-1, 1, n)).astype(np.float32)
    x[2, 0] = -123.5
    lens = torch.tensor([n, n, 1], dtype=torch.int32, device=cuda)
    off = torch.empty(3, device=cuda)
    gain = torch.empty(3, device=cuda)
    _ext.ext().audio_stats(torch.from_numpy(x).to(cuda), lens, off, gain)
    off, gain = off.cpu().numpy().astype(np.float64), gain.cpu().numpy().astype(np.float64)
    a = x[0].astype(np.float64)
    mean = a.mean()
    want_gain = 1.0 / np.abs(a - mean).max()
    assert abs(off[0] - mean) <= 1e-6 * abs(mean), (off[0], mean)
    assert abs(gain[0] - want_gain) <= 1e-6 * want_gain, (gain[0], want_gain)
    assert off[1] == 0.0 and gain[1] == 1.0       # all-zero row
    assert off[2] == -123.5 and gain[2] == 1.0    # one sample: peak 0
    # int16 rows, no lens
    xi = np.round(x[:1, :4096] - 900.0).astype(np.int16)
    off = torch.empty(1, device=cuda)
    gain = torch.empty(1, device=cuda)
    _ext.ext().audio_stats(torch.from_numpy(xi).to(cuda), None, off, gain)
    a = xi[0].astype(np.float64)
    assert abs(float(off) - a.mean()) <= 1e-6 * abs(a.mean())
    assert abs(float(gain) - 1.0 / np.abs(a - a.mean()).max()) <= 1e-6 / np.abs(a - a.mean()).max()


@pytest.mark.parametrize("kind", KINDS)
def test_bf16_output_is_rounded_fp32(cuda, kind):
    utts = [signal(n, seed=20 + i).astype(np.float32) for i, n in enumerate((5437, 401))]
    f32, fr32 = FZ.AudioFeaturizer(kind, device=cuda)(utts)
    b16, fr16 = FZ.AudioFeaturizer(kind, device=cuda, out_dtype=torch.bfloat16)(utts)
    assert b16.dtype == torch.bfloat16 and torch.equal(fr16, fr32)
    assert torch.equal(b16, f32.to(torch.bfloat16))


@pytest.mark.parametrize("kind", KINDS)
def test_chunk_invariance_bitwise(cuda, kind):
    n, B = 4000, 3
    pcm = torch.from_numpy(np.stack([np.round(signal(n, seed=30 + b) * 30000).astype(np.int16) for b in range(B)]))
    fz = FZ.AudioFeaturizer(kind, device=cuda, normalize="fixed", gain=1.0 / 30000)
    whole, frames = fz(pcm)
    again, _ = fz(pcm)
    assert torch.equal(whole, again)
    assert frames.tolist() == [FZ.num_frames(n, kind)] * B
    st = fz.stream(B)
    got, lo = [], 0
    for c in SCHEDULE:
        got.append(st.push(pcm[:, lo:lo + c]))
        lo += c
    withheld = sum(g.shape[1] for g in got)
    assert withheld == 1 + (lo - FZ.FRAME_LEN[kind]) // 160   # complete frames only so far
    got.append(st.push(pcm[:, lo:], final=True))
    got = torch.cat(got, 1)
    assert got.shape == whole.shape
    assert torch.equal(got, whole)


@pytest.mark.parametrize("normalize", ["utterance", "fixed"])
def test_graph_capture_replays_on_new_audio(cuda, normalize):
    B, n = 2, 5437
    fz = FZ.AudioFeaturizer("mfcc", device=cuda, normalize=normalize)
    first = torch.from_numpy(np.stack([signal(n, seed=40 + b) for b in range(B)]).astype(np.float32)).to(cuda)
    other = torch.from_numpy(np.stack([signal(n, seed=50 + b) for b in range(B)]).astype(np.float32)).to(cuda)
    lens = torch.tensor([n, 3000], dtype=torch.int32, device=cuda)
    fz(first, lens)                                # warm: tables uploaded, kernels loaded
    static = first.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, frames = fz(static, lens)
    static.copy_(other)
    g.replay()
    want, want_frames = fz(other, lens)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(frames, want_frames)
    assert frames.tolist() == [FZ.num_frames(n), FZ.num_frames(3000)]
    assert not out[1, FZ.num_frames(3000):].any()


def test_preprocess_gpu_featurizer(cuda, tmp_path):
    """--featurizer gpu writes the same store as numpy up to the kernels' accuracy."""
    from deepspeech_amd.data import preprocess as P
    from deepspeech_amd.data.store import StoreIndex
    d = tmp_path / "audio" / "dev-clean" / "1" / "2"
    d.mkdir(parents=True)
    lines = []
    for i, n in enumerate((3000, 1234, 5437)):
        np.save(str(d / ("1-2-%04d.npy" % i)), signal(n, seed=70 + i).astype(np.float32))
        lines.append("1-2-%04d HELLO WORLD" % i)
    (d / "1-2.trans.txt").write_text("\n".join(lines) + "\n")
    part = str(tmp_path / "audio" / "dev-clean")
    s0 = P.process_partition(part, str(tmp_path / "np"), featurizer="numpy")
    s1 = P.process_partition(part, str(tmp_path / "gpu"), featurizer="gpu")
    assert s0 == s1 and s0["utterances"] == 3
    a, b = StoreIndex.load(str(tmp_path / "np")), StoreIndex.load(str(tmp_path / "gpu"))
    for k in ("offsets", "lengths", "labels", "label_offsets", "label_lens"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    fa = np.fromfile(str(tmp_path / "np.feats"), np.float32)
    fb = np.fromfile(str(tmp_path / "gpu.feats"), np.float32)
    assert fa.shape == fb.shape == (s0["frames"] * 161,)
    # both from float32 audio; the kernels' error against the oracle is ~1e-3 at most here
    assert np.abs(fa.astype(np.float64) - fb).max() < 1e-2


def test_accept_audio_on_hip_engine(cuda):
    from deepspeech_amd.infer import StreamingRecognizer
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.ops import rnn as RNN
    torch.manual_seed(3)
    m = DeepSpeech2(num_filters=32, num_hidden=256, num_rnn_layers=2, cell="gru", bidirectional=False).to(cuda)
    m.set_engine("hip", torch.bfloat16)
    m.eval()
    B, n, step = 2, 24000, 8000                    # 1.5 s in 0.5 s chunks
    pcm = torch.from_numpy(np.stack([np.round(signal(n, seed=60 + b) * 30000).astype(np.int16) for b in range(B)]))
    feats, frames = FZ.AudioFeaturizer("mfcc", device=cuda, normalize="fixed")(pcm)
    assert frames.tolist() == [FZ.num_frames(n)] * B
    a = StreamingRecognizer(m, batch=B)
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
