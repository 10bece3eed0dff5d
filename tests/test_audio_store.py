"""Audio stores (data/store.py), the per-batch front end (data/audio_batch.py) and the drivers
that read them, on the CPU: the writer and the native loader hand back the padded samples, the
front end equals the numpy featurizer per utterance, feature stores run the code they ran before,
and a tiny training run with noise augmentation is finite, repeatable and evaluable."""
import json
import os

import numpy as np
import pytest
import torch

from deepspeech_amd.data import featurizer as F
from deepspeech_amd.data.audio_batch import AudioFrontEnd, is_audio_batch
from deepspeech_amd.data.store import AUDIO_HOP, StoreBatches, StoreIndex, StoreWriter
from deepspeech_amd.data.synthetic import DummyBucketWalk, FixedShapeBatches, to_device


def _utterances(n=8, seed=0):
    """n pseudo-utterances of about 1 s, ragged, none a whole number of hops."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = 14000 + 531 * i + 7
        t = np.arange(s) / 16000.0
        sig = 0.3 * np.sin(2 * np.pi * (200 + 40 * i) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(s)
        out.append((sig.astype(np.float32), rng.integers(0, 27, size=4 + i % 3).astype(np.int32)))
    return out


def _write_audio_store(prefix, utts):
    w = StoreWriter(prefix, AUDIO_HOP, kind="audio")
    for sig, lab in utts:
        w.add_audio(sig, lab, "")
    return w.close()


def _padded(sig):
    rows = -(-len(sig) // AUDIO_HOP)
    p = np.zeros(rows * AUDIO_HOP, np.float32)
    p[:len(sig)] = sig
    return p


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = tmp_path_factory.mktemp("audio_store")
    utts = _utterances()
    return str(d), _write_audio_store(os.path.join(str(d), "train-tiny"), utts), utts


def test_index_of_an_audio_store(store):
    _, prefix, utts = store
    ix = StoreIndex.load(prefix)
    assert ix.is_audio and ix.kind == "audio" and ix.freq == 160 and ix.rate == 16000
    assert ix.lengths.tolist() == [-(-len(s) // 160) for s, _ in utts]
    assert os.path.getsize(prefix + ".feats") == 4 * 160 * int(ix.lengths.sum())
    with pytest.raises(ValueError):
        StoreWriter(prefix + "x", 161, kind="audio")


def test_writer_to_batches_returns_the_padded_samples(store):
    _, prefix, utts = store
    src = StoreBatches(prefix, 4, shuffle=False, sortagrad_epochs=1, num_threads=1)
    try:
        assert src._min.tolist() == (src.index.min_frames() + 1).tolist()      # rows - 1 frames
        seen = 0
        for _ in range(src.steps_per_epoch()):
            hb = src.next()
            assert hb.feats.dtype == np.float32 and hb.feats.shape[2] == 160
            for i in range(len(hb.seq_lens)):
                r = int(hb.seq_lens[i])
                match = [u for u in utts if -(-len(u[0]) // 160) == r and
                         u[1].tolist() == hb.labels[i, :hb.label_lens[i]].tolist()]
                assert len(match) == 1
                assert np.array_equal(hb.feats[i, :r].reshape(-1), _padded(match[0][0]))
                assert not hb.feats[i, r:].any()
                seen += 1
        assert seen == len(utts)
    finally:
        src.close()


@pytest.mark.parametrize("kind", ["mfcc", "spectrogram"])
def test_front_end_on_the_cpu_equals_compute_features(store, kind):
    _, prefix, utts = store
    src = StoreBatches(prefix, 4, shuffle=False, num_threads=1)
    try:
        hb = src.next()
    finally:
        src.close()
    b = to_device(hb, torch.device("cpu"))
    assert is_audio_batch(b["feats"])
    out = AudioFrontEnd(kind, "cpu")(b)
    assert out["feats"].shape[2] == 161 and out["feats"].dtype == torch.float32
    assert out["seq_lens"].dtype == torch.int32
    assert out["seq_lens"].tolist() == [int(r) - 1 for r in hb.seq_lens]
    assert out["labels"] is b["labels"] and out["flat_labels"] is b["flat_labels"]
    for i, r in enumerate(hb.seq_lens):
        sig = hb.feats[i, :r].reshape(-1)
        want = F.compute_features(sig, 16000, kind).astype(np.float32)
        assert want.shape[0] == r - 1
        assert np.array_equal(out["feats"][i, :r - 1].numpy(), want)
        assert not out["feats"][i, r - 1:].any()


def test_front_end_augments_in_training_only(store):
    from deepspeech_amd.ops import waveaug as WA
    _, prefix, _ = store
    src = StoreBatches(prefix, 4, shuffle=False, num_threads=1)
    try:
        b = to_device(src.next(), torch.device("cpu"))
    finally:
        src.close()
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=10:10"), WA.NoiseBank.synthetic(0), seed=1)
    plain, front = AudioFrontEnd("mfcc", "cpu"), AudioFrontEnd("mfcc", "cpu", wave_aug=aug)
    base = plain(b)["feats"]
    assert torch.equal(front(b, step=3, training=False)["feats"], base) and aug.plan is None
    noisy = front(b, step=3, first_utt=8, training=True)
    assert not torch.equal(noisy["feats"], base) and torch.equal(noisy["seq_lens"], plain(b)["seq_lens"])
    assert aug.plan.shape == (4, 4) and bool((aug.plan[:, 0] == 1).all())
    assert torch.equal(front(b, step=3, first_utt=8, training=True)["feats"], noisy["feats"])
    with pytest.raises(ValueError):
        plain(dict(b, feats=torch.zeros(2, 10, 161)))


def test_a_feature_store_is_untouched(tmp_path):
    prefix = str(tmp_path / "train-feats")
    w = StoreWriter(prefix)
    rng = np.random.default_rng(0)
    for i in range(4):
        w.add(rng.standard_normal((60 + i, 161)).astype(np.float32), [1, 2, 3], "abc")
    w.close()
    z = np.load(prefix + ".index.npz")
    assert "kind" not in z.files and "rate" not in z.files                       # the index it always wrote
    ix = StoreIndex.load(prefix)
    assert not ix.is_audio and ix.freq == 161
    src = StoreBatches(prefix, 2, shuffle=False, num_threads=1)
    try:
        assert src._min.tolist() == ix.min_frames().tolist()
        assert src.next().feats.shape[2] == 161
    finally:
        src.close()
    from deepspeech_amd import test as TE
    from deepspeech_amd import train as TR
    from deepspeech_amd import config as C

    class _Src:
        index = ix
    args = C.build_train_parser().parse_args([])
    assert TR.build_front_end(args, _Src(), torch.device("cpu"), False) is None
    assert TE.eval_front_end(args, _Src(), torch.device("cpu")) is None
    args = C.build_train_parser().parse_args(["--wave_aug", "noise=synthetic,p=1"])
    with pytest.raises(ValueError, match="preprocess --store audio"):
        TR.build_front_end(args, _Src(), torch.device("cpu"), False)


def test_dummy_audio_sources_follow_the_frame_feed():
    a, f = DummyBucketWalk(3, seed=5, audio=True), DummyBucketWalk(3, seed=5)
    for _ in range(3):
        x, y = a.next(), f.next()
        assert x.feats.shape == (y.feats.shape[0], y.feats.shape[1] + 1, 160)
        assert (x.seq_lens == y.seq_lens + 1).all() and (x.label_lens == y.label_lens).all()
        assert x.labels.shape == y.labels.shape
    a, f = FixedShapeBatches(4, 120, seed=2, pool=1, audio=True).next(), FixedShapeBatches(4, 120, seed=2, pool=1).next()
    assert a.feats.shape == (4, 121, 160) and f.feats.shape == (4, 120, 161)
    assert a.seq_lens.max() == 121 and a.seq_lens.min() > 21 and a.seq_lens.dtype == np.int32
    for b in range(4):
        assert not a.feats[b, a.seq_lens[b]:].any() and a.feats[b, a.seq_lens[b] - 1].any()
    a.validate()


def test_preprocess_writes_an_audio_store(tmp_path):
    from scipy.io import wavfile
    from deepspeech_amd.data import preprocess as P
    d = tmp_path / "audio" / "train-x" / "1" / "2"
    d.mkdir(parents=True)
    rng = np.random.default_rng(3)
    sigs = {"1-2-0001": (rng.standard_normal(5000) * 3000).astype(np.int16),
            "1-2-0002": (rng.standard_normal(3301) * 3000).astype(np.int16)}
    for k, v in sigs.items():
        wavfile.write(str(d / (k + ".wav")), 16000, v)
    (d / "1-2.trans.txt").write_text("1-2-0001 HELLO WORLD\n1-2-0002 GOOD DAY\n")
    P.main(["--audio_path", str(tmp_path / "audio"), "--out_dir", str(tmp_path / "out"), "--store", "audio"])
    ix = StoreIndex.load(str(tmp_path / "out" / "train-x"))
    assert ix.is_audio and ix.lengths.tolist() == [21, 32]                       # sorted by length
    mm = np.memmap(str(tmp_path / "out" / "train-x.feats"), dtype=np.float32, mode="r")
    assert np.array_equal(mm[:3301], sigs["1-2-0002"].astype(np.float32)) and not mm[3301:21 * 160].any()
    wavfile.write(str(d / "1-2-0001.wav"), 8000, sigs["1-2-0001"])
    with pytest.raises(ValueError, match="resample_to"):
        P.main(["--audio_path", str(tmp_path / "audio"), "--out_dir", str(tmp_path / "o2"), "--store", "audio"])
    P.main(["--audio_path", str(tmp_path / "audio"), "--out_dir", str(tmp_path / "o3"), "--store", "audio",
            "--resample_to", "16000"])
    assert sorted(StoreIndex.load(str(tmp_path / "o3" / "train-x")).lengths.tolist()) == [21, 63]


# ------------------------------------------------------------------------------- train driver
def _train(train_dir, data_dir, extra):
    from deepspeech_amd import train as T
    rc = T.main(["--train_dir", train_dir, "--data_dir", data_dir, "--max_steps", "3", "--batch_size", "4",
                 "--num_hidden", "16", "--num_rnn_layers", "2", "--num_filters", "4", "--cell", "gru", "--device", "cpu",
                 "--engine", "ref", "--checkpoint_every", "0", "--summary_every", "1", "--activation_summaries", "False",
                 "--initial_lr", "1e-3"] + extra)
    assert rc == 0
    recs = [json.loads(l) for l in open(os.path.join(train_dir, "metrics.jsonl"))]
    losses = [r["loss"] for r in recs if "loss" in r]
    assert [r["step"] for r in recs if "loss" in r] == [0, 1, 2]
    return losses


def test_train_and_evaluate_from_an_audio_store_on_the_cpu(store, tmp_path):
    data_dir, _, _ = store
    aug = ["--wave_aug", "noise=synthetic,p=1,snr=10:10"]
    a = _train(str(tmp_path / "a"), data_dir, aug)
    b = _train(str(tmp_path / "b"), data_dir, aug)
    plain = _train(str(tmp_path / "c"), data_dir, [])
    print("augmented", a, "plain", plain)
    assert all(np.isfinite(v) for v in a + plain)
    assert a == b
    assert all(x != y for x, y in zip(a, plain))
    params = json.load(open(os.path.join(str(tmp_path / "a"), "deepSpeech_parameters.json")))
    assert params["audio_features"] == "mfcc" and params["wave_aug"] == aug[1]
    from deepspeech_amd import test as TE
    rc = TE.main(["--checkpoint_dir", str(tmp_path / "a"), "--eval_dir", str(tmp_path / "eval"), "--data_dir", data_dir,
                  "--eval_data", "train", "--run_once", "True", "--batch_size", "4", "--num_examples", "8",
                  "--device", "cpu", "--engine", "ref", "--display", "False"])
    assert rc == 0
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path / "eval"), "eval.jsonl"))]
    assert len(rows) == 1 and np.isfinite(rows[0]["char_err_rate"])
