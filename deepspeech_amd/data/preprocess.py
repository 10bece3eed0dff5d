"""Offline LibriSpeech preprocessing (reference: src/preprocess_LibriSpeech.py).

  python -m deepspeech_amd.data.preprocess --audio_path ../data/LibriSpeech/audio \
         --out_dir ../data/LibriSpeech/processed [--features mfcc|spectrogram] [--tfrecords]
         [--featurizer numpy|gpu] [--resample_to RATE] [--store features|audio]

``--store audio`` writes the samples themselves (an audio store, data/store.py: rows of one
160-sample hop at 16 kHz) instead of feature frames; training then featurizes per step on the
GPU, which is what waveform augmentation (train --wave_aug) needs.

``--featurizer numpy`` (default) runs data/featurizer.py one file at a time; ``gpu`` batches
about 64 utterances per call through the HIP featurizer (ops/featurize.py) and feeds the same
sort / store / TFRecord code. ``--resample_to RATE`` (0: off) converts every file whose rate is
not RATE to it before featurizing: with ``numpy`` through the fp64 oracle
(ops/reference.py resample_ref), with ``gpu`` on the device (ops/resample.py); off, a file is
featurized at its own rate.

For every partition directory under ``audio_path`` (train-clean-100, dev-clean, ...):
read ``*.trans.txt`` transcripts, decode audio, compute features, map characters with the
28-symbol alphabet, sort utterances by frame count (SortaGrad) and write
  * a store (``<out>/<partition>.feats`` + ``.index.npz``) for the native mmap loader, and
  * optionally reference-compatible TFRecords: train split into ``train_<len//100>``
    bins with sparse bins (< 20 utts) dropped, dev/test as one sorted file
    (src/preprocess_LibriSpeech.py:143-176).
Audio decoding: ``.wav`` via scipy, ``.npy`` arrays; ``.flac`` needs the optional
``soundfile`` module (not installed in this image) and is reported clearly if missing.
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Tuple

import numpy as np

from .. import ALPHABET
from .featurizer import compute_features
from .store import StoreWriter

CHAR_TO_IX = {ch: i for i, ch in enumerate(ALPHABET)}


def encode_transcript(text: str) -> List[int]:
    return [CHAR_TO_IX[c] for c in text.upper() if c in CHAR_TO_IX]


def read_audio(path: str) -> Tuple[np.ndarray, int]:
    ext = os.path.splitext(path)[1].lower()
    if ext == ".wav":
        from scipy.io import wavfile
        sr, data = wavfile.read(path)
        data = data.astype(np.float64)
        if data.ndim > 1:
            data = data.mean(1)
        return data, int(sr)
    if ext == ".npy":
        return np.load(path, allow_pickle=False).astype(np.float64), 16000
    if ext == ".flac":
        try:
            import soundfile as sf  # type: ignore
        except ImportError:
            raise RuntimeError("decoding .flac needs the 'soundfile' package; convert to .wav first")
        data, sr = sf.read(path)
        return np.asarray(data, np.float64), int(sr)
    raise ValueError("unsupported audio file %s" % path)


def scan_partition(part_dir: str) -> List[Tuple[str, str]]:
    """[(audio_path, transcript)] from LibriSpeech ``<spk>/<chapter>/*.trans.txt`` files."""
    items = []
    for tf in sorted(glob.glob(os.path.join(part_dir, "**", "*.txt"), recursive=True)):
        d = os.path.dirname(tf)
        with open(tf) as f:
            for line in f:
                parts = line.strip().split(" ", 1)
                if len(parts) != 2:
                    continue
                uid, text = parts
                for ext in (".flac", ".wav", ".npy"):
                    p = os.path.join(d, uid + ext)
                    if os.path.exists(p):
                        items.append((p, text))
                        break
    return items


GPU_GROUP = 64        # utterances per AudioFeaturizer call of --featurizer gpu


def _gpu_features(items: List[Tuple[str, str]], features: str, resample_to: int = 0) -> list:
    """[(feats, labels, text)] in the order of ``items``, featurized on the GPU in groups of
    GPU_GROUP files sorted by length (bounds the padding of a group's [B, S_max] upload)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("--featurizer gpu needs a GPU (none is visible); use --featurizer numpy")
    from ..ops.featurize import AudioFeaturizer
    fz: Dict[int, AudioFeaturizer] = {}
    utts = []
    for g0 in range(0, len(items), GPU_GROUP):
        group = []
        for path, text in items[g0:g0 + GPU_GROUP]:
            audio, sr = read_audio(path)
            group.append((audio, sr, text))
        order = sorted(range(len(group)), key=lambda i: (group[i][1], len(group[i][0])))
        done = {}
        for sr in sorted({g[1] for g in group}):
            idx = [i for i in order if group[i][1] == sr]
            if sr not in fz:
                if resample_to:
                    fz[sr] = AudioFeaturizer(features, sample_rate=resample_to, device="cuda",
                                             normalize="utterance", input_rate=sr)
                else:
                    fz[sr] = AudioFeaturizer(features, sample_rate=sr, device="cuda", normalize="utterance")
            # float32 PCM on the device: exact for 16-bit audio
            feats, frames = fz[sr]([group[i][0].astype(np.float32) for i in idx])
            feats, frames = feats.cpu().numpy(), frames.cpu().tolist()
            for k, i in enumerate(idx):
                done[i] = np.ascontiguousarray(feats[k, :frames[k]])
        for i, (_, _, text) in enumerate(group):
            utts.append((done[i], encode_transcript(text), text))
    return utts


def _audio_partition(part_dir: str, out_prefix: str, featurizer: str, resample_to: int) -> Dict[str, int]:
    """An audio store (data/store.py): the 16 kHz samples themselves in rows of one hop, sorted by
    length; the training and evaluation drivers featurize them per batch."""
    from .store import AUDIO_RATE
    utts = []
    for path, text in scan_partition(part_dir):
        audio, sr = read_audio(path)
        if resample_to and sr != resample_to:
            if featurizer == "gpu":
                from ..ops.resample import Resampler
                y, n = Resampler(sr, resample_to)(audio.astype(np.float32)[None, :])
                audio = y[0, : int(n[0])].cpu().numpy()
            else:
                from ..ops.reference import resample_ref
                audio = resample_ref(audio, sr, resample_to)
            sr = resample_to
        if sr != AUDIO_RATE:
            raise ValueError("%s is at %d Hz and an audio store holds %d Hz: pass --resample_to %d"
                             % (path, sr, AUDIO_RATE, AUDIO_RATE))
        utts.append((np.asarray(audio, np.float32), encode_transcript(text), text))
    utts.sort(key=lambda u: u[0].shape[0])                 # SortaGrad order
    w = StoreWriter(out_prefix, 160, kind="audio")
    for audio, lab, text in utts:
        w.add_audio(audio, lab, text)
    w.close()
    return {"utterances": len(utts), "rows": int(sum(w.lengths))}


def process_partition(part_dir: str, out_prefix: str, features: str = "mfcc",
                      tfrecord_dir: str = "", is_train: bool = False, min_bin: int = 20,
                      featurizer: str = "numpy", resample_to: int = 0, store: str = "features") -> Dict[str, int]:
    if featurizer not in ("numpy", "gpu"):
        raise ValueError("featurizer must be 'numpy' or 'gpu', not %r" % (featurizer,))
    if store not in ("features", "audio"):
        raise ValueError("store must be 'features' or 'audio', not %r" % (store,))
    resample_to = int(resample_to)
    if store == "audio":
        if tfrecord_dir:
            raise ValueError("--tfrecords holds feature frames; an audio store has no TFRecord form")
        return _audio_partition(part_dir, out_prefix, featurizer, resample_to)
    utts = []
    if featurizer == "gpu":
        utts = _gpu_features(scan_partition(part_dir), features, resample_to)
    else:
        for path, text in scan_partition(part_dir):
            audio, sr = read_audio(path)
            if resample_to and sr != resample_to:
                from ..ops.reference import resample_ref
                audio, sr = resample_ref(audio, sr, resample_to), resample_to
            feats = compute_features(audio, sr, features)
            utts.append((feats, encode_transcript(text), text))
    utts.sort(key=lambda u: u[0].shape[0])                 # SortaGrad order
    w = StoreWriter(out_prefix, utts[0][0].shape[1] if utts else 161)
    for feats, lab, text in utts:
        w.add(feats, lab, text)
    w.close()
    if tfrecord_dir:
        from ..runtime import native
        N = native.load()
        name = os.path.basename(out_prefix)
        os.makedirs(os.path.join(tfrecord_dir, name), exist_ok=True)
        if is_train:
            bins: Dict[int, list] = {}
            for feats, lab, _ in utts:
                bins.setdefault(feats.shape[0] // 100, []).append(
                    N.make_sequence_example(feats.shape[0], feats, np.asarray(lab, np.int64), "feats"))
            for k, recs in bins.items():
                if len(recs) >= min_bin:
                    N.write_records(os.path.join(tfrecord_dir, name, "train_%d.tfrecords" % k), recs)
        else:
            recs = [N.make_sequence_example(f.shape[0], f, np.asarray(l, np.int64), "feats") for f, l, _ in utts]
            N.write_records(os.path.join(tfrecord_dir, name, name + ".tfrecords"), recs)
    return {"utterances": len(utts), "frames": int(sum(u[0].shape[0] for u in utts))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--audio_path", default="../data/LibriSpeech/audio")
    ap.add_argument("--out_dir", default="../data/LibriSpeech/processed")
    ap.add_argument("--features", default="mfcc", choices=["mfcc", "spectrogram"])
    ap.add_argument("--tfrecords", action="store_true")
    ap.add_argument("--featurizer", default="numpy", choices=["numpy", "gpu"],
                    help="numpy: data/featurizer.py, one file at a time; gpu: batched HIP kernels (ops/featurize.py)")
    ap.add_argument("--resample_to", type=int, default=0, metavar="RATE",
                    help="resample every file to RATE Hz before featurizing (0: featurize at the file's rate)")
    ap.add_argument("--store", default="features", choices=["features", "audio"],
                    help="features: feature frames [frames, 161]; audio: the 16 kHz samples in rows of 160 "
                         "(--features is then chosen at training time: train --audio_features)")
    a = ap.parse_args(argv)
    for part in sorted(glob.glob(os.path.join(a.audio_path, "*"))):
        if not os.path.isdir(part):
            continue
        name = os.path.basename(part)
        stats = process_partition(part, os.path.join(a.out_dir, name), a.features,
                                  a.out_dir if a.tfrecords else "", is_train=name.startswith("train"),
                                  featurizer=a.featurizer, resample_to=a.resample_to, store=a.store)
        print(name, stats)


if __name__ == "__main__":
    main()
