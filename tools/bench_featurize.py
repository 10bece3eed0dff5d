#!/usr/bin/env python3
"""Throughput of the GPU audio featurizer (csrc/featurize.hip) next to the numpy one.

  python tools/bench_featurize.py [--iters 50]

For 32 x 10 s and 32 x 0.5 s of int16 PCM already on the device, both feature kinds and both
normalisations: ms per call (device events around ``iters`` back-to-back calls, so launch
overhead is included but no host upload) and frames per second. Then the numpy featurizer
(data/featurizer.py) on this host for one 10 s utterance. One process, a few seconds of GPU
time. One JSON line per setting.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepspeech_amd.data.featurizer import compute_features  # noqa: E402
from deepspeech_amd.ops.featurize import AudioFeaturizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    if torch.cuda.is_available():
        dev = torch.device("cuda")
        for seconds in (10.0, 0.5):
            n = int(seconds * 16000)
            pcm = torch.from_numpy(rng.randint(-8000, 8000, size=(a.batch, n)).astype(np.int16)).to(dev)
            for kind in ("mfcc", "spectrogram"):
                for norm in ("utterance", "fixed"):
                    fz = AudioFeaturizer(kind, device=dev, normalize=norm)
                    for _ in range(3):
                        feats, frames = fz(pcm)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        feats, frames = fz(pcm)
                    e1.record()
                    torch.cuda.synchronize()
                    ms = e0.elapsed_time(e1) / a.iters
                    nf = int(frames.sum())
                    print(json.dumps({"metric": "GPU featurizer", "kind": kind, "normalize": norm, "batch": a.batch,
                                      "seconds_per_utt": seconds, "frames": nf, "ms_per_call": round(ms, 4),
                                      "frames_per_s": round(nf / (ms * 1e-3)),
                                      "x_realtime": round(a.batch * seconds / (ms * 1e-3))}), flush=True)
    else:
        print(json.dumps({"metric": "GPU featurizer", "skipped": "no GPU visible"}), flush=True)
    x = rng.randint(-8000, 8000, size=160000).astype(np.int16)
    for kind in ("mfcc", "spectrogram"):
        compute_features(x, 16000, kind)
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            f = compute_features(x, 16000, kind)
        ms = (time.perf_counter() - t0) / reps * 1e3
        print(json.dumps({"metric": "numpy featurizer (one host thread as numpy schedules it)", "kind": kind,
                          "batch": 1, "seconds_per_utt": 10.0, "frames": int(f.shape[0]),
                          "ms_per_call": round(ms, 2), "frames_per_s": round(f.shape[0] / (ms * 1e-3))}), flush=True)


if __name__ == "__main__":
    main()
