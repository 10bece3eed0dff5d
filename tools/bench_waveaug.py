#!/usr/bin/env python3
"""Time of the noise-augmentation kernels (csrc/waveaug.hip) and of the whole audio front end at
the headline batch, next to a plain device copy of the waveform tensor (the bandwidth yardstick).

  python tools/bench_waveaug.py [--batch 32] [--samples 160000] [--iters 2000]

fp32 [batch, samples] with ragged lengths, the synthetic noise bank, p = 1 (every row mixed: the
upper bound of the work), in one process after warm-up, two rounds alternating the ops (the
spread): plan, energy partials, coefficient, apply, the WaveAugment call (all four), the
featurizer alone and the front end (augmentation + featurizer). Each op is timed twice: device
events around back-to-back eager calls (host launch overhead and output allocation included) and
around replays of a HIP graph of 20 calls (the GPU's time for a call). GB/s = the bytes the
algorithm needs from HBM (the bank is expected to stay in cache) over the graph time. One JSON
line per op and round.

  python tools/bench_waveaug.py --train 120

times the training step of `python -m deepspeech_amd.train --dummy True` at the headline model
(5-layer BiGRU-800, batch 32 x 1000 frames) from dummy features, from dummy audio and from dummy
audio with --wave_aug, alternating, two rounds: the median of the windows' step_ms_p50 (device
events between steps, so the front end of a step is inside) from metrics.jsonl, the first 40
steps left out.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_specaug import _events, _graph  # noqa: E402
from deepspeech_amd.ops import waveaug as WA  # noqa: E402


def train_steps(a):
    base = [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--dummy_frames", "1000",
            "--batch_size", str(a.batch), "--num_hidden", "800", "--num_rnn_layers", "5", "--cell", "gru", "--engine",
            "hip", "--max_steps", str(a.train), "--checkpoint_every", "0", "--log_every", "10"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    settings = (("dummy features", []), ("dummy audio", ["--dummy_audio", "True"]),
                ("dummy audio, --wave_aug p=0.4", ["--dummy_audio", "True", "--wave_aug", "noise=synthetic,p=0.4,snr=10:30"]))
    for rnd in range(2):
        for name, extra in settings:
            with tempfile.TemporaryDirectory() as d:
                r = subprocess.run(base + ["--train_dir", d] + extra, env=env, cwd=ROOT, capture_output=True, text=True)
                if r.returncode != 0:
                    raise SystemExit("training run failed:\n" + (r.stdout + r.stderr)[-3000:])
                recs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
            p50 = sorted(x["step_ms_p50"] for x in recs if "step_ms_p50" in x and x["step"] >= 40)
            print(json.dumps({"metric": "training step, 5x BiGRU-800, batch %d x 1000 frames" % a.batch, "setting": name,
                              "round": rnd, "steps": a.train, "windows": len(p50),
                              "step_ms_p50_median": p50[len(p50) // 2], "step_ms_p50_min": p50[0],
                              "step_ms_p50_max": p50[-1], "last_loss": [x["loss"] for x in recs if "loss" in x][-1]}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--train", type=int, default=0, metavar="STEPS", help="time whole training steps instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_waveaug: no GPU visible; there is nothing to time without one")
    if a.train > 0:
        return train_steps(a)
    from deepspeech_amd.data.audio_batch import AudioFrontEnd
    from deepspeech_amd.ops import _ext
    from deepspeech_amd.ops.featurize import AudioFeaturizer
    dev = torch.device("cuda")
    B, S = a.batch, a.samples
    g = torch.Generator().manual_seed(0)
    x_host = torch.randn(B, S, generator=g) * 0.1
    lens_host = (torch.randint(S - S // 10, S + 1, (B,), generator=g) // 160 * 160).to(torch.int32)
    lens_host[0] = S
    x, lens = x_host.to(dev), lens_host.to(dev)
    assert WA.kernels_cover(x)
    bank = WA.NoiseBank.synthetic(0)
    aug = WA.WaveAugment(WA.WaveAugPolicy.parse("p=1,snr=10:30"), bank, 1234)
    C = _ext.ext().waveaug
    data, start, length = bank.on(dev)
    aug(x, lens, 7)
    plan, energy, coef = aug.plan, aug.energy, aug.coef
    nseg = (S + C.segment() - 1) // C.segment()
    part = torch.empty(B, nseg, 2, device=dev)
    out = torch.empty_like(x)
    fz = AudioFeaturizer("mfcc", device=dev, normalize="utterance")
    front = AudioFrontEnd("mfcc", dev, wave_aug=aug)
    batch = {"feats": x.view(B, S // 160, 160), "seq_lens": (lens // 160).to(torch.int32)}
    tensor, valid = B * S * 4, int(lens_host.sum()) * 4
    shape = {"B": B, "S": S, "iters": a.iters, "bank_bytes": int(bank.data.numel()) * 4}
    ops = (
        ("device copy of the tensor (yardstick)", lambda: out.copy_(x), 2 * tensor),
        ("waveaug plan", lambda: WA.waveaug_plan(lens, B, S, bank, aug.policy, 1234, 7, device=dev), B * 20),
        ("waveaug energy partials", lambda: C.energy(x, lens, plan, data, start, length, part), valid + B * nseg * 8),
        ("waveaug coefficient", lambda: C.coef(lens, plan, part, energy, coef, S), B * nseg * 8 + B * 40),
        # x read below lens, y written whole (the tail zeros come from the same launch)
        ("waveaug apply", lambda: C.apply(x, lens, plan, coef, data, start, length, out), valid + tensor),
        ("WaveAugment call (plan + energy + coefficient + apply)", lambda: aug(x, lens, 7), 2 * valid + tensor),
        ("AudioFeaturizer mfcc, utterance statistics", lambda: fz(x, lens), 2 * valid + B * (S // 160) * 161 * 4),
        ("front end (WaveAugment + AudioFeaturizer)", lambda: front(batch, 7, training=True),
         4 * valid + tensor + B * (S // 160) * 161 * 4),
    )
    for rnd in range(2):
        for name, fn, nbytes in ops:
            eager = _events(fn, max(20, a.iters // 10))
            graph = _graph(fn, a.iters)
            print(json.dumps({"metric": name, **shape, "round": rnd, "us_per_call_eager": round(eager * 1e3, 2),
                              "us_per_call_graph": round(graph * 1e3, 2), "hbm_bytes": nbytes,
                              "GBps_graph": round(nbytes / (graph * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
