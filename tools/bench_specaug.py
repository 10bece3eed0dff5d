#!/usr/bin/env python3
"""Time of the SpecAugment kernels (csrc/specaug.hip) at the headline batch next to a plain device
copy of the same tensor (the bandwidth yardstick: it moves the same bytes, the kernel never more,
since masked rows are not read) and the numpy/torch reference on the host.

  python tools/bench_specaug.py [--batch 32] [--frames 1000] [--bins 161] [--iters 4000]

For the presets ld and ls, ragged lengths, in one process after warm-up, two rounds alternating
the ops (the spread): plan, mean, apply out of place, apply in place (the preset without its warp)
and the whole call (plan + mean + apply). Each op is timed twice: device events around
back-to-back eager calls (host launch overhead and the output allocation included) and around
replays of a HIP graph of 20 calls (the GPU's time for a call). GB/s = the bytes the algorithm
needs over the graph time. One JSON line per op, preset and round.

  python tools/bench_specaug.py --train 120

times the training step of `python -m deepspeech_amd.train --dummy True` at the headline model
(5-layer BiGRU-800, batch 32 x 1000 frames) with --specaug ls and without the flag, alternating,
two processes each: the median of the windows' step_ms_p50 (device events between steps) that
the driver writes to metrics.jsonl, the first 40 steps left out.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deepspeech_amd.ops import reference as R  # noqa: E402
from deepspeech_amd.ops import specaug as SA  # noqa: E402


def _events(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _graph(fn, iters, per_graph=20):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(per_graph)]
    reps = max(1, iters // per_graph)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    del keep
    return e0.elapsed_time(e1) / (reps * per_graph)


def train_steps(a):
    base = [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--dummy_frames", str(a.frames),
            "--batch_size", str(a.batch), "--num_hidden", "800", "--num_rnn_layers", "5", "--cell", "gru", "--engine",
            "hip", "--max_steps", str(a.train), "--checkpoint_every", "0", "--log_every", "10"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for rnd in range(2):
        for name, extra in (("no flag", []), ("--specaug ls", ["--specaug", "ls"])):
            with tempfile.TemporaryDirectory() as d:
                r = subprocess.run(base + ["--train_dir", d] + extra, env=env, cwd=ROOT, capture_output=True, text=True)
                if r.returncode != 0:
                    raise SystemExit("training run failed:\n" + (r.stdout + r.stderr)[-3000:])
                recs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
            p50 = sorted(x["step_ms_p50"] for x in recs if "step_ms_p50" in x and x["step"] >= 40)
            p95 = sorted(x["step_ms_p95"] for x in recs if "step_ms_p95" in x and x["step"] >= 40)
            print(json.dumps({"metric": "training step, 5x BiGRU-800, batch %d x %d frames" % (a.batch, a.frames),
                              "setting": name, "round": rnd, "steps": a.train, "windows": len(p50),
                              "step_ms_p50_median": p50[len(p50) // 2], "step_ms_p50_min": p50[0],
                              "step_ms_p50_max": p50[-1], "step_ms_p95_median": p95[len(p95) // 2],
                              "last_loss": [x["loss"] for x in recs if "loss" in x][-1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--bins", type=int, default=161)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--train", type=int, default=0, metavar="STEPS", help="time whole training steps instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_specaug: no GPU visible; there is nothing to time without one")
    if a.train > 0:
        return train_steps(a)
    dev = torch.device("cuda")
    B, T, F = a.batch, a.frames, a.bins
    g = torch.Generator().manual_seed(0)
    x_host = torch.randn(B, T, F, generator=g) * 3 + 1
    lens_host = torch.randint(max(1, T - T // 10), T + 1, (B,), generator=g).to(torch.int32)
    lens_host[0] = T
    x, lens = x_host.to(dev), lens_host.to(dev)
    out = torch.empty_like(x)
    assert SA.kernels_cover(x)
    tensor = B * T * F * 4
    shape = {"B": B, "T": T, "F": F, "iters": a.iters}
    for rnd in range(2):
        for preset in ("ld", "ls"):
            pol = SA.SpecAugPolicy.parse(preset)
            flat = SA.SpecAugPolicy(nF=pol.nF, Fw=pol.Fw, nT=pol.nT, Tw=pol.Tw, p_ppm=pol.p_ppm, W=0, fill=pol.fill)
            plan = SA.specaug_plan(lens, T, F, pol, 1234, 7)
            plan0 = SA.specaug_plan(lens, T, F, flat, 1234, 7)
            mean = SA.specaug_mean(x, lens)
            aug = SA.SpecAugment(pol, 1234)
            tm, fm = R.specaug_masks(lens_host, plan.cpu(), T, F, pol.nF)
            valid = torch.arange(T)[None, :] < lens_host.long()[:, None]
            rows_masked = int(tm.sum())
            cells_masked = int(((tm[:, :, None] | fm[:, None, :]) & valid[:, :, None]).sum())
            y = x.clone()
            ops = (
                ("device copy of the tensor (yardstick)", lambda: out.copy_(x), 2 * tensor),
                ("specaug_plan", lambda: SA.specaug_plan(lens, T, F, pol, 1234, 7), B * (4 + 4 * pol.plan_width)),
                ("specaug_mean", lambda: SA.specaug_mean(x, lens), int(lens_host.sum()) * F * 4 + B * F * 4),
                # written once; read once except time-masked rows (an interpolated row reads two
                # source rows, which neighbouring output rows share: counted once)
                ("specaug_apply out of place", lambda: SA.specaug_apply(x, lens, plan, mean, pol.nF),
                 2 * tensor - rows_masked * F * 4),
                ("specaug_apply in place (W = 0)", lambda: SA.specaug_apply(y, lens, plan0, mean, pol.nF, inplace=True),
                 cells_masked * 4),
                ("SpecAugment call (plan + mean + apply)", lambda: aug(x, lens, 7), 3 * tensor),
            )
            for name, fn, nbytes in ops:
                eager = _events(fn, max(20, a.iters // 10))
                graph = _graph(fn, a.iters)
                print(json.dumps({"metric": name, "preset": preset, **shape, "round": rnd,
                                  "us_per_call_eager": round(eager * 1e3, 2),
                                  "us_per_call_graph": round(graph * 1e3, 2), "algorithm_bytes": nbytes,
                                  "GBps_graph": round(nbytes / (graph * 1e-3) / 1e9, 1)}), flush=True)
    # the host reference a numpy pass on the producer thread would cost: plan + mean + apply, fp32
    pol = SA.SpecAugPolicy.parse("ls")
    aug = SA.SpecAugment(pol, 1234)
    aug(x_host, lens_host, 7)
    t0 = time.perf_counter()
    for _ in range(3):
        aug(x_host, lens_host, 7)
    print(json.dumps({"metric": "host reference (torch/numpy, %d threads), SpecAugment call" % torch.get_num_threads(),
                      "preset": "ls", **shape, "ms_per_call": round((time.perf_counter() - t0) / 3 * 1e3, 2)}),
          flush=True)


if __name__ == "__main__":
    main()
