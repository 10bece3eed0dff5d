#!/usr/bin/env python3
"""Time of the recurrent-stack dropout kernel (csrc/dropout.hip) at the headline hand-over tensor
(241 x 32 x 800 bf16: 1000 input frames, batch 32, H = 800) next to a plain device copy of the
same tensor (the bandwidth yardstick: it moves the same bytes as the out-of-place form).

  python tools/bench_dropout.py [--steps 241] [--batch 32] [--hidden 800] [--iters 4000]

Out of place and in place, element and locked, in one process after warm-up, two rounds
alternating the ops (the spread). Each op is timed twice: device events around back-to-back eager
calls (host launch overhead and the output allocation included) and around replays of a HIP graph
of 20 calls (the GPU's time for a call). GB/s = the bytes the form moves over the graph time. One
JSON line per op and round.

  python tools/bench_dropout.py --train 120

times the training step of `python -m deepspeech_amd.train --dummy True` at the headline model
(5-layer BiGRU-800, batch 32 x 1000 frames) with --rnn_dropout 0.1 and without the flag,
alternating, two processes each: the median of the windows' step_ms_p50 (device events between
steps) that the driver writes to metrics.jsonl, the first 40 steps left out.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deepspeech_amd.ops import dropout as D  # noqa: E402


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
    base = [sys.executable, "-m", "deepspeech_amd.train", "--dummy", "True", "--dummy_frames", "1000",
            "--batch_size", str(a.batch), "--num_hidden", str(a.hidden), "--num_rnn_layers", "5", "--cell", "gru",
            "--engine", "hip", "--max_steps", str(a.train), "--checkpoint_every", "0", "--log_every", "10"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for rnd in range(2):
        for name, extra in (("no flag", []), ("--rnn_dropout 0.1", ["--rnn_dropout", "0.1"])):
            with tempfile.TemporaryDirectory() as d:
                r = subprocess.run(base + ["--train_dir", d] + extra, env=env, cwd=ROOT, capture_output=True, text=True)
                if r.returncode != 0:
                    raise SystemExit("training run failed:\n" + (r.stdout + r.stderr)[-3000:])
                recs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
            p50 = sorted(x["step_ms_p50"] for x in recs if "step_ms_p50" in x and x["step"] >= 40)
            p95 = sorted(x["step_ms_p95"] for x in recs if "step_ms_p95" in x and x["step"] >= 40)
            print(json.dumps({"metric": "training step, 5x BiGRU-%d, batch %d x 1000 frames" % (a.hidden, a.batch),
                              "setting": name, "round": rnd, "steps": a.train, "windows": len(p50),
                              "step_ms_p50_median": p50[len(p50) // 2], "step_ms_p50_min": p50[0],
                              "step_ms_p50_max": p50[-1], "step_ms_p95_median": p95[len(p95) // 2],
                              "last_loss": [x["loss"] for x in recs if "loss" in x][-1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=241, help="recurrence steps T of the tensor")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=800)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--train", type=int, default=0, metavar="STEPS", help="time whole training steps instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dropout: no GPU visible; there is nothing to time without one")
    if a.train > 0:
        return train_steps(a)
    dev = torch.device("cuda")
    T, N, H = a.steps, a.batch, a.hidden
    x = torch.randn(T, N, H, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(dev)
    y, out = x.clone(), torch.empty_like(x)
    st = D.DropoutState(dev)
    st.set(7, 0)
    assert D.kernel_covers(x, st.ctr)
    thr = D.threshold(0.1)
    tensor = x.numel() * 2
    shape = {"T": T, "N": N, "H": H, "thr": thr, "iters": a.iters}
    ops = [("device copy of the tensor (yardstick)", lambda: out.copy_(x), 2 * tensor)]
    for locked in (False, True):
        mode = "locked" if locked else "element"
        ops.append(("seq_dropout out of place, " + mode,
                    lambda locked=locked: D._apply(x, st.ctr, 1234, 2, thr, locked, False), 2 * tensor))
        ops.append(("seq_dropout in place, " + mode,
                    lambda locked=locked: D._apply(y, st.ctr, 1234, 2, thr, locked, True), 2 * tensor))
    for rnd in range(2):
        # once per step, outside any graph: eager only
        print(json.dumps({"metric": "DropoutState.set (multi_fill of two words)", "round": rnd,
                          "us_per_call_eager": round(_events(lambda: st.set(7, 0), 200) * 1e3, 2)}), flush=True)
        for name, fn, nbytes in ops:
            eager = _events(fn, max(20, a.iters // 10))
            graph = _graph(fn, a.iters)
            print(json.dumps({"metric": name, **shape, "round": rnd, "us_per_call_eager": round(eager * 1e3, 2),
                              "us_per_call_graph": round(graph * 1e3, 2), "algorithm_bytes": nbytes,
                              "GBps_graph": round(nbytes / (graph * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
