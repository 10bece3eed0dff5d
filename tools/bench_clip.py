#!/usr/bin/env python3
"""Cost of gradient-norm clipping (csrc/optim.hip grad_sumsq + clip_finalize, and the CLIP variant
of adam_ema) at the headline arena (46 M parameters) and at config 5's (146 M).

  python tools/bench_clip.py [--sizes 46000000,146000000] [--iters 200]

Per size, in one process after warm-up, two rounds alternating the ops (the spread), each op
timed by device events around replays of a HIP graph of 10 calls (the GPU's time for a call):
  * a device read of the gradient's bytes (torch sum: the bandwidth yardstick of the norm pass)
  * grad_sumsq + clip_finalize with plain loads and with non-temporal loads, alone
  * the same followed by the clipped adam_ema (what a clipped step runs: whether the gradient the
    norm pass leaves in the Infinity Cache helps the update that reads it next)
  * adam_ema unclipped and clipped (coef = 0.5 in the state)
One JSON line per op and round.

  python tools/bench_clip.py --train 60

times whole training steps of the headline model (5-layer BiGRU-800, batch 32 x 1000 frames) in
this process: Trainer with and without max_grad_norm = 400, with and without defer_update, the four
settings alternated over two rounds, each a fresh Trainer, device events around the last
(--train - 20) steps, flush() inside the timed region.
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deepspeech_amd.ops import _ext  # noqa: E402


def _graph(fn, iters, per_graph=10):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(per_graph)]
    reps = max(1, iters // per_graph)
    for _ in range(2):
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


def kernels(a):
    C = _ext.ext()
    dev = torch.device("cuda")
    seg = int(C.grad_sumsq_segment())
    for n in a.sizes:
        gen = torch.Generator().manual_seed(n)
        g = (1e-3 * torch.randn(n, generator=gen)).to(dev)
        p = torch.randn(n, generator=gen).to(dev)
        m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
        p16 = torch.empty(n, device=dev, dtype=torch.bfloat16)
        part = torch.empty(-(-n // seg), device=dev, dtype=torch.float32)
        state = torch.zeros(8, device=dev, dtype=torch.float32)
        half = torch.zeros(8, device=dev, dtype=torch.float32)
        half[2] = 0.5
        hy = (1e-4, 0.9, 0.999, 1e-8, 1.0, 0.999)

        def norm(nt):
            C.grad_sumsq(g, 1.0, part, 0, nt)
            C.clip_finalize(part, float("inf"), state)          # measure only: coef stays 1

        def adam(clip):
            C.adam_ema(p, g, m, v, ema, p16, *hy, None, 0, None, 0, clip)

        ops = [("device read of the gradient (torch sum)", lambda: g.sum(), 4 * n),
               ("grad_sumsq + clip_finalize, plain loads", lambda: norm(False), 4 * n),
               ("grad_sumsq + clip_finalize, non-temporal loads", lambda: norm(True), 4 * n),
               ("adam_ema unclipped", lambda: adam(None), 38 * n),
               ("adam_ema clipped (coef 0.5)", lambda: adam(half), 38 * n),
               ("norm (plain loads) + clipped adam_ema", lambda: (norm(False), adam(state)), 42 * n),
               ("norm (non-temporal loads) + clipped adam_ema", lambda: (norm(True), adam(state)), 42 * n)]
        for rnd in range(2):
            for name, fn, nbytes in ops:
                ms = _graph(fn, a.iters)
                print(json.dumps({"metric": name, "n": n, "round": rnd, "us_per_call_graph": round(ms * 1e3, 1),
                                  "algorithm_bytes": nbytes, "GBps_graph": round(nbytes / (ms * 1e-3) / 1e9, 1)}),
                      flush=True)
        del g, p, m, v, ema, p16
        torch.cuda.empty_cache()


def train_steps(a):
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.trainer import LRSchedule, Trainer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    base = DeepSpeech2(num_filters=32, num_hidden=a.hidden, num_rnn_layers=5, cell="gru").to(dev)
    feed = FixedShapeBatches(a.batch, max_frames=1000, seed=1000, pool=4)
    batches = [to_device(feed.next(), dev) for _ in range(4)]
    warm = 20
    for rnd in range(2):
        for defer in (True, False):
            for C in (0.0, 400.0):
                tr = Trainer(copy.deepcopy(base).set_engine("hip", torch.bfloat16), LRSchedule(1e-4, 10 ** 9, 0.9),
                             defer_update=defer, max_grad_norm=C)
                for i in range(warm):
                    tr.step(batches[i % 4])
                tr.flush()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.train - warm):
                    loss = tr.step(batches[i % 4])
                tr.flush()
                e1.record()
                torch.cuda.synchronize()
                rec = {"metric": "training step, 5x BiGRU-%d, batch %d x 1000 frames" % (a.hidden, a.batch),
                       "max_grad_norm": C, "defer_update": defer, "round": rnd, "steps": a.train - warm,
                       "ms_per_step": round(e0.elapsed_time(e1) / (a.train - warm), 4), "last_loss": float(loss)}
                if C:
                    st = tr.opt.clip_stats()
                    rec.update(grad_norm=st["grad_norm"], clipped_steps=st["clipped_steps"], skipped_steps=st["skipped_steps"])
                print(json.dumps(rec), flush=True)
                del tr
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[46000000, 146000000])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=800)
    ap.add_argument("--train", type=int, default=0, metavar="STEPS", help="time whole training steps instead (> 20)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: no GPU visible; there is nothing to time without one")
    if a.train > 0:
        if a.train <= 20:
            raise SystemExit("bench_clip: --train needs more than the 20 warm-up steps")
        return train_steps(a)
    return kernels(a)


if __name__ == "__main__":
    main()
