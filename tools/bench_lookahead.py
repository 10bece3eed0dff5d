#!/usr/bin/env python3
"""Time of the lookahead convolution kernels (csrc/lookahead.hip) next to a plain device copy of
the same tensor (the bandwidth yardstick) and the torch composite of the same definition on the
device (tau + 1 or more launches).

  python tools/bench_lookahead.py [--frames 241] [--batch 32] [--hidden 800] [--tau 20] [--iters 20000]

At the headline shape after the convs (T = 241 output frames, B = 32, H = 800), tau = 20, ragged
lengths, in one process after warm-up, two rounds alternating the ops (the spread): forward, data
gradient, weight gradient (partials kernel + col_sum) and the streaming step at n = 13 frames.
Each op is timed twice: device events around back-to-back eager calls (host launch overhead and
the output allocation included) and around replays of a HIP graph of 20 calls (the GPU's time for
a call, host out of the way). GB/s = the bytes the algorithm needs (each activation tensor read or
written once, the weights once; for the weight gradient also its fp32 result) over the graph time.
One JSON line per op and round.

  python tools/bench_lookahead.py --train 40 [--lookahead 20]

times whole training steps instead (Trainer.step as bench.py drives it: arena, carried optimizer
update, synthetic 10-s utterances) of a 5-layer unidirectional GRU-800 at batch 32, with a
lookahead layer of that many frames or without one: one process per setting, one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepspeech_amd.ops import lookahead as LA  # noqa: E402


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
    import time
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.ops import rnn as RNN
    from deepspeech_amd.trainer import LRSchedule, Trainer
    dev = torch.device("cuda")
    torch.manual_seed(1234)
    m = DeepSpeech2(num_filters=32, num_hidden=a.hidden, num_rnn_layers=a.layers, cell="gru", bidirectional=False,
                    lookahead=a.lookahead).to(dev)
    if a.lookahead > 0:
        with torch.no_grad():
            m.lookahead_weight.normal_(0.0, (a.lookahead + 1) ** -0.5)
    m.set_engine("hip", torch.bfloat16)
    tr = Trainer(m, LRSchedule(1e-4, 10 ** 9, 0.9), moving_avg_decay=0.9999, defer_update=True)
    feed = FixedShapeBatches(a.batch, max_frames=1000, seed=1000, pool=4)
    batches = [to_device(feed.next(), dev) for _ in range(4)]
    for i in range(10):
        tr.step(batches[i % 4])
    tr.flush()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(3):                                   # three timed windows: the spread
        t0 = time.perf_counter()
        for i in range(a.train):
            loss = tr.step(batches[i % 4])
        tr.flush()
        torch.cuda.synchronize()
        rounds.append(round((time.perf_counter() - t0) / a.train * 1e3, 3))
    RNN.check_errors()
    print(json.dumps({"metric": "training step, %dx uni-GRU-%d, batch %d x 10 s" % (a.layers, a.hidden, a.batch),
                      "lookahead": a.lookahead, "steps_per_window": a.train, "ms_per_step_windows": rounds,
                      "ms_per_step_best": min(rounds), "loss": round(float(loss), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=241)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=800)
    ap.add_argument("--tau", type=int, default=20)
    ap.add_argument("--stream_frames", type=int, default=13)
    ap.add_argument("--iters", type=int, default=20000)
    ap.add_argument("--train", type=int, default=0, metavar="STEPS", help="time whole training steps instead")
    ap.add_argument("--lookahead", type=int, default=0, help="--train: frames of lookahead (0: no layer)")
    ap.add_argument("--layers", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookahead: no GPU visible; there is nothing to time without one")
    if a.train > 0:
        return train_steps(a)
    dev = torch.device("cuda")
    T, B, H, tau, n = a.frames, a.batch, a.hidden, a.tau, a.stream_frames
    g = torch.Generator().manual_seed(0)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)   # noqa: E731
    h, dr, w = bf(T, B, H), bf(T, B, H), (torch.randn(H, tau + 1, generator=g) * (tau + 1) ** -0.5).to(
        torch.bfloat16).to(dev)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    lens[0] = T
    out, dw = torch.empty_like(h), torch.empty(H, tau + 1, device=dev)
    hist, x = torch.zeros(tau, B, H, dtype=torch.bfloat16, device=dev), bf(n, B, H)
    assert LA.kernels_cover(h, w) and LA.kernels_cover(x, w)
    act = T * B * H * 2
    wb = H * (tau + 1) * 2
    ops = (
        ("device copy of the activation tensor (yardstick)", lambda: out.copy_(h), 2 * act),
        ("lookahead_fwd", lambda: LA.lookahead_fwd(h, w, lens, out=out), 2 * act + wb),
        ("lookahead_bwd_data", lambda: LA.lookahead_bwd_data(dr, w, lens, out=out), 2 * act + wb),
        ("lookahead_bwd_weight (partials + col_sum)", lambda: LA.lookahead_bwd_weight(dr, h, lens, tau, dw),
         2 * act + 2 * wb),
        ("lookahead_stream, n = %d" % n, lambda: LA.lookahead_stream(hist, x, w), (2 * n + 2 * tau) * B * H * 2 + wb),
        ("torch composite forward (%d taps)" % (tau + 1), lambda: LA._composite_fwd(h, w, lens), 2 * act + wb),
        ("torch composite data gradient", lambda: LA._composite_bwd_data(dr, w, lens), 2 * act + wb),
        ("torch composite weight gradient", lambda: LA._composite_bwd_weight(dr, h, lens, tau + 1), 2 * act + 2 * wb),
    )
    shape = {"T": T, "B": B, "H": H, "tau": tau, "iters": a.iters}
    for rnd in range(2):
        for name, fn, nbytes in ops:
            slow = "composite" in name
            eager = _events(fn, max(20, a.iters // (100 if slow else 10)))
            graph = _graph(fn, max(20, a.iters // (20 if slow else 1)))
            print(json.dumps({"metric": name, **shape, "round": rnd, "us_per_call_eager": round(eager * 1e3, 2),
                              "us_per_call_graph": round(graph * 1e3, 2), "algorithm_bytes": nbytes,
                              "GBps_graph": round(nbytes / (graph * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
