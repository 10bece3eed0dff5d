#!/usr/bin/env python3
"""Time of CTC forced alignment on the GPU (csrc/align.hip) next to the host path and the CTC loss.

  python tools/bench_align.py [--iters 1000]

At the headline shape after the convs (N = 32 utterances, T = 241 output frames, 150 labels each,
K = 29) and at N = 1, in one process after warm-up:
  * ``ctc_forced_align`` on fp32 logits (log-softmax + Viterbi + backtrack) and on ready log-probs,
    device events around ``iters`` back-to-back eager calls (host launch overhead and the op's
    output / workspace allocations included, no host copy), and around replays of a HIP graph of
    10 calls (the GPU's time for a call, host out of the way);
  * the same on log-probs whose last frame is -inf: the forward pass runs whole, finds no finite
    path and skips the backtrack, which splits a call into its two passes;
  * the host path a user has without the kernel: copy the log-probs out, run ``ctc_viterbi_ref``;
  * ``ctc_loss_hip`` (log-softmax + alpha/beta recursion + gradient) on the same logits and labels.
One JSON line per setting.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepspeech_amd.ops import reference as R  # noqa: E402
from deepspeech_amd.ops.align import ctc_forced_align  # noqa: E402
from deepspeech_amd.ops.ctc import ctc_loss_hip  # noqa: E402

K, BLANK = 29, 28


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


def _graph(fn, iters, per_graph=10):
    """ms per call with the host out of the way: per_graph calls captured into one HIP graph,
    replayed until ``iters`` calls have run, device events around the replays."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=241)
    ap.add_argument("--labels", type=int, default=150)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"metric": "ctc_forced_align", "skipped": "no GPU visible"}))
        return
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    for N in (32, 1):
        T, L = a.frames, a.labels
        g = torch.Generator().manual_seed(N)
        logits = (2.0 * torch.randn(T, N, K, generator=g)).to(dev)
        lp = torch.log_softmax(logits, -1)
        lp_dead = lp.clone()
        lp_dead[T - 1] = float("-inf")
        lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        labels = torch.from_numpy(rng.integers(0, BLANK, size=(N, L)).astype(np.int32)).to(dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        shape = {"N": N, "T": T, "labels": L, "K": K, "iters": a.iters}
        ops = (("ctc_forced_align, fp32 logits",
                lambda: ctc_forced_align(logits, lens, labels, label_lens, BLANK, log_probs=False)),
               ("ctc_forced_align, fp32 log-probs",
                lambda: ctc_forced_align(lp, lens, labels, label_lens, BLANK, log_probs=True)),
               # last frame -inf: the whole forward pass runs, finds no finite path and skips the backtrack
               ("ctc_forced_align, fp32 log-probs with a -inf last frame (forward pass only, no backtrack)",
                lambda: ctc_forced_align(lp_dead, lens, labels, label_lens, BLANK, log_probs=True)),
               ("ctc_loss_hip (log-softmax + alpha/beta + gradient)",
                lambda: ctc_loss_hip(logits, lens, labels, label_lens, BLANK)))
        for _ in range(2):                           # two rounds, alternating the ops: the spread
            for name, fn in ops:
                print(json.dumps({"metric": name, **shape, "ms_per_call_eager": round(_events(fn, a.iters), 4),
                                  "ms_per_call_graph": round(_graph(fn, a.iters), 4)}), flush=True)
        got = ctc_forced_align(lp, lens, labels, label_lens, BLANK, log_probs=True)
        torch.cuda.synchronize()
        reps = 3 if N == 1 else 1
        t0 = time.perf_counter()
        for _ in range(reps):
            host = R.ctc_viterbi_ref(lp.cpu(), lens.cpu(), labels.cpu(), label_lens.cpu(), BLANK)
        hms = (time.perf_counter() - t0) / reps * 1e3
        same = bool(torch.equal(host[4], got.score.cpu()) and torch.equal(host[0], got.path.cpu()))
        print(json.dumps({"metric": "host path: copy log-probs out + ctc_viterbi_ref (numpy, one thread)", **shape,
                          "ms_per_call": round(hms, 2), "matches_kernel": same}), flush=True)


if __name__ == "__main__":
    main()
