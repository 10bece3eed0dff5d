#!/usr/bin/env python3
"""Time of the resampling kernel (csrc/resample.hip) next to its yardsticks.

  python tools/bench_resample.py [--batch 64] [--seconds 30] [--iters 20] [--rounds 2]
                                 [--rates 8000,44100,48000]

For ``batch`` x ``seconds`` of int16 PCM already on the device at each rate, converted to
16 kHz: ms per call (device events around ``iters`` back-to-back calls, launch overhead and the
output allocation included) of

  * the kernel (``Resampler.__call__``),
  * a device ``copy_`` of the output tensor (the floor of anything that writes that tensor),
  * the torch composite of the same definition (``resample_composite``; 2 iterations), and
  * the whole ``AudioFeaturizer`` call at that ``input_rate`` next to the same featurizer on
    16 kHz PCM of the same duration (mfcc, per-utterance statistics),

the settings alternated over ``rounds`` rounds in one process, and once the fp64 host oracle
(``resample_ref``) on one utterance. The kernel is also checked against the composite on the
benchmark input (max |difference| over max |output|). One JSON line per setting. Nothing here
is a pass/fail criterion.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepspeech_amd.ops.featurize import AudioFeaturizer  # noqa: E402
from deepspeech_amd.ops.reference import resample_ref  # noqa: E402
from deepspeech_amd.ops.resample import Resampler, resample_composite  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rates", default="8000,44100,48000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"metric": "resample", "skipped": "no GPU visible"}), flush=True)
        return 1
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    n16 = int(a.seconds * 16000)
    pcm16 = (torch.randn(a.batch, n16, generator=g) * 3000.0).clamp_(-32768, 32767).to(torch.int16).to(dev)
    fz16 = AudioFeaturizer("mfcc", device=dev)
    for rate in [int(r) for r in a.rates.split(",")]:
        n = int(a.seconds * rate)
        pcm = (torch.randn(a.batch, n, generator=g) * 3000.0).clamp_(-32768, 32767).to(torch.int16).to(dev)
        rs = Resampler(rate, device=dev)
        fz = AudioFeaturizer("mfcc", device=dev, input_rate=rate)
        y, _ = rs(pcm)
        K, L, M = rs.K, rs.L, rs.M

        def composite(x, rs=rs, n_out=y.shape[1]):
            return resample_composite(x, None, rs.h, rs.L, rs.M, -(rs.K // 2 - 1), 0, n_out, True)

        yc, _ = composite(pcm)
        rel = float((y - yc).abs().max() / yc.abs().max())
        del yc
        dst = torch.empty_like(y)
        base = {"in_rate": rate, "L": L, "M": M, "K": K, "batch": a.batch, "seconds": a.seconds,
                "outputs": int(y.numel()), "kernel": bool(rs.use_kernel)}
        ops = [
            ("resample kernel", lambda: rs(pcm), a.iters),
            ("device copy of the output", lambda: dst.copy_(y), a.iters),
            ("torch composite", lambda: composite(pcm), 2),
            ("AudioFeaturizer(input_rate)", lambda: fz(pcm), a.iters),
            ("AudioFeaturizer at 16 kHz", lambda: fz16(pcm16), a.iters),
        ]
        res = {name: [] for name, _, _ in ops}
        for _ in range(a.rounds):
            for name, fn, iters in ops:
                res[name].append(round(timed(fn, iters), 4))
        for name, _, _ in ops:
            row = dict(base, metric=name, ms_per_call=res[name])
            if name == "resample kernel":
                ms = min(res[name])
                row.update(max_diff_vs_composite_rel=rel, gfma_per_s=round(y.numel() * K / ms / 1e6, 1),
                           x_realtime=round(a.batch * a.seconds / (ms * 1e-3)))
            print(json.dumps(row), flush=True)
        x1 = pcm[0].cpu().numpy()
        t0 = time.perf_counter()
        resample_ref(x1, rate, 16000)
        print(json.dumps(dict(base, metric="fp64 host oracle (resample_ref), one utterance", batch=1,
                              ms_per_call=round((time.perf_counter() - t0) * 1e3, 1))), flush=True)
        del pcm, y, dst
    return 0


if __name__ == "__main__":
    sys.exit(main())
