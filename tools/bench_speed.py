#!/usr/bin/env python3
"""Time of the speed-perturbation kernels (csrc/speed.hip) at the headline batch, next to a plain
device copy of the waveform tensor (the bandwidth yardstick) and the resampling kernel at one
ratio on the same rows.

  python tools/bench_speed.py [--batch 32] [--samples 160000] [--iters 400] [--policy 0.9,1.0,1.1]

fp32 [batch, samples] with ragged lengths, in one process after warm-up, two rounds alternating
the ops (the spread): the plan, the apply launch at the worst-case and at the tight output width,
the SpeedPerturb call (both launches and the output allocation), the policy (1.0,) (every row
copied), ``Resampler(110, 100)`` on the same rows (every row through the chain at one ratio), the
featurizer alone and the front end (speed + featurizer). Each op is timed twice: device events
around back-to-back eager calls (host launch overhead and output allocation included) and around
replays of a HIP graph of 20 calls (the GPU's time for a call). One JSON line per op and round.

  python tools/bench_speed.py --train 60

times whole training steps of the headline model (5-layer BiGRU-800, batch 32 x 1000 frames) fed
from dummy audio through the front end, in one process: without speed perturbation, with it at
the tight output width (the train driver's way: the plan of the host batch's lengths) and with it
at the policy's worst-case width, alternating, two rounds; host-to-device copy, front end and
step are all inside the timed region, the first 20 steps are left out. Nothing here is a pass/fail
criterion.
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_specaug import _events, _graph  # noqa: E402
from deepspeech_amd.ops import speed as SP  # noqa: E402


def train_steps(a):
    from deepspeech_amd.data.audio_batch import AudioFrontEnd
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.trainer import LRSchedule, Trainer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    base = DeepSpeech2(num_filters=32, num_hidden=800, num_rnn_layers=5, cell="gru").to(dev)
    policy = SP.SpeedPolicy.parse(a.policy)
    warm = 20
    if a.train <= warm:
        raise SystemExit("bench_speed: --train needs more than the %d warm-up steps" % warm)
    for rnd in range(2):
        for name in ("dummy audio", "speed_perturb %s, tight width" % policy, "speed_perturb %s, worst-case width" % policy):
            feed = FixedShapeBatches(a.batch, max_frames=1000, seed=1000, pool=4, audio=True)
            sp = SP.SpeedPerturb(policy, 1234) if "speed" in name else None
            front = AudioFrontEnd("mfcc", dev, speed=sp, max_frames=1800)
            tr = Trainer(copy.deepcopy(base).set_engine("hip", torch.bfloat16), LRSchedule(1e-4, 10 ** 9, 0.9), defer_update=True)
            frames, drawn = 0, {}

            def step(i):
                nonlocal frames
                hb = feed.next()
                batch = front(to_device(hb, dev), i, training=True, host=hb if "tight" in name else None)
                frames += batch["feats"].shape[1]
                if sp is not None and i % 10 == 0:                   # a look at the ratios: one small read-back in ten steps
                    for p in sp.plan[:, 0].tolist():
                        drawn[p] = drawn.get(p, 0) + 1
                return tr.step(batch)
            for i in range(warm):
                step(i)
            tr.flush()
            torch.cuda.synchronize()
            frames, drawn = 0, {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(warm, a.train):
                loss = step(i)
            tr.flush()
            e1.record()
            torch.cuda.synchronize()
            n = a.train - warm
            print(json.dumps({"metric": "training step from dummy audio, 5x BiGRU-800, batch %d x 1000 frames" % a.batch,
                              "setting": name, "round": rnd, "steps": n, "ms_per_step": round(e0.elapsed_time(e1) / n, 3),
                              "mean_padded_frames": round(frames / n, 1), "ratios_seen": drawn, "last_loss": float(loss)}),
                  flush=True)
            del tr
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--policy", default="0.9,1.0,1.1")
    ap.add_argument("--train", type=int, default=0, metavar="STEPS", help="time whole training steps instead (> 20)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speed: no GPU visible; there is nothing to time without one")
    if a.train > 0:
        return train_steps(a)
    from deepspeech_amd.data.audio_batch import AudioFrontEnd
    from deepspeech_amd.ops import _ext
    from deepspeech_amd.ops.featurize import AudioFeaturizer
    from deepspeech_amd.ops.resample import Resampler
    dev = torch.device("cuda")
    B, S = a.batch, a.samples
    g = torch.Generator().manual_seed(0)
    x_host = torch.randn(B, S, generator=g) * 0.1
    lens_host = (torch.randint(S - S // 10, S + 1, (B,), generator=g) // 160 * 160).to(torch.int32)
    lens_host[0] = S
    x, lens = x_host.to(dev), lens_host.to(dev)
    assert SP.kernels_cover(x)
    policy = SP.SpeedPolicy.parse(a.policy)
    sp, ident = SP.SpeedPerturb(policy, 1234), SP.SpeedPerturb(SP.SpeedPolicy((100,)), 1234)
    C = _ext.ext().speed
    y, out_lens = sp(x, lens, 7)
    plan, table, vtab = sp.plan, policy.table.to(dev), policy.vtab
    worst, tight = y.shape[1], sp.tight_width(lens_host, B, S, 7)
    y_tight = torch.empty(B, tight, device=dev)
    rs = Resampler(110, 100, device=dev)
    fz = AudioFeaturizer("mfcc", device=dev, normalize="utterance")
    front = AudioFrontEnd("mfcc", dev, speed=sp)
    batch = {"feats": x.view(B, S // 160, 160), "seq_lens": (lens // 160).to(torch.int32),
             "labels": torch.zeros(B, 4, dtype=torch.int32, device=dev), "label_lens": torch.ones(B, dtype=torch.int32, device=dev)}
    out = torch.empty_like(x)
    rows = {p: int((plan[:, 0] == p).sum()) for p in policy.pcts}
    shape = {"B": B, "S": S, "iters": a.iters, "policy": str(policy), "rows_per_percent": rows, "worst_width": worst,
             "tight_width": tight}
    taps = {r[0]: r[3] for r in policy.records}
    fma = sum(n * taps[p] for p, n in plan.tolist())
    ops = (
        ("device copy of the tensor (yardstick)", lambda: out.copy_(x)),
        ("speed plan", lambda: SP.speed_plan(lens, B, S, policy, 1234, 7, device=dev)),
        ("speed apply, worst-case width", lambda: C.apply(x, lens, plan, table, vtab, y, out_lens, False)),
        ("speed apply, tight width", lambda: C.apply(x, lens, plan, table, vtab, y_tight, out_lens, True)),
        ("SpeedPerturb call (plan + apply), worst-case width", lambda: sp(x, lens, 7)),
        ("SpeedPerturb call, policy 1.0 (every row copied)", lambda: ident(x, lens, 7)),
        ("Resampler(110, 100) on the same rows", lambda: rs(x, lens)),
        ("AudioFeaturizer mfcc, utterance statistics", lambda: fz(x, lens)),
        ("front end (SpeedPerturb + AudioFeaturizer), worst-case width", lambda: front(batch, 7, training=True)),
    )
    for rnd in range(2):
        for name, fn in ops:
            eager = _events(fn, max(20, a.iters // 10))
            graph = _graph(fn, a.iters)
            rec = {"metric": name, **shape, "round": rnd, "us_per_call_eager": round(eager * 1e3, 2),
                   "us_per_call_graph": round(graph * 1e3, 2)}
            if name.startswith("speed apply"):
                rec["gfma_per_s"] = round(fma / (graph * 1e-3) / 1e9, 1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
