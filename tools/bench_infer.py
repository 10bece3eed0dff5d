#!/usr/bin/env python3
"""Streaming-inference real-time factor (BASELINE.json config 4: unidirectional GRU + CTC
beam-search decoder on one MI355X).

  python tools/bench_infer.py [--layers 5] [--hidden 800] [--seconds 20] [--chunks 0.25,0.5,1.0]
                              [--batches 1,32] [--decoders greedy,beam] [--audio] [--lm ORDER]
                              [--lookahead TAU] [--audio_rate R[,R...]]

RTF = compute seconds / audio seconds per stream (B concurrent streams share each chunk
launch, so B streams at RTF r serve B * (1 / r) x real time). Random-init weights and
synthetic 161-bin features (no checkpoint or dataset offline). One JSON line per setting.
``--audio`` streams synthetic int16 PCM through StreamingRecognizer.accept_audio instead, so the
RTF includes the featurization (csrc/featurize.hip). ``--lm ORDER`` fuses a character n-gram LM
of that order, trained on seeded synthetic text, into the beam decoder (deepspeech_amd/lm.py).
``--lookahead TAU`` puts a lookahead convolution over TAU future frames above the recurrent stack
(random weights); the RTF then includes its streaming step and the flush in finish().
``--audio_rate R`` (with ``--audio``) makes the synthetic PCM R Hz, resampled to 16 kHz on the
device inside the RTF (csrc/resample.hip); several rates, e.g. ``16000,48000``, run one after the
other in the same process so their RTFs can be read side by side.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepspeech_amd.infer import rtf  # noqa: E402
from deepspeech_amd.models import DeepSpeech2  # noqa: E402


def bench_one(a, m, eng, data, lm, extra, B, c, d, R):
    kw = dict(extra)
    if a.audio:
        kw.update(audio_rate=R)
    if lm is not None and d == "beam":
        kw.update(lm=lm, lm_weight=a.lm_weight, label_bonus=a.label_bonus)
    r, _ = rtf(m, seconds=a.seconds, chunk_s=c, batch=B, decoder=d, beam_width=a.beam_width, **kw)
    print(json.dumps({"metric": "streaming RTF (lower is better)", "model": "DS2 2xconv(32) + %dx uni-%s-%d"
                      % (a.layers, a.cell.upper(), a.hidden), "engine": eng, "streams": B,
                      "chunk_s": c, "decoder": d, "lookahead": a.lookahead, "beam_width": a.beam_width if d == "beam" else None,
                      "rtf": round(r, 5), "x_realtime_per_stream": round(1.0 / r, 1) if r > 0 else None,
                      "x_realtime_total": round(B / r, 1) if r > 0 else None,
                      "audio_s": a.seconds, "data": data, **({"audio_rate": R} if a.audio else {}),
                      **({"lm_order": a.lm, "lm_states": int(lm.compile()[0].shape[0])}
                         if "lm" in kw else {})}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=800)
    ap.add_argument("--cell", default="gru")
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--chunks", default="0.25,0.5,1.0")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--decoders", default="greedy,beam")
    ap.add_argument("--beam_width", type=int, default=16)
    ap.add_argument("--engine", default="hip")
    ap.add_argument("--audio", action="store_true", help="stream int16 PCM (featurization included in the RTF)")
    ap.add_argument("--lm", type=int, default=0, metavar="ORDER",
                    help="beam decoder with a character LM of this order (seeded synthetic text)")
    ap.add_argument("--lm_weight", type=float, default=0.8)
    ap.add_argument("--label_bonus", type=float, default=0.5)
    ap.add_argument("--lookahead", type=int, default=0, metavar="TAU",
                    help="lookahead convolution over TAU future frames (0: none)")
    ap.add_argument("--audio_rate", default="16000", metavar="R[,R...]",
                    help="sample rate(s) of the synthetic PCM of --audio (other than 16000: resampled on the device)")
    a = ap.parse_args()
    rates = [int(x) for x in a.audio_rate.split(",")] if a.audio else [16000]
    lm = None
    if a.lm > 0:
        from deepspeech_amd.lm import CharNgramLM, synthetic_corpus
        lm = CharNgramLM.train(synthetic_corpus(2000, seed=0, vocab=400), a.lm)
    extra = {"audio": True} if a.audio else {}
    data = "synthetic int16 PCM, random-init weights" if a.audio else "synthetic features, random-init weights"
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    eng = a.engine if dev.type == "cuda" else "ref"
    torch.manual_seed(0)
    m = DeepSpeech2(num_filters=32, num_hidden=a.hidden, num_rnn_layers=a.layers, cell=a.cell,
                    bidirectional=False, lookahead=a.lookahead).to(dev)
    if a.lookahead > 0:
        with torch.no_grad():
            m.lookahead_weight.normal_(0.0, (a.lookahead + 1) ** -0.5)
    m.set_engine(eng, torch.bfloat16 if eng == "hip" else torch.float32)
    rtf(m, seconds=2.0, chunk_s=0.5, batch=1, **extra)  # warm-up (plans, kernels, allocator)
    for R in rates:
        if R != 16000:
            rtf(m, seconds=2.0, chunk_s=0.5, batch=1, audio_rate=R, **extra)  # warm-up of the resampler
    for B in [int(x) for x in a.batches.split(",")]:
        for c in [float(x) for x in a.chunks.split(",")]:
            for d in a.decoders.split(","):
                for R in rates:
                    bench_one(a, m, eng, data, lm, extra, B, c, d, R)


if __name__ == "__main__":
    main()
