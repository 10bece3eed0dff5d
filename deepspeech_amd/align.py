"""Word timestamps and per-utterance alignment scores from CTC forced alignment.

  python -m deepspeech_amd.align --eval_data train --checkpoint_dir ../models/librispeech/train \
      --data_dir ../data/LibriSpeech/processed/ --out align.jsonl [--dummy True]

writes one JSON line per utterance (transcript, word timings, score, score_per_frame, feasible):
a low score per frame marks a transcript that does not fit its audio, the usual cleaning pass
over a training set.

Time convention. The conv front-end's output frame t sees feature frames [4t, 4t + 38)
(``infer.STRIDE`` / ``infer.RECEPTIVE``, 10 ms hop); its time is the centre of that receptive
field, ``frame_time(t) = 0.04 t + 0.19`` s. A span of output frames [a, b] (inclusive) is
reported as ``[frame_time(a) - 0.02, frame_time(b) + 0.02]`` s, half an output frame to either
side, so adjacent spans meet, and it is clamped to [0, duration] when the duration is known.

The alignment itself (``ops/align.py ctc_forced_align``: csrc/align.hip on the GPU, the oracle
``ops/reference.py ctc_viterbi_ref`` on the CPU) is the best CTC path of the given labels; on
ties it stays in a state before it advances (see ctc_viterbi_ref).
"""
from __future__ import annotations

import json
import math
import sys
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ALPHABET, BLANK
from .infer import RECEPTIVE, STRIDE
from .ops.align import Alignment, ctc_forced_align

HOP_S = 0.01                              # feature frame hop
FRAME_S = STRIDE * HOP_S                  # one output frame: 0.04 s
CENTER_S = RECEPTIVE * HOP_S / 2.0        # centre of output frame 0's receptive field: 0.19 s
SPACE = ALPHABET.index(" ")
CHAR_TO_IX = {c: i for i, c in enumerate(ALPHABET)}


class Word(NamedTuple):
    text: str
    start_s: float
    end_s: float
    confidence: float      # geometric mean of the per-frame probabilities on the word's label states


class UtteranceAlignment(NamedTuple):
    words: List[Word]
    score: float               # log-probability of the best path (-inf: no path, NaN: NaN emissions)
    score_per_frame: float     # score / output frames
    feasible: bool
    frames: int                # output frames of the utterance


def frame_time(t: float) -> float:
    """Centre of output frame t's receptive field, in seconds."""
    return FRAME_S * t + CENTER_S


def span_seconds(a: int, b: int, duration: Optional[float] = None) -> Tuple[float, float]:
    """Output frames [a, b] (inclusive) -> (start_s, end_s), clamped to [0, duration] if known."""
    lo, hi = frame_time(a) - FRAME_S / 2.0, frame_time(b) + FRAME_S / 2.0
    if duration is not None:
        lo, hi = min(max(lo, 0.0), duration), min(max(hi, 0.0), duration)
    return max(lo, 0.0), max(hi, 0.0)


def text_to_ids(text: Union[str, Sequence[int]]) -> List[int]:
    if not isinstance(text, str):
        return [int(i) for i in text]
    try:
        return [CHAR_TO_IX[c] for c in text.upper()]
    except KeyError as e:
        raise ValueError("character %r is not in the alphabet %r" % (e.args[0], ALPHABET)) from None


def ids_to_text(ids) -> str:
    return "".join(ALPHABET[int(i)] for i in ids if 0 <= int(i) < len(ALPHABET))


def tokens_to_words(alignment: Alignment, labels, n: int, duration: Optional[float] = None) -> List[Word]:
    """Words of utterance ``n``: ``labels`` is that batch's label ids ([N, Lmax] tensor / array or a
    list of id lists), split on the alphabet's space. A word spans from its first label's first
    frame to its last label's last frame (times as in the module docstring); its confidence is
    exp(sum of tok_score / frames on its label states). An utterance without a path has no words.
    Reads the alignment back from its device."""
    ts = alignment.tok_start[n].cpu().numpy()
    te = alignment.tok_end[n].cpu().numpy()
    tsc = alignment.tok_score[n].cpu().numpy()
    row = labels[n]
    row = row.cpu().tolist() if isinstance(row, torch.Tensor) else list(row)
    words: List[Word] = []
    cur: List[int] = []

    def flush():
        if cur:
            a, b = int(ts[cur[0]]), int(te[cur[-1]])
            frames = sum(int(te[i]) - int(ts[i]) + 1 for i in cur)
            conf = math.exp(float(sum(float(tsc[i]) for i in cur)) / max(1, frames))
            s, e = span_seconds(a, b, duration)
            words.append(Word(ids_to_text(row[i] for i in cur), s, e, conf))
            cur.clear()

    for i, c in enumerate(row):
        if i >= len(ts) or ts[i] < 0:          # past label_lens, or no path
            break
        if int(c) == SPACE:
            flush()
        else:
            cur.append(i)
    flush()
    return words


def _pad_labels(ids: List[List[int]]) -> Tuple[torch.Tensor, torch.Tensor]:
    L = max(1, max((len(x) for x in ids), default=1))
    lab = np.zeros((len(ids), L), np.int32)
    for i, x in enumerate(ids):
        lab[i, : len(x)] = x
    return torch.from_numpy(lab), torch.tensor([len(x) for x in ids], dtype=torch.int32)


def utterances(al: Alignment, ids: List[List[int]], lens, durations) -> List[UtteranceAlignment]:
    """Host-side view of a batch's alignment (one read-back)."""
    score = al.score.cpu().tolist()
    lens = [int(v) for v in torch.as_tensor(lens).cpu().tolist()]
    out = []
    for n, sc in enumerate(score):
        ok = math.isfinite(sc)
        words = tokens_to_words(al, ids, n, None if durations is None else durations[n]) if ok else []
        out.append(UtteranceAlignment(words, sc, sc / max(1, lens[n]), ok, lens[n]))
    return out


class Aligner:
    """Forced alignment of transcripts against a model's emissions: the model's forward on either
    engine, unidirectional or bidirectional, then ``ctc_forced_align`` on the logits where they are."""

    def __init__(self, model, features: str = "mfcc"):
        self.model = model.eval()
        self.dev = model.fc_weight.device
        self.features = features
        self._featurizer = None
        self._featurizer_key = None

    @torch.no_grad()
    def align(self, feats: torch.Tensor, seq_lens: torch.Tensor, transcripts, durations=None
              ) -> List[UtteranceAlignment]:
        """feats [N, T, F], seq_lens [N] feature frames, transcripts: strings or label-id lists.
        Durations default to seq_lens * 10 ms."""
        ids = [text_to_ids(t) for t in transcripts]
        if len(ids) != feats.shape[0]:
            raise ValueError("one transcript per utterance")
        seq_lens = torch.as_tensor(seq_lens).to(torch.int32)
        if durations is None:
            durations = [HOP_S * float(v) for v in seq_lens.cpu().tolist()]
        logits, lens = self.model(feats.to(self.dev), seq_lens.to(self.dev))
        labels, label_lens = _pad_labels(ids)
        al = ctc_forced_align(logits, lens, labels.to(self.dev), label_lens.to(self.dev), BLANK, log_probs=False)
        if self.model.engine == "hip":
            torch.cuda.synchronize(self.dev)
            from .ops import rnn as RNN
            RNN.check_errors()
        return utterances(al, ids, lens, durations)

    @torch.no_grad()
    def align_audio(self, pcm, transcripts, sample_rate: int = 16000,
                    resample: bool = False) -> List[UtteranceAlignment]:
        """pcm: [B, S] samples or a list of 1-D arrays (int16 or float), featurized on the model's
        device (ops/featurize.py AudioFeaturizer). ``resample=True`` converts ``sample_rate`` to
        16 kHz on the device first (ops/resample.py) instead of featurizing at ``sample_rate``;
        durations come from the original sample counts either way."""
        key = (int(sample_rate), bool(resample))
        if self._featurizer is None or self._featurizer_key != key:
            from .ops.featurize import AudioFeaturizer
            if resample:
                self._featurizer = AudioFeaturizer(self.features, device=self.dev, input_rate=sample_rate)
            else:
                self._featurizer = AudioFeaturizer(self.features, sample_rate=sample_rate, device=self.dev)
            self._featurizer_key = key
        if isinstance(pcm, (torch.Tensor, np.ndarray)) and getattr(pcm, "ndim", 1) == 2:
            samples = [int(pcm.shape[1])] * int(pcm.shape[0])
        else:
            samples = [int(len(u)) for u in pcm]
        feats, frames = self._featurizer(pcm)
        return self.align(feats.float(), frames, transcripts, durations=[s / float(sample_rate) for s in samples])


def main(argv=None) -> int:
    import argparse
    from . import config as C
    from .data.synthetic import to_device
    from .models import DeepSpeech2
    from .test import NUM_EXAMPLES, build_eval_data, eval_front_end
    from .utils import checkpoint as CK

    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--out", type=str, required=True, help="JSON-lines file: one alignment per utterance")
    own, rest = pre.parse_known_args(argv)
    args = C.parse_eval_args(rest)
    dev = C.resolve_device(args.device)
    engine = C.resolve_engine(args.engine, dev)
    dtype = C.resolve_dtype(args.dtype, False, dev)
    model = DeepSpeech2(**C.model_kwargs_from_args(args)).to(dev)
    model.set_engine(engine, dtype)
    path = CK.latest_checkpoint(args.checkpoint_dir)
    if path is None:
        print("No checkpoint file found")
        return 1
    tensors = {k: v for k, v in CK.load_checkpoint_file(path).items() if isinstance(v, torch.Tensor)}
    CK.load_model_from_tf(model, tensors, strict=True, use_ema=args.use_ema)
    data = build_eval_data(args)
    n = args.num_examples or NUM_EXAMPLES.get(args.eval_data, 2048)
    aligner = Aligner(model)
    front = eval_front_end(args, data, dev)       # an audio store is featurized per batch, unaugmented
    done = bad = 0
    with open(own.out, "w") as f:
        for _ in range(int(math.ceil(n / args.batch_size))):
            hb = data.next()
            b = to_device(hb, dev)
            if front is not None:
                b = front(b)
            ids = [hb.labels[i, : hb.label_lens[i]].tolist() for i in range(len(hb.label_lens))]
            for i, u in enumerate(aligner.align(b["feats"], b["seq_lens"], ids)):
                f.write(json.dumps({
                    "utterance": done, "transcript": ids_to_text(ids[i]), "feasible": u.feasible,
                    "score": u.score if u.feasible else None,
                    "score_per_frame": u.score_per_frame if u.feasible else None, "frames": u.frames,
                    "words": [{"text": w.text, "start_s": round(w.start_s, 3), "end_s": round(w.end_s, 3),
                               "confidence": w.confidence} for w in u.words]}) + "\n")
                done += 1
                bad += 0 if u.feasible else 1
    if hasattr(data, "close"):
        data.close()
    print("aligned %d utterances (%d without a path) -> %s" % (done, bad, own.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
