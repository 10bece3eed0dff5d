"""Streaming inference (BASELINE.json north-star config 4: unidirectional GRU + CTC
beam-search decoder, real-time factor on one MI355X).

The reference only evaluates whole utterances (src/deepSpeech_test.py:112-136, greedy
CTC on a bidirectional model). A unidirectional model (``rnn_type='uni-dir'``, which the
reference's NHWC path supports: src/deepSpeech.py:173-183) can instead run on audio as it
arrives:

  * conv front-end: output frame t2 sees input frames [4*t2, 4*t2 + 38) (two strided VALID
    convs, kernel 20 / 10, stride 2 / 2 in time), so each chunk re-runs the convs on the
    38-frame-overlapping slice that produces exactly the NEW output frames; BatchNorm is in
    inference mode (running statistics), so frames are independent;
  * recurrent stack: every layer carries its final hidden state to the next chunk (the
    persistent kernels start from an initial state: ops/rnn.py:recurrent_layer_infer);
  * head + log-softmax per new frame; greedy decoding collapses across chunk boundaries
    incrementally, and the prefix beam search also advances chunk by chunk, so a transcript is
    ready when the audio ends: on the GPU the beams stay on the device (csrc/beam.hip, one
    launch per chunk, no log-prob copy), on the CPU the native runtime runs it (one host
    thread per stream group).

Lookahead models (``DeepSpeech2(lookahead=tau)``): the lookahead convolution above the top
recurrent layer gives output frame t the recurrent outputs of frames t .. t + tau, so the
recogniser keeps the last tau recurrent outputs in a static buffer (``hist``, beside the
recurrent states, inside the graph on the graph path) and every chunk of ``new`` recurrent frames
yields the outputs of frames [done - tau, done - tau + new); those below 0 are dropped on the
host. ``finish()`` pushes tau zero frames through to flush the last tau outputs. Frame t is still
frame t (the time convention of align.py is unchanged); what accept() returns simply lags the
audio by tau output frames of 40 ms each.

Batched streams: ``StreamingRecognizer`` takes [B, T_chunk, F] chunks of B concurrent
streams (equal chunk schedule, per-stream valid lengths), which is how a server batches.
"""
from __future__ import annotations

import os
import time
from typing import List, Optional

import numpy as np
import torch

from . import BLANK
from .models.deepspeech2 import DeepSpeech2, conv_out_len
from .ops import reference as R

RECEPTIVE = 38     # input frames seen by one output frame (see module docstring)
STRIDE = 4         # input frames per output frame


def frames_out(T: int) -> int:
    return conv_out_len(T)[1] if T >= RECEPTIVE else 0


class StreamingRecognizer:
    def __init__(self, model: DeepSpeech2, decoder: str = "greedy", beam_width: int = 16, batch: int = 1,
                 graphs: Optional[bool] = None, features: str = "mfcc", audio_gain: Optional[float] = None,
                 lm=None, lm_weight: float = 1.0, label_bonus: float = 0.0, audio_rate: int = 16000):
        """``lm`` (a deepspeech_amd.lm.CharNgramLM, beam decoder only): shallow fusion with weight
        ``lm_weight`` and a per-label bonus ``label_bonus`` (ops/decode.py). ``audio_rate``: the
        sample rate of the PCM given to accept_audio(); other than 16 kHz it is resampled on the
        device first (ops/resample.py), which delays the audio by half the filter's taps."""
        if model.bidirectional:
            raise ValueError("streaming needs a unidirectional model (rnn_type='uni-dir')")
        # accept_audio(): PCM is featurized on the model's device (ops/featurize.py) with a fixed
        # gain (None: 1/32768 for int16 PCM, 1 for float); the featurizer is built on first use
        self.features = features
        self.audio_gain = audio_gain
        self.audio_rate = int(audio_rate)
        self._featurizer = None
        self._audio = None
        self.model = model.eval()
        self.decoder = decoder
        self.beam_width = beam_width
        if lm is not None and decoder != "beam":
            raise ValueError("a language model needs decoder='beam'")
        self.lm, self.lm_weight, self.label_bonus = lm, float(lm_weight), float(label_bonus)
        self.B = batch
        self.dev = model.fc_weight.device
        # HIP graphs: a chunk's ~40 launches (conv front-end, 5 x (projection GEMM, sentinel
        # fill, persistent recurrence), head, log-softmax, argmax) are captured once per chunk
        # shape and replayed, so the per-chunk cost is GPU time, not host launch overhead.
        # The recurrent state lives in static buffers the graph reads and rewrites.
        if graphs is None:
            graphs = os.environ.get("DS2_INFER_GRAPHS", "1") != "0"
        self.use_graphs = bool(graphs) and self.dev.type == "cuda" and model.engine == "hip"
        self._graphs = {}
        self._h = None
        # lookahead model: the last tau recurrent outputs (static, zeroed by reset())
        self.tau = int(getattr(model, "lookahead", 0))
        self._hist = None
        self.reset()

    def reset(self) -> None:
        self.buf = torch.zeros(self.B, 0, self.model.freq_bins, device=self.dev)
        self.buf_start = 0                  # absolute frame index of buf[:, 0]
        self.total = 0                      # frames received
        self.done = 0                       # output (post-conv) frames emitted
        self.states: List[Optional[torch.Tensor]] = [None] * len(self.model.rnn)
        if self._h is not None:
            for h in self._h:
                h.zero_()
        if self._hist is not None:
            self._hist.zero_()
        self.emitted = 0                    # output frames handed to the head and the decoder
        self._flushed = False
        self.logprobs: List[torch.Tensor] = []
        self.beams = None
        self.gbeams = None
        if self.decoder == "beam":
            from .ops.decode import GpuBeamSearch
            if self.dev.type == "cuda" and self.beam_width <= GpuBeamSearch.MAX_BEAM:
                self.gbeams = GpuBeamSearch(self.B, self.beam_width, BLANK, -10.0, self.dev, lm=self.lm,
                                            lm_weight=self.lm_weight, label_bonus=self.label_bonus)
            elif self.lm is None:
                from .runtime import native
                self.beams = native.load().BatchBeamSearch(self.B, self.beam_width, BLANK, -10.0)
            else:
                from .ops.decode import host_lm
                from .runtime import native
                self.beams = native.load().BatchBeamSearch(
                    self.B, self.beam_width, BLANK, -10.0,
                    lm=host_lm(self.lm, self.lm_weight, self.label_bonus, BLANK))
        self.last_sym = [-1] * self.B
        self.greedy: List[List[int]] = [[] for _ in range(self.B)]
        self.compute_s = 0.0
        self._audio = None if self._featurizer is None else self._featurizer.stream(self.B)

    @torch.no_grad()
    def accept_audio(self, pcm, final: bool = False) -> List[List[int]]:
        """Feed [B, S_c] PCM samples (int16 or float, at ``audio_rate``, 16 kHz unless the
        recognizer was built with another); the feature frames they complete go
        through accept(). ``final=True`` also emits the zero-padded last frame. Returns the newly
        decoded (greedy) labels per stream."""
        t0 = time.perf_counter()
        if self._featurizer is None:
            from .ops.featurize import AudioFeaturizer
            self._featurizer = AudioFeaturizer(self.features, device=self.dev, normalize="fixed",
                                               gain=self.audio_gain, input_rate=self.audio_rate)
            self._audio = self._featurizer.stream(self.B)
        feats = self._audio.push(pcm, final=final)
        # no sync here: the kernels run ahead of accept()'s on the same stream, so their GPU time
        # falls inside accept()'s timed section; this one covers the host side of the push
        self.compute_s += time.perf_counter() - t0
        if feats.shape[1] == 0:
            return [[] for _ in range(self.B)]
        return self.accept(feats)

    @torch.no_grad()
    def accept(self, chunk: torch.Tensor) -> List[List[int]]:
        """Feed [B, T_c, F] feature frames; returns the newly decoded (greedy) labels per stream.
        With a lookahead model they are the labels of the frames tau (40 ms each) before the ones
        this chunk completed; the last tau frames come out of finish()."""
        if self._flushed:
            raise RuntimeError("the stream was finished; reset() starts a new one")
        t0 = time.perf_counter()
        m = self.model
        chunk = chunk.to(self.dev, torch.float32)
        self.buf = torch.cat([self.buf, chunk], 1)
        self.total += chunk.shape[1]
        t2_total = frames_out(self.total)
        new = t2_total - self.done
        out: List[List[int]] = [[] for _ in range(self.B)]
        if new <= 0:
            return out
        lo = STRIDE * self.done - self.buf_start
        hi = STRIDE * (t2_total - 1) + RECEPTIVE - self.buf_start
        feats = self.buf[:, lo:hi]
        if m.engine == "hip":
            feats = feats.to(m.compute_dtype)
        if not m.stack_fix:
            raise ValueError("streaming requires stack_fix=True")
        # lookahead: this chunk yields frames [done - tau, done - tau + new); those below 0 go
        drop = min(new, max(0, self.tau - self.done))
        if self.use_graphs:
            lp, best_t = self._graph_chunk(feats.contiguous(), drop)
        else:
            x = m.frontend(feats)                              # [new, B, C*F2]
            assert x.shape[0] == new, (x.shape, new)
            lens = torch.full((self.B,), new, dtype=torch.int32, device=self.dev)
            for i, layer in enumerate(m.rnn):
                x, self.states[i] = self._layer(layer, x, lens, self.states[i])
            lp, best_t = self._head(self._lookahead_step(x), drop)
        assert (0 if lp is None else lp.shape[0]) == new - drop, (None if lp is None else lp.shape, new, drop)
        out = self._emit(lp, best_t)
        self.done = t2_total
        # keep only the input frames future outputs can still see
        keep_from = STRIDE * self.done
        if keep_from > self.buf_start:
            self.buf = self.buf[:, keep_from - self.buf_start:]
            self.buf_start = keep_from
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        self.compute_s += time.perf_counter() - t0
        if m.engine == "hip":
            from .ops import rnn as RNN
            RNN.check_errors()        # after the chunk's sync: one 4-byte read
        return out

    def _emit(self, lp, best_t) -> List[List[int]]:
        """Hand the log-probs [n, B, K] of n more output frames to the stored log-probs, the beam
        search and the greedy merge; returns the newly decoded (greedy) labels per stream."""
        out: List[List[int]] = [[] for _ in range(self.B)]
        if lp is None or lp.shape[0] == 0:
            return out
        n = lp.shape[0]
        self.logprobs.append(lp)
        best = best_t.cpu().numpy()                            # [n, B]
        if self.gbeams is not None:
            # prefix beam search advances chunk by chunk, beams resident on the device
            self.gbeams.feed(lp)
        elif self.beams is not None:
            # prefix beam search advances chunk by chunk (beams carried in the native
            # runtime, streams decoded on parallel host threads)
            self.beams.feed(lp.cpu().numpy(), np.full((self.B,), n, dtype=np.int32))
        for b in range(self.B):
            for t in range(best.shape[0]):
                s = int(best[t, b])
                if s != self.last_sym[b] and s != BLANK:
                    out[b].append(s)
                self.last_sym[b] = s
            self.greedy[b].extend(out[b])
        self.emitted += n
        return out

    def _lookahead_step(self, x):
        """Recurrent outputs x [n, B, H] of n more frames -> the lookahead layer's outputs of the n
        frames tau before them (x itself for a model without the layer); ``hist`` carries the
        last tau recurrent outputs to the next call, in place (capturable)."""
        if self.tau == 0:
            return x
        m = self.model
        if self._hist is None:
            self._hist = torch.zeros(self.tau, self.B, x.shape[2], device=self.dev, dtype=x.dtype)
        if m.engine == "hip":
            from .ops import lookahead as LA
            return LA.lookahead_stream(self._hist, x.contiguous(), LA.shadow_of(m.lookahead_weight))
        return R.lookahead_stream_ref(self._hist, x, m.lookahead_weight)

    def _head(self, x, drop: int):
        """(log-probs, argmax) of the frames of x [n, B, H] after the first ``drop``; (None, None)
        when none is left (the first chunks of a lookahead stream)."""
        x = x[drop:]
        if x.shape[0] == 0:
            return None, None
        lp = torch.log_softmax(self.model.head(x).float(), -1)
        return lp, lp.argmax(-1)

    # ---- HIP-graph path -------------------------------------------------------------
    def _chunk_body(self, feats, drop: int):
        """The whole GPU part of a chunk on static state buffers (capturable: no host sync)."""
        m = self.model
        x = m.frontend(feats)
        lens = torch.full((self.B,), x.shape[0], dtype=torch.int32, device=self.dev)
        for i, layer in enumerate(m.rnn):
            x, _ = self._layer(layer, x, lens, self._h[i], out=self._h[i])   # state carried in place
        return self._head(self._lookahead_step(x), drop)

    def _graph_chunk(self, feats, drop: int = 0):
        if self._h is None:
            self._h = [torch.zeros(self.B, layer.hidden, device=self.dev, dtype=torch.float32)
                       for layer in self.model.rnn]
        # the frames a lookahead stream drops at its start change what the graph computes
        key = tuple(feats.shape) + (drop,)
        g = self._graphs.get(key)
        clone = lambda t: None if t is None else t.clone()   # noqa: E731
        if g is None:
            # first chunk of this shape: run it eagerly (real result, warms plans/handles),
            # then capture the same work into a graph for every later chunk of this shape
            lp, best = self._chunk_body(feats, drop)
            static_in = feats.clone()
            state = self._h + ([self._hist] if self._hist is not None else [])
            saved = [h.clone() for h in state]                # capture records, never runs
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._chunk_body(static_in, drop)
            for h, s in zip(state, saved):
                h.copy_(s)
            self._graphs[key] = (graph, static_in, out)
            return clone(lp), clone(best)
        graph, static_in, out = g
        static_in.copy_(feats)
        graph.replay()
        return clone(out[0]), clone(out[1])

    def _layer(self, layer, x, lens, h0, out=None):
        """One uni-directional layer from state h0 [B, H]; returns (y, h_last [B, H]), h_last
        written into `out` when given (it may be h0 itself: the kernel has read h0 by then)."""
        m = self.model
        if m.engine == "hip":
            from .ops import rnn as RNN
            y, h = RNN.recurrent_layer_infer(layer, x, lens, None if h0 is None else h0.unsqueeze(0),
                                             h_out=None if out is None else out.unsqueeze(0))
            return y, h[0]
        gx = layer.input_projection_ref(x, layer.fw, lens)
        bh = layer.fw.b_h.to(x.dtype) if layer.fw.b_h is not None else None
        y, h = R.recurrent_scan(layer.cell, gx, layer.fw.U.to(x.dtype), bh, lens, h0)
        if out is not None:
            out.copy_(h)
            h = out
        return y, h

    @torch.no_grad()
    def finish(self) -> List[List[int]]:
        """Final transcript label ids per stream (beam search over the whole stream if the
        decoder is 'beam', otherwise the incremental greedy result). With an LM the streams
        end here: the end-of-sentence term counts. A lookahead stream ends here too: the last tau
        output frames, which were waiting for recurrent outputs that will not come, are computed
        against tau zero frames (what the whole-utterance layer sees past the end) and go through
        the head and the decoder first, once; the stream then holds frames_out(total) log-prob
        rows, and accept() refuses more input until reset()."""
        self._flush_lookahead()
        final = self.lm is not None
        if self.gbeams is not None:
            return self.gbeams.best(final) if final else self.gbeams.best()
        if self.beams is None:
            return [list(g) for g in self.greedy]
        return self.beams.best(final) if final else self.beams.best()

    def _flush_lookahead(self) -> None:
        if self.tau == 0 or self._flushed:
            return
        self._flushed = True
        if self.done == 0:
            return
        t0 = time.perf_counter()
        H = self.model.num_hidden
        dtype = self._hist.dtype if self._hist is not None else torch.float32
        zeros = torch.zeros(self.tau, self.B, H, device=self.dev, dtype=dtype)
        # outputs of frames [done - tau, done); those below 0 (a stream shorter than tau) go
        lp, best_t = self._head(self._lookahead_step(zeros), max(0, self.tau - self.done))
        self._emit(lp, best_t)
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        self.compute_s += time.perf_counter() - t0

    @torch.no_grad()
    def finish_timed(self):
        """Words with times per stream: the final hypothesis of the configured decoder (as
        finish() returns it) force-aligned against the stream's stored log-probs
        (ops/align.py ctc_forced_align, on the device where they are; time convention in
        align.py). The alignment itself is kept in ``self.alignment``."""
        from .align import HOP_S, _pad_labels, tokens_to_words
        from .ops.align import ctc_forced_align
        hyp = self.finish()
        self.alignment = None
        if not self.logprobs:
            return [[] for _ in range(self.B)]
        lp = torch.cat(self.logprobs, 0)                        # [T2, B, K] log-probs
        lens = torch.full((self.B,), lp.shape[0], dtype=torch.int32, device=lp.device)
        labels, label_lens = _pad_labels(hyp)
        al = ctc_forced_align(lp, lens, labels.to(lp.device), label_lens.to(lp.device), BLANK, log_probs=True)
        self.alignment = al
        duration = HOP_S * self.total
        return [tokens_to_words(al, hyp, b, duration) for b in range(self.B)]


def rtf(model: DeepSpeech2, seconds: float = 10.0, chunk_s: float = 1.0, batch: int = 1,
        decoder: str = "greedy", beam_width: int = 16, seed: int = 0, audio: bool = False, lm=None,
        lm_weight: float = 1.0, label_bonus: float = 0.0, audio_rate: int = 16000):
    """Real-time factor of streaming synthetic audio: compute time / audio time (per stream;
    ``batch`` streams are processed together). Returns (rtf, transcripts). ``audio=True`` streams
    synthetic int16 PCM through accept_audio() (featurization included in the compute time)
    instead of ready-made feature frames, sampled at ``audio_rate`` (other than 16 kHz: resampled
    on the device, inside the compute time). ``lm``: a CharNgramLM fused into the beam decoder."""
    g = torch.Generator().manual_seed(seed)
    lmkw = {} if lm is None else dict(lm=lm, lm_weight=lm_weight, label_bonus=label_bonus)
    if audio:
        n = int(round(seconds * audio_rate))
        pcm = (torch.randn(batch, n, generator=g) * 3000.0).clamp_(-32768, 32767).to(torch.int16)
        rec = StreamingRecognizer(model, decoder=decoder, beam_width=beam_width, batch=batch,
                                  audio_rate=audio_rate, **lmkw)
        step = max(1, int(round(chunk_s * audio_rate)))
        for s in range(0, n, step):
            rec.accept_audio(pcm[:, s:s + step], final=s + step >= n)
        res = rec.finish()
        return rec.compute_s / seconds, res
    T = int(round(seconds * 100))
    feats = torch.randn(batch, T, model.freq_bins, generator=g)
    rec = StreamingRecognizer(model, decoder=decoder, beam_width=beam_width, batch=batch, **lmkw)
    step = max(1, int(round(chunk_s * 100)))
    for s in range(0, T, step):
        rec.accept(feats[:, s:s + step])
    res = rec.finish()
    return rec.compute_s / seconds, res
