"""Character n-gram language model for shallow fusion in the CTC prefix beam searches
(csrc/beam.hip on the GPU, runtime/decoder.cpp on the host).

  python -m deepspeech_amd.lm --text corpus.txt --order 5 --out lm.arpa [--npz lm.npz]
  python -m deepspeech_amd.lm --data_dir ../data/LibriSpeech/processed/ --partition train \
      --order 5 --out lm.arpa

A prefix l_1..l_n is ranked by  log P_ctc + alpha * sum_i ln P(l_i | l_1..l_{i-1}) + beta * n
(DeepSpeech2's decoding objective with a character LM). The decoders never walk backoff
chains: :meth:`CharNgramLM.compile` expands the model into an automaton

  logp [S, K] fp32   ln P(k | state), backoff fully resolved in fp64 on the host
  nxt  [S, K] int32  state after appending label k (longest suffix of state + k that is a state)

whose states are the distinct contexts of length <= order - 1 (with the empty context and the
``<s>`` contexts). Column ``blank`` holds ln P(</s> | state) and nxt -1: K indexes labels and
the end of sentence alike, so a lookup is one row read whatever the order. :meth:`fold` bakes
the LM weight and the per-label bonus into the table (``alpha * logp + beta``), so a decoder
adds one fp32 number per extension.

Training is interpolated Witten-Bell in numpy (no external toolkit); ARPA files (one character
per token, space written ``<space>``) are read and written, so a character LM built elsewhere
can be used.
"""
from __future__ import annotations

import argparse
import math
import sys
from collections import defaultdict
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import ALPHABET

BOS = -1            # token id of <s> inside n-gram tuples (labels are their class ids, </s> is `blank`)
_LN10 = math.log(10.0)


class CharNgramLM:
    """Backoff n-gram over the K - 1 labels of a CTC alphabet plus ``</s>``.

    ``logp[ngram]`` is ln P(ngram[-1] | ngram[:-1]) and ``bow[context]`` the ln backoff weight,
    n-grams being tuples of class ids (``BOS`` for ``<s>``, ``blank`` for ``</s>``). A model
    restored by :meth:`load` holds only the compiled automaton."""

    def __init__(self, order: int, alphabet: str = ALPHABET, blank: Optional[int] = None,
                 logp: Optional[Dict[tuple, float]] = None, bow: Optional[Dict[tuple, float]] = None):
        self.order = int(order)
        self.alphabet = alphabet
        self.K = len(alphabet) + 1
        self.blank = self.K - 1 if blank is None else int(blank)
        if self.order < 1 or not 0 <= self.blank < self.K:
            raise ValueError("CharNgramLM: order >= 1 and 0 <= blank < K")
        self.logp = logp
        self.bow = bow if bow is not None else {}
        self._compiled = None

    # ---- alphabet <-> class ids ------------------------------------------------------
    def _ids(self) -> List[int]:
        return [k for k in range(self.K) if k != self.blank]

    def _char_to_id(self) -> Dict[str, int]:
        return {c: k for c, k in zip(self.alphabet, self._ids())}

    def encode(self, text) -> List[int]:
        """A transcript (str: characters outside the alphabet are dropped; or label ids)."""
        if isinstance(text, str):
            m = self._char_to_id()
            out = []
            for c in text:
                k = m.get(c, m.get(c.upper()))
                if k is not None:
                    out.append(k)
            return out
        ids = [int(k) for k in text]
        for k in ids:
            if not 0 <= k < self.K or k == self.blank:
                raise ValueError("CharNgramLM: label id %d outside the alphabet" % k)
        return ids

    # ---- training --------------------------------------------------------------------
    @classmethod
    def train(cls, transcripts: Iterable, order: int, alphabet: str = ALPHABET,
              blank: Optional[int] = None) -> "CharNgramLM":
        """Interpolated Witten-Bell: P(w | h) = (c(hw) + N1+(h.) P(w | h')) / (c(h) + N1+(h.)),
        the unigram interpolated with the uniform distribution over the labels and </s>, so every
        label is finite and every context sums to 1."""
        lm = cls(order, alphabet, blank)
        counts: List[Dict[tuple, Dict[int, float]]] = [defaultdict(lambda: defaultdict(float))
                                                        for _ in range(order)]
        for tr in transcripts:
            s = [BOS] + lm.encode(tr) + [lm.blank]
            for i in range(1, len(s)):
                for m in range(min(order, i + 1)):
                    counts[m][tuple(s[i - m:i])][s[i]] += 1.0
        V = lm.K                                 # K - 1 labels + </s>
        vocab = lm._ids() + [lm.blank]
        uni = counts[0].get((), {})
        c0, n0 = sum(uni.values()), max(1, len(uni))
        prob: Dict[tuple, float] = {}
        for w in vocab:
            prob[(w,)] = (uni.get(w, 0.0) + n0 / V) / (c0 + n0)
        bow: Dict[tuple, float] = {}
        for m in range(1, order):
            for h, foll in counts[m].items():
                c, n1 = sum(foll.values()), len(foll)
                bow[h] = math.log(n1 / (c + n1))
                for w, cw in foll.items():
                    prob[h + (w,)] = (cw + n1 * lm._prob_lower(prob, bow, h[1:], w)) / (c + n1)
        lm.logp = {ng: math.log(p) for ng, p in prob.items()}
        lm.bow = bow
        return lm

    @staticmethod
    def _prob_lower(prob, bow, h, w) -> float:
        p = prob.get(h + (w,))
        if p is not None:
            return p
        return math.exp(bow.get(h, 0.0)) * CharNgramLM._prob_lower(prob, bow, h[1:], w)

    # ---- evaluation ------------------------------------------------------------------
    def _need_ngrams(self):
        if self.logp is None:
            raise ValueError("CharNgramLM: this model holds only the compiled automaton")

    def cond_logp(self, w: int, context: Sequence[int]) -> float:
        """ln P(w | context) by the textbook backoff recursion, in fp64 (w = blank: </s>)."""
        self._need_ngrams()
        h = tuple(context)[-(self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        while True:
            p = self.logp.get(h + (w,))
            if p is not None:
                return acc + p
            if not h:
                raise KeyError("CharNgramLM: no unigram for class %d" % w)
            acc += self.bow.get(h, 0.0)
            h = h[1:]

    def score(self, text, eos: bool = True) -> float:
        """ln P(transcript [</s>] | <s>) by direct backoff evaluation."""
        ids = self.encode(text)
        hist, tot = [BOS], 0.0
        for k in ids + ([self.blank] if eos else []):
            tot += self.cond_logp(k, hist)
            hist.append(k)
        return tot

    # ---- automaton -------------------------------------------------------------------
    def compile(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """(logp float32 [S, K], nxt int32 [S, K], start)."""
        if self._compiled is not None:
            return self._compiled
        self._need_ngrams()
        n, K = self.order, self.K
        states = {()}
        if n > 1:
            states.add((BOS,))
            for ng in self.logp:
                if len(ng) >= 2:
                    states.add(ng[:-1][-(n - 1):])
            for h in self.bow:
                if 1 <= len(h) <= n - 1:
                    states.add(h)
        # a context reached only through </s> is never a decoder state
        states = sorted((s for s in states if self.blank not in s), key=lambda s: (len(s), s))
        S = len(states)
        if S * K >= 2 ** 31:
            raise ValueError("CharNgramLM.compile: S * K = %d * %d does not fit int32" % (S, K))
        index = {s: i for i, s in enumerate(states)}
        logp = np.empty((S, K), np.float64)
        nxt = np.full((S, K), -1, np.int32)
        for i, s in enumerate(states):
            for k in range(K):
                logp[i, k] = self.cond_logp(k, s)
                if k == self.blank:
                    continue
                h = (s + (k,))[-(n - 1):] if n > 1 else ()
                while h not in index:
                    h = h[1:]
                nxt[i, k] = index[h]
        start = index[(BOS,)] if n > 1 else 0
        self._compiled = (logp.astype(np.float32), nxt, int(start))
        return self._compiled

    def fold(self, alpha: float = 1.0, beta: float = 0.0) -> np.ndarray:
        """The fp32 table the decoders add: alpha * logp + beta per label, alpha * logp for </s>."""
        logp = self.compile()[0].astype(np.float64)
        w = alpha * logp + beta
        w[:, self.blank] = alpha * logp[:, self.blank]
        return w.astype(np.float32)

    # ---- persistence -----------------------------------------------------------------
    def save(self, path: str) -> None:
        logp, nxt, start = self.compile()
        with open(path, "wb") as f:
            np.savez(f, logp=logp, nxt=nxt, start=np.int64(start), order=np.int64(self.order),
                     blank=np.int64(self.blank), alphabet=np.array(self.alphabet))

    @classmethod
    def load(cls, path: str) -> "CharNgramLM":
        with np.load(path) as z:
            lm = cls(int(z["order"]), str(z["alphabet"]), int(z["blank"]))
            logp, nxt, start = z["logp"].astype(np.float32), z["nxt"].astype(np.int32), int(z["start"])
        S = logp.shape[0]
        lab = np.delete(nxt, lm.blank, axis=1)
        if logp.shape != (S, lm.K) or nxt.shape != logp.shape or not 0 <= start < S or lab.min() < 0 \
                or lab.max() >= S:
            raise ValueError("CharNgramLM.load: %s is not a compiled LM of this alphabet" % path)
        lm._compiled = (logp, nxt, start)
        return lm

    @classmethod
    def read(cls, path: str, alphabet: str = ALPHABET, blank: Optional[int] = None) -> "CharNgramLM":
        """An ARPA text file or a compiled .npz, by extension."""
        if path.endswith(".npz"):
            return cls.load(path)
        return cls.from_arpa(path, alphabet, blank)

    # ---- ARPA ------------------------------------------------------------------------
    def _token(self, k: int) -> str:
        if k == BOS:
            return "<s>"
        if k == self.blank:
            return "</s>"
        c = self.alphabet[self._ids().index(k)]
        return "<space>" if c == " " else c

    def to_arpa(self, path: str) -> None:
        self._need_ngrams()
        by_len: List[List[tuple]] = [[] for _ in range(self.order)]
        for ng in self.logp:
            by_len[len(ng) - 1].append(ng)
        by_len[0].append((BOS,))
        with open(path, "w") as f:
            f.write("\\data\\\n")
            for m, ngs in enumerate(by_len):
                f.write("ngram %d=%d\n" % (m + 1, len(ngs)))
            for m, ngs in enumerate(by_len):
                f.write("\n\\%d-grams:\n" % (m + 1))
                for ng in sorted(ngs):
                    lp = -99.0 if ng == (BOS,) else self.logp[ng] / _LN10
                    line = "%.17g\t%s" % (lp, " ".join(self._token(k) for k in ng))
                    if m + 1 < self.order and ng in self.bow:
                        line += "\t%.17g" % (self.bow[ng] / _LN10)
                    f.write(line + "\n")
            f.write("\n\\end\\\n")

    @classmethod
    def from_arpa(cls, path: str, alphabet: str = ALPHABET, blank: Optional[int] = None) -> "CharNgramLM":
        """Standard ARPA (log10 probabilities, backoff weights), one character per token; the
        space is ``<space>`` or ``|``. N-grams with a token outside the alphabet are ignored; a
        label without a unigram takes ``<unk>``'s, and it is an error if there is none."""
        probe = cls(1, alphabet, blank)
        tok = dict(probe._char_to_id())
        for c, k in list(tok.items()):
            tok.setdefault(c.lower(), k)
        if " " in tok:
            tok["<space>"] = tok["|"] = tok[" "]
        tok["<s>"], tok["</s>"] = BOS, probe.blank
        logp: Dict[tuple, float] = {}
        bow: Dict[tuple, float] = {}
        unk = None
        order, cur = 0, 0
        with open(path, "r") as f:
            for raw in f:
                line = raw.strip()
                if not line or line == "\\data\\" or line.startswith("ngram "):
                    continue
                if line == "\\end\\":
                    break
                if line.startswith("\\") and line.endswith("-grams:"):
                    cur = int(line[1:-len("-grams:")])
                    order = max(order, cur)
                    continue
                if cur == 0:
                    continue
                parts = line.split()
                if len(parts) not in (cur + 1, cur + 2):
                    raise ValueError("from_arpa: bad %d-gram line %r" % (cur, line))
                words = parts[1:1 + cur]
                if cur == 1 and words[0] == "<unk>":
                    unk = float(parts[0]) * _LN10
                    continue
                if any(w not in tok for w in words):
                    continue
                ng = tuple(tok[w] for w in words)
                if ng[-1] != BOS:
                    logp[ng] = float(parts[0]) * _LN10
                if len(parts) == cur + 2:
                    bow[ng] = float(parts[-1]) * _LN10
        if order < 1:
            raise ValueError("from_arpa: no n-gram section in %s" % path)
        lm = cls(order, alphabet, blank, logp, bow)
        for k in range(lm.K):
            if (k,) not in logp:
                if unk is None:
                    raise ValueError("from_arpa: no unigram for %r and no <unk> in %s" % (lm._token(k), path))
                logp[(k,)] = unk
        return lm


def synthetic_corpus(sentences: int = 200, seed: int = 0, vocab: int = 60, alphabet: str = ALPHABET) -> List[str]:
    """Seeded pseudo-text: sentences of 2..7 words drawn (Zipf-like) from a random vocabulary of
    1..8-letter words. For tests and tools/bench_infer.py, where no corpus is at hand."""
    rng = np.random.default_rng(seed)
    letters = [c for c in alphabet if c != " "]
    words = ["".join(rng.choice(letters, size=int(rng.integers(1, 9)))) for _ in range(vocab)]
    pw = 1.0 / np.arange(1, vocab + 1)
    pw /= pw.sum()
    return [" ".join(words[i] for i in rng.choice(vocab, size=int(rng.integers(2, 8)), p=pw))
            for _ in range(sentences)]


def labels_of_store(data_dir: str, partition: str) -> Iterable[List[int]]:
    """Label-id lists of a preprocessed store partition (data/store.py)."""
    from .data.store import StoreIndex, find_store
    prefix = find_store(data_dir, partition)
    if prefix is None:
        raise ValueError("no %s store under %s" % (partition, data_dir))
    idx = StoreIndex.load(prefix)
    for o, n in zip(idx.label_offsets, idx.label_lens):
        yield idx.labels[int(o):int(o) + int(n)].tolist()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="train a character n-gram LM (interpolated Witten-Bell)")
    ap.add_argument("--text", help="text file, one transcript per line")
    ap.add_argument("--data_dir", help="preprocessed store: train on its labels")
    ap.add_argument("--partition", default="train")
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--out", required=True, help="ARPA file to write")
    ap.add_argument("--npz", help="also write the compiled automaton")
    a = ap.parse_args(argv)
    if (a.text is None) == (a.data_dir is None):
        ap.error("give exactly one of --text and --data_dir")
    if a.text is not None:
        with open(a.text, "r") as f:
            src = [line.rstrip("\n") for line in f if line.strip()]
    else:
        src = labels_of_store(a.data_dir, a.partition)
    lm = CharNgramLM.train(src, a.order)
    lm.to_arpa(a.out)
    logp, _, _ = lm.compile()
    if a.npz:
        lm.save(a.npz)
    print("order %d, %d n-grams, %d states -> %s" % (a.order, len(lm.logp), logp.shape[0], a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
