"""Shallow LM fusion in the native host prefix beam search (runtime/decoder.cpp): a prefix
l_1..l_n is ranked by log P_ctc + alpha * ln P_lm(l_1..l_n) + beta * n, checked against a
brute-force maximum over all K^T paths; the LM moves a coin-flip the intended way; no LM is
the search as it was; chunked, threaded and batched decoding agree with one stream."""
import itertools

import numpy as np
import pytest

from deepspeech_amd.lm import CharNgramLM, synthetic_corpus
from deepspeech_amd.ops.decode import host_lm
from deepspeech_amd.runtime import native

N = native.load()
ALPHA, BETA = 0.8, 0.5


def _brute_force(lp, blank, lm, alpha, beta, final):
    """max over collapsed prefixes of (log-sum of its paths) + alpha * ln P_lm + beta * n, fp64."""
    T, K = lp.shape
    logp, nxt, start = lm.compile()
    logp = logp.astype(np.float64)
    scores = {}
    for path in itertools.product(range(K), repeat=T):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        p = sum(lp[t, c] for t, c in enumerate(path))
        key = tuple(out)
        scores[key] = np.logaddexp(scores.get(key, -np.inf), p)
    best = None
    for key, ac in scores.items():
        s, tot = start, ac + beta * len(key)
        for k in key:
            tot += alpha * logp[s, k]
            s = int(nxt[s, k])
        if final:
            tot += alpha * logp[s, blank]
        if best is None or tot > best[1]:
            best = (key, tot)
    return best


@pytest.mark.parametrize("blank", [2, 0])
def test_lm_beam_search_exact_for_wide_beam(blank):
    rng = np.random.default_rng(3 + blank)
    labels = [k for k in range(3) if k != blank]
    data = [[labels[i] for i in rng.integers(0, 2, size=int(rng.integers(1, 6)))] for _ in range(12)]
    lm = CharNgramLM.train(data, 2, alphabet="AB", blank=blank)
    L = host_lm(lm, ALPHA, BETA, blank)
    assert (L.S, L.K, L.blank) == (lm.compile()[0].shape[0], 3, blank)
    for _ in range(3):
        lp = np.log(rng.dirichlet(np.ones(3), size=5)).astype(np.float32)
        bs = N.PrefixBeamSearch(256, blank, -1e9, L)
        bs.feed(lp)
        for final in (False, True):
            ref, rscore = _brute_force(lp.astype(np.float64), blank, lm, ALPHA, BETA, final)
            best, score = bs.results(final)[0]
            assert tuple(best) == ref and abs(score - rscore) < 1e-4, (final, best, score, ref, rscore)
            assert bs.best(final) == list(ref)
            sc = [s for _, s in bs.results(final)]
            assert sc == sorted(sc, reverse=True)


def test_lm_decides_a_coin_flip():
    """Frames: C, blank, then A (0.52) against B (0.48). Acoustically the answer is CA; an LM
    that has only ever seen CB turns it into CB."""
    K, blank = 29, 28
    A, B, C = 0, 1, 2
    p = np.full((3, K), 1e-4)
    p[0, C] = 1.0
    p[1, blank] = 1.0
    p[2, A], p[2, B] = 0.52, 0.48
    lp = np.log(p / p.sum(1, keepdims=True)).astype(np.float32)
    plain = N.PrefixBeamSearch(8, blank, -10.0)
    plain.feed(lp)
    assert plain.best() == [C, A]
    lm = CharNgramLM.train(["CB"] * 20, 2)
    for final in (False, True):
        fused = N.PrefixBeamSearch(8, blank, -10.0, lm=host_lm(lm, 1.0, 0.0, blank))
        fused.feed(lp)
        assert fused.best(final) == [C, B]


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(11)
    T, B, K = 40, 6, 29
    lp = np.log(rng.dirichlet(np.ones(K) * 0.3, size=(T, B))).astype(np.float32)   # [T, B, K]
    lens = np.array([40, 33, 17, 40, 1, 25], np.int32)
    return lp, lens


def test_no_lm_is_the_existing_search(batch):
    lp, lens = batch
    for b in range(lp.shape[1]):
        x = np.ascontiguousarray(lp[: lens[b], b])
        old = N.PrefixBeamSearch(8, 28, -8.0)
        old.feed(x)
        new = N.PrefixBeamSearch(8, 28, -8.0, lm=None)
        new.feed(x)
        assert new.results() == old.results() == new.results(final=True)
        assert new.best(final=True) == old.best()
    assert N.beam_search_batch(lp, lens, 8, 28, -8.0, 2, lm=None, final=True) == \
        N.beam_search_batch(lp, lens, 8, 28, -8.0, 2)


def test_lm_batch_threads_and_streaming_match_single(batch):
    lp, lens = batch
    T, B, _ = lp.shape
    lm = CharNgramLM.train(synthetic_corpus(80, seed=1), 3)
    L = host_lm(lm, ALPHA, BETA, 28)
    single, single_final, plain = [], [], []
    for b in range(B):
        x = np.ascontiguousarray(lp[: lens[b], b])
        bs = N.PrefixBeamSearch(8, 28, -8.0, L)
        bs.feed(x)
        single.append(bs.best())
        single_final.append(bs.best(final=True))
        whole = bs.results(final=True)
        bs.reset()
        for s in range(0, len(x), 7):                       # chunked feeding after a reset
            bs.feed(x[s:s + 7])
        assert bs.results(final=True) == whole
        pl = N.PrefixBeamSearch(8, 28, -8.0)
        pl.feed(x)
        plain.append(pl.best())
    assert single != plain                                   # the LM is not a no-op here
    for threads in (1, 4):
        assert N.beam_search_batch(lp, lens, 8, 28, -8.0, threads, lm=L, final=True) == single_final
        assert N.beam_search_batch(lp, lens, 8, 28, -8.0, threads, lm=L) == single
    bb = N.BatchBeamSearch(B, 8, 28, -8.0, 3, lm=L)
    for s in range(0, T, 15):
        chunk = np.ascontiguousarray(lp[s:s + 15])
        bb.feed(chunk, np.clip(lens - s, 0, chunk.shape[0]).astype(np.int32))
    assert bb.best() == single and bb.best(final=True) == single_final


def test_lm_must_match_the_decoder(batch):
    lp, _ = batch
    lm = CharNgramLM.train(["AB"], 2, alphabet="AB")         # K = 3
    with pytest.raises(ValueError):
        host_lm(lm, 1.0, 0.0, 28)
    L = host_lm(lm, 1.0, 0.0, 2)
    with pytest.raises(RuntimeError):
        N.PrefixBeamSearch(8, 28, -8.0, L)                   # folded for blank 2
    bs = N.PrefixBeamSearch(8, 2, -8.0, L)
    with pytest.raises(RuntimeError):
        bs.feed(np.ascontiguousarray(lp[:4, 0]))             # 29 classes against the LM's 3
    bad = np.zeros((2, 3), np.int32)
    bad[1, 0] = 2                                            # next state 2 of S = 2
    with pytest.raises(RuntimeError):
        N.BeamLM(np.zeros((2, 3), np.float32), bad, 0, 2)
