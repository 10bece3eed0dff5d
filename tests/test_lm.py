"""Character n-gram LM (deepspeech_amd/lm.py): Witten-Bell training is normalised, the compiled
automaton equals direct backoff evaluation, ARPA files round-trip and hand-computed ARPA
probabilities (double backoff, <s> contexts, <unk>) come out of the table."""
import math

import numpy as np
import pytest

from deepspeech_amd.lm import BOS, CharNgramLM, synthetic_corpus

LN10 = math.log(10.0)


def _table_logp(lm, ids, eos=True):
    """ln P(ids [</s>]) by walking the compiled automaton."""
    logp, nxt, s = lm.compile()
    tot = 0.0
    for k in ids:
        tot += float(logp[s, k])
        s = int(nxt[s, k])
        assert s >= 0
    return tot + (float(logp[s, lm.blank]) if eos else 0.0)


@pytest.fixture(scope="module")
def corpus():
    return synthetic_corpus(sentences=120, seed=5)        # ~500 words


@pytest.mark.parametrize("order", [1, 3, 6])
def test_trained_model_is_normalised_and_table_equals_backoff(corpus, order):
    lm = CharNgramLM.train(corpus, order)
    logp, nxt, start = lm.compile()
    S, K = logp.shape
    assert K == 29 and nxt.shape == (S, K) and logp.dtype == np.float32 and nxt.dtype == np.int32
    assert (S == 1) == (order == 1) and 0 <= start < S
    assert np.isfinite(logp).all()
    # labels + </s> (column blank) sum to 1 in every state
    lse = np.log(np.exp(logp.astype(np.float64)).sum(1))
    assert np.abs(lse).max() < 1e-5, np.abs(lse).max()
    assert (nxt[:, lm.blank] == -1).all()
    lab = np.delete(nxt, lm.blank, axis=1)
    assert lab.min() >= 0 and lab.max() < S
    # held-out strings (unseen words, so the backoff chains are exercised)
    for text in synthetic_corpus(sentences=4, seed=99) + ["ZZQ' XJ", ""]:
        ids = lm.encode(text)
        for eos in (True, False):
            assert abs(_table_logp(lm, ids, eos) - lm.score(text, eos)) < 2e-5, (text, eos)


def test_label_id_lists_and_blank_zero():
    """Label-id transcripts with blank = 0: classes 1..K-1 are the labels, column 0 is </s>."""
    rng = np.random.default_rng(2)
    data = [rng.integers(1, 5, size=int(rng.integers(1, 9))).tolist() for _ in range(50)]
    lm = CharNgramLM.train(data, 3, alphabet="ABCD", blank=0)
    logp, nxt, _ = lm.compile()
    assert logp.shape[1] == 5 and (nxt[:, 0] == -1).all() and nxt[:, 1:].min() >= 0
    assert np.abs(np.log(np.exp(logp.astype(np.float64)).sum(1))).max() < 1e-5
    assert abs(_table_logp(lm, [1, 4, 4, 2]) - lm.score([1, 4, 4, 2])) < 2e-5
    with pytest.raises(ValueError):
        lm.encode([0, 1])


def test_arpa_round_trip_and_npz(corpus, tmp_path):
    lm = CharNgramLM.train(corpus, 4)
    path = str(tmp_path / "lm.arpa")
    lm.to_arpa(path)
    text = open(path).read()
    assert text.startswith("\\data\\\nngram 1=") and "<space>" in text and "\\4-grams:" in text
    back = CharNgramLM.from_arpa(path)
    a, b = lm.compile(), back.compile()
    assert back.order == 4 and a[2] == b[2]
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-6)
    npz = str(tmp_path / "lm.npz")
    lm.save(npz)
    c = CharNgramLM.read(npz)
    np.testing.assert_array_equal(a[0], c.compile()[0])
    np.testing.assert_array_equal(a[1], c.compile()[1])
    np.testing.assert_array_equal(lm.fold(0.8, 0.5), c.fold(0.8, 0.5))
    w = lm.fold(0.8, 0.5).astype(np.float64)
    want = 0.8 * a[0].astype(np.float64) + 0.5
    want[:, lm.blank] -= 0.5
    np.testing.assert_allclose(w, want, rtol=1e-6)


TINY = """\\data\\
ngram 1=5
ngram 2=3
ngram 3=1

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.3\tA\t-0.2
-0.6\tB\t-0.4
-0.9\t%(sp)s\t-0.1

\\2-grams:
-0.25\t<s> A\t-0.3
-0.45\tA B\t-0.15
-0.7\tB %(sp)s

\\3-grams:
-0.05\t<s> A B

\\end\\
"""


@pytest.mark.parametrize("space", ["<space>", "|"])
def test_hand_written_arpa(tmp_path, space):
    path = str(tmp_path / "tiny.arpa")
    with open(path, "w") as f:
        f.write(TINY % {"sp": space})
    lm = CharNgramLM.from_arpa(path, alphabet="AB ")      # classes A=0, B=1, ' '=2, blank / </s> = 3
    assert lm.order == 3 and lm.K == 4 and lm.blank == 3
    A, B, SP, EOS = 0, 1, 2, 3
    logp, nxt, start = lm.compile()

    def walk(ctx):
        s = start
        for k in ctx:
            s = int(nxt[s, k])
        return s

    # (context after <s>, class, log10 P worked out by hand)
    cases = [
        ([], A, -0.25),                                   # bigram "<s> A"
        ([], B, -0.5 - 0.6),                              # <s> context backs off: bow(<s>) + P(B)
        ([A], B, -0.05),                                  # trigram "<s> A B"
        ([A], A, -0.3 - 0.2 - 0.3),                       # double: bow(<s> A) + bow(A) + P(A)
        ([A, B], A, -0.15 - 0.4 - 0.3),                   # double: bow(A B) + bow(B) + P(A)
        ([A, B], SP, -0.15 - 0.7),                        # bow(A B) + bigram "B <space>"
        ([A, B, SP], EOS, 0.0 - 0.1 - 1.0),               # "B <space>" has no bow: 0 + bow(<space>) + P(</s>)
        ([B, B], B, -0.4 - 0.6),                          # context "B B" is no state: falls to "B"
    ]
    for ctx, k, log10p in cases:
        assert abs(float(logp[walk(ctx), k]) - log10p * LN10) < 1e-6, (ctx, k)
        assert abs(lm.cond_logp(k, [BOS] + ctx) - log10p * LN10) < 1e-12, (ctx, k)


def test_missing_label_needs_unk(tmp_path):
    lines = [l for l in (TINY % {"sp": "<space>"}).splitlines() if not l.startswith("-0.6\tB")]
    path = str(tmp_path / "nob.arpa")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match="unk"):
        CharNgramLM.from_arpa(path, alphabet="AB ")
    with open(path, "w") as f:
        f.write("\n".join(lines).replace("-1.0\t</s>", "-1.0\t</s>\n-2.0\t<unk>") + "\n")
    lm = CharNgramLM.from_arpa(path, alphabet="AB ")
    logp, _, start = lm.compile()
    assert abs(float(logp[start, 1]) - (-0.5 - 2.0) * LN10) < 1e-6       # bow(<s>) + P(<unk>)


def test_eval_flags_and_word_error_rate():
    from deepspeech_amd import config as C
    from deepspeech_amd.test import word_errors
    a = C.build_eval_parser().parse_args([])
    assert (a.lm_path, a.lm_weight, a.label_bonus, a.report_wer) == ("", 1.0, 0.0, False)
    a = C.build_eval_parser().parse_args(["--lm_path", "x.arpa", "--lm_weight", "0.7", "--label_bonus", "1.5",
                                          "--report_wer", "True"])
    assert (a.lm_path, a.lm_weight, a.label_bonus, a.report_wer) == ("x.arpa", 0.7, 1.5, True)
    assert word_errors("THE CAT SAT", "THE CAT SAT") == (0, 3)
    assert word_errors("THE CAT SAT", "THE BAT SAT DOWN") == (2, 3)     # one substitution, one insertion
    assert word_errors("A B", "") == (2, 2)


def test_lm_cli_writes_arpa_and_npz(tmp_path):
    from deepspeech_amd import lm as LM
    txt = tmp_path / "corpus.txt"
    txt.write_text("\n".join(synthetic_corpus(30, seed=8)) + "\n")
    arpa, npz = str(tmp_path / "lm.arpa"), str(tmp_path / "lm.npz")
    assert LM.main(["--text", str(txt), "--order", "3", "--out", arpa, "--npz", npz]) == 0
    a, b = CharNgramLM.read(arpa).compile(), CharNgramLM.read(npz).compile()
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-6)
