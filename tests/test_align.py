"""CTC forced alignment on the CPU: the oracle (ops/reference.py ctc_viterbi_ref) against a brute
force over every frame path, the fixed tie rule, infeasible / empty lattices, the greedy
invariant, the frame -> seconds convention and words, StreamingRecognizer.finish_timed() on the
reference engine, and the register budget of csrc/align.hip."""
import itertools
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from align_cases import collapse, pad_labels, path_score, quantised_lp, random_lp

from deepspeech_amd import ALPHABET, BLANK
from deepspeech_amd.ops import reference as R
from deepspeech_amd.ops.align import Alignment, ctc_forced_align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _align(lp, lens, rows, blank):
    lab, ll = pad_labels(rows)
    return Alignment(*R.ctc_viterbi_ref(lp, torch.tensor(lens, dtype=torch.int32), lab, ll, blank))


# ---------------------------------------------------------------- oracle against brute force
@pytest.mark.parametrize("labels", [[], [0], [1], [0, 1], [1, 0], [0, 0], [1, 1]])
def test_oracle_matches_brute_force(labels):
    K, blank = 3, 2
    for T in range(1, 7):
        lp = random_lp(T, 1, K, seed=10 * T + len(labels), sharp=1.5)
        a = _align(lp, [T], [labels], blank)
        lpn = lp[:, 0].numpy()
        best = None
        for p in itertools.product(range(K), repeat=T):
            if collapse(p, blank) == labels:
                s = path_score(lpn, p)
                best = s if best is None or s > best else best
        if best is None:
            assert a.score[0] == -math.inf and (a.path[0] == -1).all() and (a.tok_start[0] == -1).all()
            continue
        assert np.float32(a.score[0].item()) == best, (T, labels)
        got = a.path[0].tolist()
        assert collapse(got, blank) == labels
        assert path_score(lpn, got) == best
        for l, c in enumerate(labels):          # spans cover exactly the label's frames on the path
            s, e = int(a.tok_start[0, l]), int(a.tok_end[0, l])
            assert 0 <= s <= e < T and got[s:e + 1] == [c] * (e - s + 1)
            assert (s == 0 or got[s - 1] != c) and (e == T - 1 or got[e + 1] != c)
            np.testing.assert_allclose(a.tok_score[0, l].item(), lpn[s:e + 1, c].sum(), rtol=1e-6)


# ---------------------------------------------------------------- tie rule
def test_tie_rule_hand_written():
    """Every frame scores -0.5 whatever the class, so all paths of 'AB' through 5 frames tie at
    -2.5. Stay-before-advance in the forward pass records, for each state, the EARLIEST frame at
    which it can be reached (later equal arrivals lose to staying), and the final tie goes to
    the trailing blank: the backtrack therefore emits A at frame 0, B at frame 1 (reached from A
    by the s-2 skip, the only finite predecessor then), and blank for the rest."""
    K, blank = 3, 2
    lp = torch.full((5, 1, K), -0.5)
    a = _align(lp, [5], [[0, 1]], blank)
    assert a.path[0].tolist() == [0, 1, 2, 2, 2]
    assert a.tok_start[0].tolist() == [0, 1] and a.tok_end[0].tolist() == [0, 1]
    assert a.score[0].item() == -2.5
    assert a.tok_score[0].tolist() == [-0.5, -0.5]
    # a repeated label needs the blank between: A at 0, blank at 1, A at 2, trailing blanks
    a = _align(lp, [5], [[0, 0]], blank)
    assert a.path[0].tolist() == [0, 2, 0, 2, 2]
    # final tie: state 2L (trailing blank) is preferred, 2L-1 only when strictly better
    lp2 = lp.clone()
    lp2[4, 0, 1] = -0.25
    a = _align(lp2, [5], [[0, 1]], blank)
    assert a.path[0].tolist() == [0, 1, 1, 1, 1] and a.score[0].item() == -2.25


def test_quantised_ties_are_deterministic_and_optimal():
    K, blank = 3, 2
    lp = quantised_lp(6, 1, K, seed=3)
    a = _align(lp, [6], [[0, 1]], blank)
    lpn = lp[:, 0].numpy()
    scores = [path_score(lpn, p) for p in itertools.product(range(K), repeat=6) if collapse(p, blank) == [0, 1]]
    assert a.score[0].item() == max(scores)
    assert path_score(lpn, a.path[0].tolist()) == max(scores)


# ---------------------------------------------------------------- infeasible / empty
def test_infeasible_and_empty():
    K, blank, T = 5, 4, 6
    lp = random_lp(T, 6, K, seed=1)
    rows = [[0, 1, 2], [0, 0, 1], [], [1, 2], [0, 1, 2, 3, 0, 1, 2], [3]]
    lens = [6, 3, 4, 0, 6, -2]
    a = _align(lp, lens, rows, blank)
    # row 1: 3 labels + 1 adjacent repeat need 4 frames, 3 given; row 3 / 5: no frames; row 4: 7 labels, 6 frames
    for b in (1, 3, 4, 5):
        assert a.score[b] == -math.inf
        assert (a.path[b] == -1).all() and (a.tok_start[b] == -1).all() and (a.tok_end[b] == -1).all()
    assert math.isfinite(a.score[0]) and collapse(a.path[0].tolist(), blank) == rows[0]
    # L = 0: the all-blank path over the valid frames, -1 after them, no spans
    assert a.path[2].tolist() == [blank] * 4 + [-1, -1]
    assert a.score[2].item() == path_score(lp[:, 2].numpy(), [blank] * 4)
    assert (a.tok_start[2] == -1).all()
    # entries at or past label_lens
    assert a.tok_start[0, 3:].tolist() == [-1] * 4 and a.tok_end[0, 3:].tolist() == [-1] * 4
    # exactly enough frames for a repeat: feasible
    ok = _align(lp, [4] + [0] * 5, [[0, 0, 1]] + [[]] * 5, blank)
    assert ok.path[0].tolist() == [0, blank, 0, 1, -1, -1]


def test_nan_frame_gives_nan_score():
    lp = random_lp(8, 2, 5, seed=2)
    lp[3, 1, 2] = float("nan")
    a = _align(lp, [8, 8], [[0, 1], [0, 1]], 4)
    assert math.isfinite(a.score[0]) and math.isnan(a.score[1])
    lp[3, 1, 2] = 0.0
    lp[7, 1, 0] = float("nan")                     # past the valid length: ignored
    assert math.isfinite(_align(lp, [8, 7], [[0, 1], [0, 1]], 4).score[1])


def test_limits_raise_value_error():
    lens = torch.tensor([4], dtype=torch.int32)
    with pytest.raises(ValueError, match="32"):
        ctc_forced_align(torch.zeros(4, 1, 33), lens, torch.zeros(1, 2, dtype=torch.int32), lens, blank=32)
    with pytest.raises(ValueError, match="2048"):
        ctc_forced_align(torch.zeros(4, 1, 5), lens, torch.zeros(1, 1024, dtype=torch.int32), lens, blank=4)


# ---------------------------------------------------------------- greedy invariant
def test_greedy_hypothesis_aligns_to_the_argmax_path():
    T, N, K, blank = 40, 4, 29, 28
    lp = random_lp(T, N, K, seed=5, sharp=3.0)
    top2 = lp.topk(2, -1).values
    assert (top2[..., 0] > top2[..., 1]).all()     # no frame-wise argmax ties
    lens = torch.tensor([40, 33, 1, 17], dtype=torch.int32)
    hyp = R.greedy_decode(lp, lens, blank)
    lab, ll = pad_labels(hyp)
    a = ctc_forced_align(lp, lens, lab, ll, blank, log_probs=True)      # CPU tensors: the oracle
    best = lp.argmax(-1)
    for b in range(N):
        n = int(lens[b])
        assert a.path[b, :n].tolist() == best[:n, b].tolist()
        assert (a.path[b, n:] == -1).all()
        assert a.score[b].item() == path_score(lp[:, b].numpy(), best[:n, b].tolist())
    # logits input on the CPU: log-softmax first
    a2 = ctc_forced_align(3.0 * lp, lens, lab, ll, blank, log_probs=False)
    a3 = ctc_forced_align(torch.log_softmax(3.0 * lp, -1), lens, lab, ll, blank, log_probs=True)
    assert torch.equal(a2.score, a3.score) and torch.equal(a2.path, a3.path)


# ---------------------------------------------------------------- times and words
def test_tokens_to_words_and_time_mapping():
    from deepspeech_amd import align as A
    assert A.frame_time(0) == pytest.approx(0.19) and A.frame_time(10) == pytest.approx(0.59)
    assert A.FRAME_S == pytest.approx(0.04) and A.CENTER_S == pytest.approx(0.19)
    ids = A.text_to_ids("ab c")
    assert ids == [0, 1, ALPHABET.index(" "), 2]
    # A: frames 2-3, B: 5-5, space: 8-8, C: 10-12; 20 frames in all
    al = Alignment(path=torch.full((1, 20), BLANK, dtype=torch.int32),
                   tok_start=torch.tensor([[2, 5, 8, 10, -1]], dtype=torch.int32),
                   tok_end=torch.tensor([[3, 5, 8, 12, -1]], dtype=torch.int32),
                   tok_score=torch.tensor([[math.log(0.5) * 2, math.log(0.25), -1.0, math.log(0.8) * 3, 0.0]]),
                   score=torch.tensor([-7.0]))
    words = A.tokens_to_words(al, [ids + [0]], 0)
    assert [w.text for w in words] == ["AB", "C"]
    assert words[0].start_s == pytest.approx(0.04 * 2 + 0.19 - 0.02)       # 0.25
    assert words[0].end_s == pytest.approx(0.04 * 5 + 0.19 + 0.02)         # 0.41
    assert words[1].start_s == pytest.approx(0.57) and words[1].end_s == pytest.approx(0.69)
    # geometric mean of the per-frame probabilities: (0.5 * 0.5 * 0.25) ** (1/3), and 0.8
    assert words[0].confidence == pytest.approx((0.5 * 0.5 * 0.25) ** (1 / 3), rel=1e-6)
    assert words[1].confidence == pytest.approx(0.8, rel=1e-6)
    # clamping to a known duration
    clamped = A.tokens_to_words(al, [ids + [0]], 0, duration=0.6)
    assert clamped[1].start_s == pytest.approx(0.57) and clamped[1].end_s == 0.6
    assert A.span_seconds(0, 0) == (pytest.approx(0.17), pytest.approx(0.21))
    assert A.span_seconds(0, 3, duration=0.1) == (0.1, 0.1)
    with pytest.raises(ValueError):
        A.text_to_ids("a?b")


def _tiny_uni_model():
    from deepspeech_amd.models import DeepSpeech2
    torch.manual_seed(5)
    m = DeepSpeech2(num_filters=4, num_hidden=48, num_rnn_layers=2, cell="gru", bidirectional=False)
    for blk in (m.conv1, m.conv2):
        blk.running_mean.uniform_(-0.1, 0.1)
        blk.running_var.uniform_(0.5, 1.5)
    with torch.no_grad():
        m.fc_weight.mul_(8.0)                      # sharper frames: a transcript with several labels
    return m.eval()


@pytest.mark.parametrize("decoder", ["greedy", "beam"])
def test_finish_timed_on_the_reference_engine(decoder):
    from deepspeech_amd import align as A
    from deepspeech_amd.infer import StreamingRecognizer
    m = _tiny_uni_model()
    T, B = 338, 2
    rec = StreamingRecognizer(m, decoder=decoder, beam_width=4, batch=B)
    feats = torch.randn(B, T, 161)
    for s in range(0, T, 100):
        rec.accept(feats[:, s:s + 100])
    hyp = rec.finish()
    words = rec.finish_timed()
    assert rec.finish() == hyp                      # finish() is unchanged by it
    assert len(words) == B and any(len(h) > 0 for h in hyp)
    for b in range(B):
        text = A.ids_to_text(hyp[b])
        assert "".join(w.text for w in words[b]) == text.replace(" ", "")
        assert [w.text for w in words[b]] == text.split()
        t = 0.0
        for w in words[b]:
            assert 0.0 <= w.start_s <= w.end_s <= T * 0.01
            assert w.start_s >= t
            t = w.end_s
            assert 0.0 < w.confidence <= 1.0
    if decoder == "greedy":
        lp = torch.cat(rec.logprobs, 0)
        mx = lp.max(-1).values
        got = lp.gather(-1, rec.alignment.path.t().long().unsqueeze(-1)).squeeze(-1)
        assert torch.equal(got, mx)                 # the aligned path is a frame-wise argmax path


def test_aligner_runs_a_bidirectional_model_on_the_cpu():
    from deepspeech_amd import align as A
    from deepspeech_amd.models import DeepSpeech2
    torch.manual_seed(3)
    m = DeepSpeech2(num_filters=4, num_hidden=32, num_rnn_layers=1, cell="gru", bidirectional=True).eval()
    feats = torch.randn(2, 200, 161)
    res = A.Aligner(m).align(feats, torch.tensor([200, 150], dtype=torch.int32), ["ab c", "a" * 60])
    assert res[0].feasible and [w.text for w in res[0].words] == ["AB", "C"]
    assert res[0].score_per_frame == pytest.approx(res[0].score / res[0].frames)
    assert not res[1].feasible and res[1].words == [] and res[1].score == -math.inf   # 60 labels, 29 frames


def test_align_cli_writes_one_json_line_per_utterance(tmp_path):
    import json
    from deepspeech_amd import align as A
    from deepspeech_amd.data.synthetic import FixedShapeBatches, to_device
    from deepspeech_amd.models import DeepSpeech2
    from deepspeech_amd.trainer import LRSchedule, Trainer
    from deepspeech_amd.utils import checkpoint as CK
    torch.manual_seed(0)
    t = Trainer(DeepSpeech2(num_filters=4, num_hidden=16, num_rnn_layers=1, cell="gru"), LRSchedule(1e-3, 100, 0.9),
                moving_avg_decay=0.99)
    t.step(to_device(FixedShapeBatches(2, max_frames=120, seed=0, pool=1).next(), torch.device("cpu")))
    CK.CheckpointManager(str(tmp_path), async_save=False).save(t, 1)
    json.dump({"num_hidden": 16, "num_rnn_layers": 1, "rnn_type": "bidirectional", "num_filters": 4, "cell": "gru",
               "use_fp16": False, "moving_avg_decay": 0.99}, open(tmp_path / "deepSpeech_parameters.json", "w"))
    out = tmp_path / "align.jsonl"
    rc = A.main(["--checkpoint_dir", str(tmp_path), "--eval_dir", str(tmp_path / "eval"), "--dummy", "True",
                 "--batch_size", "2", "--num_examples", "4", "--device", "cpu", "--engine", "ref", "--out", str(out)])
    assert rc == 0
    rows = [json.loads(l) for l in open(out)]
    assert len(rows) == 4
    for r in rows:
        assert set(r) >= {"transcript", "words", "score", "score_per_frame", "feasible"}
        assert r["feasible"] and r["score"] < 0 and r["score_per_frame"] == pytest.approx(r["score"] / r["frames"])
        assert "".join(w["text"] for w in r["words"]) == r["transcript"].replace(" ", "")
        assert all(0.0 <= w["start_s"] <= w["end_s"] for w in r["words"])


# ---------------------------------------------------------------- register budget
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
def test_align_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    rows = KR.analyse(os.path.join(ROOT, "deepspeech_amd", "csrc", "align.hip"))
    assert len(rows) >= 2, "no kernels found"
    bad = [r["name"] for r in rows if r.get("VGPRs Spill", 0) or r.get("ScratchSize [bytes/lane]", 0)]
    assert not bad, bad
