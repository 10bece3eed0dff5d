"""CPU side of the decoder oracle suite (tests/beam_cases.py): the fp64 prefix search against a
brute-force sum over all K^T paths (every prefix' score, with and without an LM, both final modes);
the host decoder (runtime/decoder.cpp: PrefixBeamSearch, beam_search_batch, BatchBeamSearch)
against the oracle on every case of the table, pruned beams included; the conditions the table
promises (every case decidable under the recorded margin, the margin not smaller than 8 x the
measured host error, tight windows that really drop the blank and really leave one class, which
seeds the trie-node identity rule gets wrong); and the greedy oracle's own cases."""
import functools

import numpy as np
import pytest

import beam_cases as bc
from deepspeech_amd.ops.decode import host_lm
from deepspeech_amd.runtime import native

N = native.load()


# ------------------------------------------------------------------------------ oracle vs brute force
def _tiny_lm(K, blank, order):
    case = bc.BeamCase("tiny", K, 4, 6, blank, -10, 1.0, (0,), lm=(order, "rand"))
    return bc.case_lm(case)[1]


@pytest.mark.parametrize("K,T,blank", [(2, 6, 0), (2, 6, 1), (3, 6, 2), (3, 5, 0), (3, 6, 1)])
@pytest.mark.parametrize("lm_order", [0, 1, 3])
def test_oracle_equals_the_sum_over_all_paths(K, T, blank, lm_order):
    lp = bc.stream_lp(T, K, 1.0, 100 + 10 * K + blank)
    tab = _tiny_lm(K, blank, lm_order) if lm_order else None
    for final in (False, True):
        want = bc.brute_force(lp.astype(np.float64), blank, tab, final)
        got, gap = bc.prefix_search(lp, 4096, blank, -1e30, tab, final)       # exhaustive: nothing is cut
        assert gap == float("inf")
        assert {e[0] for e in got} == set(want) and len(got) == len(want)
        for P, pb, pnb, s in got:
            assert abs(s - want[P]) <= 1e-12 * max(1.0, abs(want[P])), (P, s, want[P])
        assert [e[3] for e in got] == sorted((e[3] for e in got), reverse=True)


# ------------------------------------------------------------------------------ the table's promises
@pytest.mark.parametrize("case", bc.ALL_BEAM_CASES, ids=repr)
def test_every_case_is_decidable(case):
    for b, (beam, gap) in enumerate(bc.case_oracle(case)):
        assert gap >= bc.MARGIN, "%s stream %d (seed %d): cut gap %.3e below the margin %.1e" % (
            case, b, case.seeds[b], gap, bc.MARGIN)
        assert 1 <= len(beam) <= case.W
        assert all(e[3] > bc.NEG for e in beam)


def test_the_table_reaches_what_it_claims():
    t = bc.ALL_BEAM_CASES
    assert {2, 3, 33, 64} <= {c.K for c in t} and {1, 2, 3, 32} <= {c.W for c in t}
    assert any(c.K == 64 and c.W == 32 and c.T == 30 for c in t) and any(c.K == 6 and c.W == 32 for c in t)
    assert {"first", "middle", "last"} <= {"first" if c.blank == 0 else "last" if c.blank == c.K - 1 else "middle" for c in t}
    assert {1, 5} <= {c.B for c in t} and any({0, 1, c.T} <= set(c.frames) for c in t if c.B == 5)
    assert {c.prune for c in bc.TIGHT_CASES} == {-1.5, -2.0}
    assert all(c.T <= 100 for c in t)
    lm = {(c.lm[0], c.K, c.blank) for c in bc.LM_CASES}
    assert {(o, K, bl) for o in (1, 3) for K in (3, 4, 5) for bl in (0, K - 1)} <= lm and (3, 29, 28) in lm
    zeros = [c for c in t if c.zeros]
    assert zeros and all(np.isneginf(bc.case_lp(c)).any() for c in zeros)
    # W = 32 over K = 6: fewer than W hypotheses exist after the first frames
    c = next(c for c in t if c.K == 6 and c.W == 32)
    snaps = bc.prefix_search(bc.case_lp(c)[:, 0], c.W, c.blank, c.prune, trace=True)[0]
    assert len(snaps[1]) < c.W and len(snaps[2]) < c.W and len(snaps[-1]) == c.W


@pytest.mark.parametrize("case", bc.TIGHT_CASES + [c for c in bc.STALE_CASES if c.prune > -10], ids=repr)
def test_tight_windows_drop_the_blank_and_leave_single_classes(case):
    no_blank, single = bc.tight_frames(case)
    assert no_blank > 0 and single > 0, (no_blank, single)


@pytest.mark.parametrize("case", bc.STALE_CASES, ids=repr)
def test_node_identity_model_diverges_only_on_the_stale_seeds(case):
    """The trie-node rule (csrc/beam.hip's acoustic search before it carried fingerprints) leaves
    the oracle's beam on exactly the seeds marked stale; the fingerprint rule on none."""
    lp = bc.case_lp(case)
    for b, seed in enumerate(case.seeds):
        x = lp[: case.frames[b], b]
        assert (bc.model_diverges(x, case.W, case.blank, case.prune, "node") is not None) == (seed in case.stale), seed
        assert bc.model_diverges(x, case.W, case.blank, case.prune, "key") is None, seed


# ------------------------------------------------------------------------------ host decoder vs oracle
def _host_lm(case):
    lm = bc.case_lm(case)[0]
    return None if lm is None else host_lm(lm, bc.ALPHA, bc.BETA, case.blank)


def _in_first_group(best, want):
    """best is the oracle's best, or one of those within MARGIN of it"""
    top = [e[0] for e in want if want[0][3] - e[3] <= bc.MARGIN]
    return tuple(best) in top


@functools.lru_cache(maxsize=None)
def _host_against_oracle(case):
    """every assertion of the host comparison; returns the largest |host score - oracle score|"""
    lp = bc.case_lp(case)
    L = _host_lm(case)
    lens = np.asarray(case.frames, np.int32)
    worst = 0.0
    for final in ((False, True) if L is not None else (False,)):
        want = bc.case_oracle(case, final)
        for b in range(case.B):
            bs = N.PrefixBeamSearch(case.W, case.blank, case.prune, L)
            bs.feed(np.ascontiguousarray(lp[: case.frames[b], b]))
            name = "%s stream %d final %d" % (case, b, final)
            worst = max(worst, bc.compare(name, bs.results(final), want[b][0]))
            assert _in_first_group(bs.best(final), want[b][0]), name
        for threads in (1, 3):
            got = N.beam_search_batch(lp, lens, case.W, case.blank, case.prune, threads, lm=L, final=final)
            assert all(_in_first_group(got[b], want[b][0]) for b in range(case.B)), (threads, final)
        bb = N.BatchBeamSearch(case.B, case.W, case.blank, case.prune, 2, lm=L)
        for s in range(0, case.T, 13):
            chunk = np.ascontiguousarray(lp[s:s + 13])
            bb.feed(chunk, np.clip(lens - s, 0, chunk.shape[0]).astype(np.int32))
        assert all(_in_first_group(p, want[b][0]) for b, p in enumerate(bb.best(final))), final
    return worst


@pytest.mark.parametrize("case", bc.ALL_BEAM_CASES, ids=repr)
def test_host_decoder_matches_the_oracle(case):
    """Same prefixes, same order (where the margin decides it) and scores: the host decoder's first
    test of a pruned beam. One stream, the threaded batch call and the chunked stream set."""
    _host_against_oracle(case)


def test_margin_and_tolerance_come_from_the_measured_host_error():
    """MARGIN >= 8 x the largest |host score - oracle score| over the whole table, SCORE_TOL = 4 x
    the recorded error."""
    errs = {c.name: _host_against_oracle(c) for c in bc.ALL_BEAM_CASES}
    measured = max(errs.values())
    print("largest |host score - oracle score| over the table: %.3e (%s)" % (measured, max(errs, key=errs.get)))
    assert measured > 0.0
    assert bc.HOST_ERR >= measured and bc.MARGIN >= 8 * measured
    assert bc.MARGIN == 8 * bc.HOST_ERR and bc.SCORE_TOL == 4 * bc.HOST_ERR
    assert bc.HOST_ERR <= 2 * measured, "HOST_ERR is a measurement, not an allowance: re-measure it"


# ------------------------------------------------------------------------------ greedy oracle
def test_greedy_cases_hold_what_they_claim():
    cs = bc.GREEDY_CASES
    assert {1, 255, 256, 257, 513} <= {c.T for c in cs}
    assert {(2, 0), (2, 1), (64, 0), (64, 63)} <= {(c.K, c.blank) for c in cs}
    for c in cs:
        x, lens = bc.greedy_inputs(c)
        assert {0, min(1, c.T), c.T} <= set(lens.tolist())
        assert all(not (np.abs(x[lens[n]:, n]) < 1e29).any() for n in range(bc.GREEDY_N))   # NaN or 2^100 past lens
        assert bc.greedy_ties(c) > 0 or c.T == 1, c                  # constructed in fp32, natural in bf16
        seqs, score = bc.greedy(x, lens, c.blank)
        assert seqs[4] == [] and score[4] == 0.0 and np.isfinite(score).all()
        lab = [k for k in range(c.K) if k != c.blank]
        if c.T >= 261:
            assert seqs[1] == [lab[0]]                               # a run over the block edge emits once
        if c.T >= 257:
            assert seqs[2] == [lab[-1], lab[-1]]                     # label, blank at 255, label at 256: twice
            assert seqs[3] == [lab[0], lab[-1]]                      # the blank run ends at the block edge
    # the tie rule: the lowest class index
    x = np.zeros((1, 1, 4))
    x[0, 0, [1, 3]] = 2.0
    assert bc.greedy(x, np.array([1]), 0)[0] == [[1]]
    assert bc.greedy(x, np.array([1]), 1)[0] == [[]]


def test_greedy_oracle_matches_the_reference_decoder():
    import torch
    from deepspeech_amd.ops import reference as R
    for c in bc.GREEDY_CASES:
        x, lens = bc.greedy_inputs(c)
        seqs, score = bc.greedy(x, lens, c.blank)
        clean = torch.from_numpy(np.nan_to_num(x, nan=0.0, posinf=0.0)).clamp(max=1e3)
        lp = torch.log_softmax(clean, -1)
        assert R.greedy_decode(lp, torch.from_numpy(lens), c.blank) == seqs, c
        ref = [float(lp[: int(lens[n]), n].max(-1).values.sum()) for n in range(bc.GREEDY_N)]
        np.testing.assert_allclose(score, ref, rtol=1e-12, atol=1e-9)
