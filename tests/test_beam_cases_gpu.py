"""csrc/beam.hip and csrc/decode.hip against the fp64 oracles of tests/beam_cases.py, case by case.
GpuBeamSearch only, never the host decoder: a failure names the kernel.

Every acoustic case runs through both instantiations: ctc_beam_kernel<false>, and
ctc_beam_kernel<true> with an LM whose folded weights are all zero (lm_weight = label_bonus = 0),
which must compute the same search. The LM cases run <true> with real weights, both final modes.
Per stream: the oracle's prefix set, no prefix twice (a stale trie node shows as a duplicate), the
oracle's best and order (where its scores are more than MARGIN apart), score / pb / pnb within
SCORE_TOL with -inf exactly -inf; the state invariants after every feed; chunked feeding (1..13
frames, the trie table regrown on the way) bitwise equal to whole feeding, also after reset()."""
import numpy as np
import pytest
import torch

import beam_cases as bc

pytestmark = pytest.mark.gpu

CHUNKS = (1, 13, 7, 2, 5, 11, 3)
INSTS = ("acoustic", "lm0")


def _search(case, inst, dev, frames_hint):
    from deepspeech_amd.ops.decode import GpuBeamSearch
    kw = {}
    if case.lm is not None:
        kw = dict(lm=bc.case_lm(case)[0], lm_weight=bc.ALPHA, label_bonus=bc.BETA)
    elif inst == "lm0":
        kw = dict(lm=bc.random_lm(case.K, case.blank, 2), lm_weight=0.0, label_bonus=0.0)
    return GpuBeamSearch(case.B, case.W, case.blank, case.prune, dev, frames_hint=frames_hint, **kw)


def _read(gs, fed, final=False, fresh=True):
    """The beams through the backtrack binding with caller-owned, sentinel-filled buffers, after the
    state invariants of a search whose stream b has seen fed[b] frames (fresh: since it was made;
    reset() leaves the node table as it is). Per stream, in beam order: (prefix, score, pb, pnb,
    lmstate)."""
    from deepspeech_amd.ops import _ext
    B, W = gs.B, gs.W
    L = max(1, int(max(fed)))
    out = torch.full((B, W, L), bc.SENTINEL, device=gs.dev, dtype=torch.int32)
    out_len = torch.full((B, W), bc.SENTINEL, device=gs.dev, dtype=torch.int32)
    score = torch.full((B, W), float("nan"), device=gs.dev, dtype=torch.float32)
    st = (gs.node, gs.last, gs.parent, gs.pb, gs.pnb, gs.nbeam, gs.nodes, gs.nnodes)
    if final and gs.lm is not None:
        _ext.ext().ctc_beam_backtrack_lm(*st, out, out_len, score, gs.lm, gs.lmstate, gs.blank)
    else:
        _ext.ext().ctc_beam_backtrack(*st, out, out_len, score)
    assert int(gs.err.item()) == 0
    nbeam, nnodes, nodes = gs.nbeam.cpu().numpy(), gs.nnodes.cpu().numpy(), gs.nodes.cpu().numpy()
    node, pb, pnb = gs.node.cpu().numpy(), gs.pb.cpu().numpy(), gs.pnb.cpu().numpy()
    lms = gs.lmstate.cpu().numpy() if gs.lm is not None else np.zeros((B, W), np.int32)
    o, n, s = out.cpu().numpy(), out_len.cpu().numpy(), score.cpu().numpy()
    res = []
    for b in range(B):
        nb = int(nbeam[b])
        assert 1 <= nb <= W and (fed[b] > 0 or nb == 1), (b, nb)
        assert 1 <= nnodes[b] <= 1 + W * fed[b], (b, int(nnodes[b]), fed[b])
        assert not (fresh and nodes[b, nnodes[b]:].any()), "stream %d: the node table past nnodes was written" % b
        assert (n[b, nb:] == -1).all() and np.isneginf(s[b, nb:]).all(), (b, n[b], s[b])
        hyps = []
        for h in range(nb):
            depth, x = 0, int(node[b, h])
            assert 0 <= x < nnodes[b]
            while x > 0:
                depth, x = depth + 1, int(nodes[b, x, 0])
            assert n[b, h] == depth, "stream %d hypothesis %d: backtracked length %d, trie depth %d" % (b, h, n[b, h], depth)
            assert (o[b, h, depth:] == bc.SENTINEL).all()
            hyps.append((tuple(o[b, h, :depth].tolist()), float(s[b, h]), float(pb[b, h]), float(pnb[b, h]), int(lms[b, h])))
        res.append(hyps)
    return res


def _component(name, got, want):
    if want == bc.NEG or got == bc.NEG:
        assert got == want, "%s: got %r, oracle %r" % (name, got, want)
    else:
        assert abs(got - want) <= bc.SCORE_TOL, "%s: got %r, oracle %r" % (name, got, want)


def _against_oracle(case, tag, beams, oracle, final=False):
    """beams: _read's result; oracle: per stream (beam, gap). Returns the largest score error."""
    worst = 0.0
    for b in range(case.B):
        name = "%s %s stream %d (seed %d)%s" % (case, tag, b, case.seeds[b], " final" if final else "")
        want = oracle[b][0]
        got = beams[b]
        if final:
            got = sorted(got, key=lambda e: -e[1])               # stable: as GpuBeamSearch.results
        worst = max(worst, bc.compare(name, [(p, s) for p, s, _, _, _ in got], want))
        w = {e[0]: e for e in want}
        for p, _, pb, pnb, _ in got:
            _component(name + " pb of %r" % (p,), pb, w[p][1])
            _component(name + " pnb of %r" % (p,), pnb, w[p][2])
    return worst


def _feed_whole(case, gs, lp):
    gs.feed(lp, torch.tensor(case.frames, dtype=torch.int32, device=lp.device))
    return list(case.frames)


_WHOLE = {}


def _whole(case, inst, dev):
    """the whole-utterance run of a case, made once: (search, beams, final beams)"""
    if (case, inst) not in _WHOLE:
        lp = torch.tensor(bc.case_lp(case)).to(dev)
        gs = _search(case, inst, dev, case.T)
        fed = _feed_whole(case, gs, lp)
        _WHOLE[case, inst] = (gs, lp, _read(gs, fed), _read(gs, fed, final=True))
    return _WHOLE[case, inst]


def _cases():
    return [pytest.param(c, i, id="%s-%s" % (c, i)) for c in bc.BEAM_CASES for i in INSTS] + \
           [pytest.param(c, "lm", id=repr(c)) for c in bc.LM_CASES]


@pytest.mark.parametrize("case,inst", _cases())
def test_whole_feed_matches_the_oracle(cuda, case, inst):
    gs, _, beams, beams_final = _whole(case, inst, cuda)
    worst = _against_oracle(case, inst, beams, bc.case_oracle(case))
    if case.lm is not None:
        worst = max(worst, _against_oracle(case, inst, beams_final, bc.case_oracle(case, True), final=True))
    else:
        assert beams_final == beams                              # no LM weight: no final term
    print("%s %s: largest |score - oracle| %.2e (tolerance %.2e)" % (case, inst, worst, bc.SCORE_TOL))
    # the public accessors say the same
    plain = [[(list(p), s) for p, s, _, _, _ in r] for r in beams]
    assert gs.results() == plain
    assert gs.best() == [r[0][0] for r in plain]
    fin = [sorted(((list(p), s) for p, s, _, _, _ in r), key=lambda e: -e[1]) for r in beams_final]
    assert gs.results(final=True) == fin


@pytest.mark.parametrize("case,inst", _cases())
def test_chunked_feed_equals_whole_feed_bitwise(cuda, case, inst):
    """chunks of 1..13 frames with the smallest trie table, the invariants after every feed; then
    the same search object again after reset()"""
    _, lp, whole, whole_final = _whole(case, inst, cuda)
    gs = _search(case, inst, cuda, 1)
    cap0 = gs.cap
    frames = np.asarray(case.frames)
    s, i = 0, 0
    while s < case.T:
        n = min(CHUNKS[i % len(CHUNKS)], case.T - s)
        gs.feed(lp[s:s + n], torch.from_numpy(np.clip(frames - s, 0, n).astype(np.int32)).to(cuda))
        s, i = s + n, i + 1
        got = _read(gs, np.minimum(frames, s).tolist())
    assert case.T * case.W < cap0 or gs.cap > cap0               # the table was regrown on the way
    assert got == whole, "chunked feeding differs from whole feeding"
    assert _read(gs, case.frames, final=True) == whole_final
    _against_oracle(case, inst + " chunked", got, bc.case_oracle(case))
    gs.reset()
    assert _read(gs, [0] * case.B, fresh=False) == [[((), 0.0, 0.0, bc.NEG, gs.lm_start if gs.lm is not None else 0)]] * case.B
    fed = _feed_whole(case, gs, lp)
    assert _read(gs, fed, fresh=False) == whole and _read(gs, fed, final=True, fresh=False) == whole_final


@pytest.mark.parametrize("inst", INSTS)
@pytest.mark.parametrize("case", bc.STALE_CASES, ids=repr)
def test_stale_cases_frame_by_frame(cuda, case, inst):
    """One frame per launch, the oracle's beam after every frame: a prefix that was pruned and came
    back must merge with its live extensions, not sit in the beam beside them. (On seeds 16 of
    stale-K3 and 6 of stale-K4 the trie-node rule is wrong for some frames and right at the end.)"""
    lp = torch.tensor(bc.case_lp(case)).to(cuda)
    gs = _search(case, inst, cuda, case.T)
    traces = [bc.prefix_search(bc.case_lp(case)[:, b], case.W, case.blank, case.prune, trace=True)[0] for b in range(case.B)]
    for t in range(case.T):
        gs.feed(lp[t:t + 1])
        got = _read(gs, [t + 1] * case.B)
        _against_oracle(case, "%s after %d frames" % (inst, t + 1), got, [(tr[t + 1], None) for tr in traces])


# ------------------------------------------------------------------------------ greedy decoder
_GREEDY_WORST = {}


@pytest.mark.parametrize("case", bc.GREEDY_CASES, ids=repr)
def test_greedy_kernel_matches_the_oracle(cuda, case):
    """the ctc_greedy binding with caller-owned, sentinel-filled buffers: exact labels and counts,
    nothing written past counts, the score within the bound of test_ctc_greedy_kernel"""
    from deepspeech_amd.ops import _ext
    x, lens = bc.greedy_inputs(case)
    T, N = case.T, bc.GREEDY_N
    lg = torch.tensor(x).to(torch.bfloat16 if case.bf16 else torch.float32)
    live = torch.from_numpy(np.nan_to_num(x, nan=0.0))
    assert torch.equal(torch.nan_to_num(lg.double(), nan=0.0), live)      # the device reads the oracle's values
    labels = torch.full((N, T), bc.SENTINEL, device=cuda, dtype=torch.int32)
    counts = torch.full((N,), bc.SENTINEL, device=cuda, dtype=torch.int32)
    score = torch.full((N,), float("nan"), device=cuda, dtype=torch.float32)
    _ext.ext().ctc_greedy(lg.to(cuda).contiguous(), torch.from_numpy(lens).to(cuda), labels, counts, case.blank, score)
    want, wscore = bc.greedy(x, lens, case.blank)
    lab, cnt, sc = labels.cpu().numpy(), counts.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    assert cnt.tolist() == [len(w) for w in want]
    for n in range(N):
        assert lab[n, :cnt[n]].tolist() == want[n], n
        assert (lab[n, cnt[n]:] == bc.SENTINEL).all(), n
    err = np.abs(sc - wscore)
    bound = bc.GREEDY_ATOL + bc.GREEDY_RTOL * np.abs(wscore)
    _GREEDY_WORST[case.name] = float((err / bound).max())
    print("%s: largest score error %.3e, %.3f of the bound" % (case, err.max(), _GREEDY_WORST[case.name]))
    assert (err <= bound).all(), (sc, wscore)
    assert sc[4] == 0.0                                                   # lens 0: no frame, no label
