"""fp64 oracles and case tables of the CTC decoders: the prefix beam search (csrc/beam.hip, both
instantiations, and the host decoder runtime/decoder.cpp) and the greedy decoder (csrc/decode.hip).
numpy only; torch and the package are imported where an LM or a bf16 rounding is needed. Used by
tests/test_beam_oracle.py (CPU) and tests/test_beam_cases_gpu.py.

Beam oracle (prefix_search). The beam is a dict keyed by the label tuple, its values (log p of the
paths ending in blank, log p of the paths ending in a label). Per frame, as runtime/decoder.cpp:
  * candidate classes: row[k] >= max(row) + prune, evaluated in fp32 exactly as both
    implementations do, so the three candidate sets are identical by construction;
  * blank:   next[P].pb   += log_add(pb, pnb) + row[blank]
  * repeat:  next[P].pnb  += pnb + row[k]              (k = last label of P: collapses into P)
             next[P+k].pnb += pb + row[k] + w           (a repeat needs a blank between)
  * other k: next[P+k].pnb += log_add(pb, pnb) + row[k] + w
    (w = the LM's folded weight of k in P's state, 0 without an LM; "+=" is log_add)
  * keep the W best by log_add(pb, pnb). A prefix whose probability is zero (log p = -inf) is
    not a hypothesis and is never kept.
Everything but the candidate window is fp64. Beside the beam the oracle returns its cut gap: the
minimum over frames of (score of the W-th kept candidate - score of the best dropped one), frames
with at most W candidates not counting.

Decidability. fp32 implementations can only be held to the oracle's beam where no cut is closer
than their own rounding. HOST_ERR is the largest |host score - oracle score| over the whole table
(measured on the CPU, recomputed by tests/test_beam_oracle.py); MARGIN = 8 x that: the device
differs from the host only in the last ulps of expf / log1pf, and a cut compares two rounded
scores. Every case of the table has a cut gap of at least MARGIN (asserted, never skipped); the
order inside a beam is compared only between neighbours whose oracle scores differ by more than
MARGIN. SCORE_TOL = 4 x HOST_ERR bounds |device score - oracle score| (and pb, pnb): the device
evaluates the host's fp32 formulae, so the bound comes from the reference's own fp32 run.

kernel_model is a transcription of beam.hip's merge and selection logic with either prefix
identity rule: "node" (a prefix is its trie node id: what ctc_beam_kernel<false> did before it
carried fingerprints) and "key" (a prefix is its fingerprint; modelled as the label tuple). It
says which cases the node rule gets wrong (STALE rows) without a GPU.

Greedy oracle (greedy). Per frame the class of the largest logit, the LOWEST index among exact
ties (np.argmax's rule and the kernel's strict ">"); merge repeats, drop blanks; score = the fp64
sum of max log_softmax over the first min(lens, T) frames.
"""
import functools
import math

import numpy as np

NEG = float("-inf")
ALPHA, BETA = 0.8, 0.5                 # LM weight and label bonus of every LM case

# largest |host score - oracle score| over ALL_BEAM_CASES, both final modes: 2.58e-5 measured (case
# lm1-K4-blank0, scores near -45), rounded up to one digit; tests/test_beam_oracle.py recomputes it
HOST_ERR = 3e-5
MARGIN = 8 * HOST_ERR                  # 2.4e-4
SCORE_TOL = 4 * HOST_ERR               # 1.2e-4


def log_add(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def window(row32, prune):
    """candidate classes of one fp32 frame, in fp32 (decoder.cpp and beam.hip: p >= mx + prune)"""
    thr = np.float32(row32.max()) + np.float32(prune)
    return [k for k in range(row32.shape[0]) if row32[k] >= thr]


class LMTables:
    """the folded fp32 weights widened to fp64, the next-state table and the start state"""

    def __init__(self, lm, blank):
        from deepspeech_amd.ops.decode import lm_tables
        w, nxt, start = lm_tables(lm, ALPHA, BETA, blank)
        self.w, self.nxt, self.start, self.blank = w.astype(np.float64), nxt, int(start), blank

    def state(self, prefix):
        s = self.start
        for k in prefix:
            s = int(self.nxt[s, k])
        return s


def prefix_search(lp32, W, blank, prune, lm=None, final=False, trace=False):
    """lp32 [T, K] fp32 log-probs -> ([(prefix, pb, pnb, score)] best first, cut gap). lm: LMTables.
    final (with an LM): score also gets the </s> weight of the prefix' state, sorted again.
    trace: the first result is the list of such beams after 0, 1, .. T frames."""
    lp = lp32.astype(np.float64)
    beam = {(): (0.0, NEG)}
    state = {(): lm.start} if lm else None
    gap = float("inf")

    def listing():
        out = [(P, pb, pnb, log_add(pb, pnb)) for P, (pb, pnb) in beam.items()]
        if lm and final:
            out = [(P, pb, pnb, s + lm.w[state[P], blank]) for P, pb, pnb, s in out]
        return sorted(out, key=lambda e: (-e[3], e[0]))

    snaps = [listing()]
    for t in range(lp.shape[0]):
        cand = window(lp32[t], prune)
        nxt = {}

        def add(P, i, v):
            e = nxt.setdefault(P, [NEG, NEG])
            e[i] = log_add(e[i], v)

        for P, (pb, pnb) in beam.items():
            tot = log_add(pb, pnb)
            w = lm.w[state[P]] if lm else None
            for k in cand:
                p = lp[t, k]
                if k == blank:
                    add(P, 0, tot + p)
                    continue
                wk = w[k] if lm else 0.0
                if P and k == P[-1]:
                    add(P + (k,), 1, pb + p + wk)
                    add(P, 1, pnb + p)
                else:
                    add(P + (k,), 1, tot + p + wk)
        ranked = sorted(((log_add(*v), P) for P, v in nxt.items() if log_add(*v) > NEG), key=lambda e: (-e[0], e[1]))
        if len(ranked) > W:
            gap = min(gap, ranked[W - 1][0] - ranked[W][0])
        beam = {P: tuple(nxt[P]) for _, P in ranked[:W]}
        if lm:
            for P in beam:
                if P not in state:
                    state[P] = int(lm.nxt[state[P[:-1]], P[-1]])
        if trace:
            snaps.append(listing())
    return (snaps if trace else listing()), gap


def brute_force(lp, blank, lm=None, final=False):
    """{prefix: score} from the sum over all K^T paths (fp64); the LM factor is a function of the
    prefix alone"""
    import itertools
    T, K = lp.shape
    acc = {}
    for path in itertools.product(range(K), repeat=T):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        p = sum(lp[t, c] for t, c in enumerate(path))
        acc[tuple(out)] = np.logaddexp(acc.get(tuple(out), NEG), p)
    if lm is None:
        return {P: float(s) for P, s in acc.items()}
    res = {}
    for P, s in acc.items():
        st = lm.start
        for k in P:
            s += lm.w[st, k]
            st = int(lm.nxt[st, k])
        res[P] = float(s + (lm.w[st, blank] if final else 0.0))
    return res


def kernel_model(lp32, W, blank, prune, rule):
    """csrc/beam.hip's frame loop (acoustic) in fp64 with prefix identity `rule` ("node" or "key").
    Returns the beams after 0, 1, .. T frames, each [(prefix, score)] in beam order; a stale
    duplicate shows as a prefix listed twice."""
    lp = lp32.astype(np.float64)
    H = [dict(node=0, last=-1, par=-1, pb=0.0, pnb=NEG, P=())]
    nn = 1
    ident = (lambda h: h["node"]) if rule == "node" else (lambda h: h["P"])
    parent = (lambda h: h["par"]) if rule == "node" else (lambda h: h["P"][:-1])
    snaps = [[((), 0.0)]]
    for t in range(lp.shape[0]):
        cand = set(window(lp32[t], prune))
        tot = [log_add(h["pb"], h["pnb"]) for h in H]
        stays, merged = [], [set() for _ in H]
        for i, h in enumerate(H):
            msrc = -1
            for j, o in enumerate(H):
                if h["last"] >= 0 and ident(o) == parent(h):
                    msrc = j
                if o["last"] >= 0 and parent(o) == ident(h):
                    merged[i].add(o["last"])
            s_pb = tot[i] + lp[t, blank] if blank in cand else NEG
            s_pnb = NEG
            if h["last"] >= 0 and h["last"] in cand:
                s_pnb = h["pnb"] + lp[t, h["last"]]
                if msrc >= 0:
                    m = H[msrc]
                    s_pnb = log_add(s_pnb, (m["pb"] if m["last"] == h["last"] else tot[msrc]) + lp[t, h["last"]])
            stays.append((s_pb, s_pnb))
        pool = [(log_add(*s), i) for i, s in enumerate(stays)]
        for j, h in enumerate(H):
            for k in cand:
                if k != blank and k not in merged[j]:
                    pool.append(((h["pb"] if k == h["last"] else tot[j]) + lp[t, k], W + j * 64 + k))
        pool = sorted((e for e in pool if e[0] > NEG), key=lambda e: (-e[0], e[1]))[:W]
        new = []
        for sc, cid in pool:
            if cid < W:
                new.append(dict(H[cid], pb=stays[cid][0], pnb=stays[cid][1]))
            else:
                j, k = (cid - W) >> 6, (cid - W) & 63
                new.append(dict(node=nn, last=k, par=H[j]["node"], pb=NEG, pnb=sc, P=H[j]["P"] + (k,)))
                nn += 1
        H = new
        snaps.append([(h["P"], log_add(h["pb"], h["pnb"])) for h in H])
    return snaps


def model_diverges(lp32, W, blank, prune, rule):
    """first frame count after which kernel_model(rule)'s beam is not the oracle's (a prefix twice,
    another prefix set, or a score off by more than 1e-9), None if there is none"""
    want = prefix_search(lp32, W, blank, prune, trace=True)[0]
    for t, (g, w) in enumerate(zip(kernel_model(lp32, W, blank, prune, rule), want)):
        ws = {e[0]: e[3] for e in w}
        gp = [p for p, _ in g]
        if len(set(gp)) != len(gp) or set(gp) != set(ws) or any(abs(s - ws[p]) > 1e-9 for p, s in g):
            return t
    return None


# ------------------------------------------------------------------------------ beam inputs
def stream_lp(T, K, sharp, seed, zeros=False):
    """log_softmax(sharp * N(0, 1)) of one stream as fp32 [T, K]; zeros: a fifth of the entries (never
    a frame's largest) are hard zeros, log p = -inf"""
    rng = np.random.default_rng(seed)
    x = sharp * rng.standard_normal((T, K))
    if zeros:
        m = rng.random((T, K)) < 0.2
        m[np.arange(T), x.argmax(1)] = False
        x = np.where(m, NEG, x)
    mx = x.max(1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (x - mx - np.log(np.exp(x - mx).sum(1, keepdims=True))).astype(np.float32)


class BeamCase:
    """One launch geometry: B = len(seeds) streams, stream b the first frames[b] frames of
    stream_lp(T, K, sharp, seeds[b]). lm: None or (order, corpus kind). stale: the seeds for which
    kernel_model's node rule leaves the oracle's beam."""

    def __init__(self, name, K, W, T, blank, prune, sharp, seeds, frames=None, lm=None, zeros=False, stale=()):
        self.name, self.K, self.W, self.T, self.blank, self.prune, self.sharp = name, K, W, T, blank, float(prune), sharp
        self.seeds, self.lm, self.zeros, self.stale = tuple(seeds), lm, zeros, tuple(stale)
        self.frames = tuple(frames) if frames is not None else (T,) * len(self.seeds)
        self.B = len(self.seeds)
        assert len(self.frames) == self.B and T <= 100 and max(self.frames) <= T and set(self.stale) <= set(self.seeds)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def case_lp(case):
    """[T, B, K] fp32, read-only"""
    lp = np.stack([stream_lp(case.T, case.K, case.sharp, s, case.zeros) for s in case.seeds], axis=1)
    lp.setflags(write=False)
    return lp


@functools.lru_cache(maxsize=None)
def case_lm(case):
    """(CharNgramLM, LMTables) of an LM case. "rand": 60 random label strings over the K - 1 labels
    (seed 4, as tests/test_beam_lm_gpu.py); "text": the K = 29 synthetic corpus"""
    if case.lm is None:
        return None, None
    order, kind = case.lm
    if kind == "text":
        from deepspeech_amd.lm import CharNgramLM, synthetic_corpus
        lm = CharNgramLM.train(synthetic_corpus(150, seed=3), order)
    else:
        lm = random_lm(case.K, case.blank, order)
    assert lm.K == case.K and lm.blank == case.blank
    return lm, LMTables(lm, case.blank)


@functools.lru_cache(maxsize=None)
def random_lm(K, blank, order):
    """a CharNgramLM over K classes trained on 60 random label strings. With lm_weight = 0 and
    label_bonus = 0 every folded weight is 0: the LM instantiation then computes the acoustic search"""
    from deepspeech_amd.lm import CharNgramLM
    rng = np.random.default_rng(4)
    labels = [k for k in range(K) if k != blank]
    data = [[labels[i] for i in rng.integers(0, K - 1, size=int(rng.integers(1, 10)))] for _ in range(60)]
    return CharNgramLM.train(data, order, alphabet="".join(chr(48 + i) for i in range(K - 1)), blank=blank)


@functools.lru_cache(maxsize=None)
def case_oracle(case, final=False):
    """per stream (beam, cut gap) of the oracle; computed once, shared, not to be modified"""
    lp = case_lp(case)
    tab = case_lm(case)[1]
    return tuple(prefix_search(lp[: case.frames[b], b], case.W, case.blank, case.prune, tab, final) for b in range(case.B))


def compare(name, got, want, scores=True):
    """got: [(prefix, score)] of an implementation in its beam order; want: the oracle's beam.
    Same prefixes, none twice, same best, same order wherever the oracle's neighbours are more than
    MARGIN apart, scores within SCORE_TOL. Returns the largest score error."""
    gp = [tuple(p) for p, _ in got]
    wp = [e[0] for e in want]
    assert len(set(gp)) == len(gp), "%s: a prefix is in the beam twice: %r" % (name, sorted(p for p in set(gp) if gp.count(p) > 1))
    assert set(gp) == set(wp), "%s: prefixes differ: only got %r, only oracle %r" % (
        name, sorted(set(gp) - set(wp)), sorted(set(wp) - set(gp)))
    ws = {e[0]: e[3] for e in want}
    worst = 0.0
    if scores:
        for p, s in got:
            err = abs(s - ws[tuple(p)])
            worst = max(worst, err)
            assert err <= SCORE_TOL, "%s: score of %r: got %r, oracle %r" % (name, p, s, ws[tuple(p)])
    # order: cut the oracle's list into groups at every gap above MARGIN; the groups come in order
    groups, cur = [], [wp[0]] if wp else []
    for a, b in zip(want, want[1:]):
        if a[3] - b[3] > MARGIN:
            groups.append(cur)
            cur = []
        cur.append(b[0])
    groups.append(cur)
    i = 0
    for g in groups:
        assert set(gp[i:i + len(g)]) == set(g), "%s: beam order: positions %d..%d hold %r, oracle %r" % (
            name, i, i + len(g) - 1, gp[i:i + len(g)], g)
        i += len(g)
    if wp and len(groups[0]) == 1:
        assert gp[0] == wp[0]
    return worst


def tight_frames(case):
    """(frames whose window drops the blank, frames whose window holds a single class)"""
    lp = case_lp(case)
    nob = one = 0
    for b in range(case.B):
        for t in range(case.frames[b]):
            c = window(lp[t, b], case.prune)
            nob += case.blank not in c
            one += len(c) == 1
    return nob, one


# The seeds were chosen on the CPU by the oracle alone, from 0..39: those with a cut gap of at least
# MARGIN (most are); tests/test_beam_oracle.py asserts it for every case. Each case is one launch of
# len(seeds) streams.
C = BeamCase
BEAM_CASES = [
    # ---- stale trie nodes: kernel_model's node rule leaves the oracle's beam on `stale` (at some
    # frame; on 16 and 6 it is back by the last one) and on none of the other seeds
    C("stale-K3", 3, 3, 40, 2, -10, 1.0, (10, 16, 18, 0, 1, 2), stale=(10, 16, 18)),
    C("stale-K4", 4, 4, 60, 3, -10, 1.0, (6, 13, 15, 0, 1, 2), stale=(6, 13, 15)),
    C("stale-K5", 5, 8, 100, 4, -10, 1.0, (0, 20, 28, 4, 6, 8), stale=(0, 20, 28)),
    C("stale-K4-blank0", 4, 4, 80, 0, -2, 2.0, (9, 0, 1, 2), stale=(9,)),
    # ---- K edges: 2; 33 and 64: merge-mask bits >= 32, all 64 class lanes; W = 32 at K = 64
    C("K2", 2, 3, 40, 1, -10, 1.0, (0, 1, 2)),
    C("K33", 33, 8, 40, 32, -10, 2.0, (0, 1, 2)),
    C("K64-W32-blank0", 64, 32, 30, 0, -10, 2.0, (0, 1)),
    # ---- blank in the middle (first and last: above and below)
    C("K5-blank2", 5, 4, 50, 2, -10, 1.0, (2, 4, 5)),
    # ---- W edges; W = 32 over K = 6: nbeam < W for the first frames, the early break
    C("W1", 5, 1, 50, 4, -10, 1.0, (0, 1, 2)),
    C("W2-blank0", 4, 2, 50, 0, -10, 1.0, (0, 1, 2)),
    C("W32-K6", 6, 32, 40, 5, -10, 1.0, (4, 7)),
    C("K29-W16", 29, 16, 60, 28, -10, 2.0, (1, 2)),
    # ---- tight windows: frames without the blank (s_pb = -inf), frames with a single class
    C("prune-1.5", 6, 4, 60, 5, -1.5, 2.0, (0, 1, 2)),
    C("prune-2-blank0", 8, 8, 60, 0, -2, 2.0, (0, 1, 2)),
    # ---- hard zeros: a fifth of the log-probs are -inf
    C("zeros", 6, 4, 50, 3, -10, 1.0, (0, 1, 2), zeros=True),
    # ---- stream layout: one stream; five (row stride 5, idle waves in the last workgroup) with 0, 1 and T frames
    C("B1", 5, 4, 40, 4, -10, 1.0, (0,)),
    C("B5-frames", 5, 4, 40, 4, -10, 1.0, (0, 1, 2, 3, 4), frames=(0, 1, 40, 17, 40)),
]
# ---- LM fusion: orders 1 and 3 over K = 3, 4, 5 with the blank first and last; the K = 29 text LM
_LM_SEEDS = {(3, 0, 1): (0, 1, 2), (3, 0, 3): (0, 1, 2), (3, 2, 1): (0, 1, 3), (3, 2, 3): (0, 1, 2),
             (4, 0, 1): (0, 1, 2), (4, 0, 3): (0, 1, 2), (4, 3, 1): (0, 1, 2), (4, 3, 3): (0, 2, 3),
             (5, 0, 1): (1, 2, 3), (5, 0, 3): (1, 3, 4), (5, 4, 1): (1, 3, 4), (5, 4, 3): (0, 2, 3)}
LM_CASES = [C("lm%d-K%d-blank%d" % (o, K, bl), K, {3: 3, 4: 4, 5: 8}[K], {3: 40, 4: 60, 5: 60}[K], bl, -10, 1.0, sd,
              lm=(o, "rand")) for (K, bl, o), sd in sorted(_LM_SEEDS.items())]
LM_CASES.append(C("lm3-K29-W8", 29, 8, 24, 28, -10, 2.0, (0, 1, 2), frames=(24, 13, 24), lm=(3, "text")))
ALL_BEAM_CASES = BEAM_CASES + LM_CASES
STALE_CASES = [c for c in BEAM_CASES if c.stale]
TIGHT_CASES = [c for c in BEAM_CASES if c.prune > -10 and not c.stale]


# ------------------------------------------------------------------------------ greedy decoder
SENTINEL = -7777
GREEDY_ATOL, GREEDY_RTOL = 1e-2, 1e-4          # the bound of tests/test_kernels_gpu.py::test_ctc_greedy_kernel
# largest |score - oracle| / (atol + rtol |oracle|) seen on an MI355X over GREEDY_CASES: an error of
# 4.9e-5 on a score near -390 (T513-K29-blank28-bf16); the other cases 5e-8 .. 1.3e-5
GREEDY_WORST_SEEN = 0.001


class GreedyCase:
    def __init__(self, T, K, blank, bf16, seed):
        self.T, self.K, self.blank, self.bf16, self.seed = T, K, blank, bf16, seed
        self.name = "T%d-K%d-blank%d-%s" % (T, K, blank, "bf16" if bf16 else "fp32")

    def __repr__(self):
        return self.name


GREEDY_N = 7


@functools.lru_cache(maxsize=None)
def greedy_inputs(case):
    """(logits [T, N, K] fp64 holding fp32- or bf16-exact values, NaN / 2^100 past lens; lens [N]).
    Utterances: 0 random; 1 a run of one label over frames 250..260 between blanks (emits once);
    2 label, blank at 255, the same label at 256 (emits twice); 3 a label at 199, blanks 200..255,
    a label at 256 (a blank run that ends at the block edge); 4 lens 0; 5 lens 1; 6 random with
    lens T - 1 and, in fp32, exact two- and three-way ties at the maximum on every third frame.
    Each pattern is cut off at T."""
    T, K, blank = case.T, case.K, case.blank
    rng = np.random.default_rng(case.seed)
    x = 2.0 * rng.standard_normal((T, GREEDY_N, K))
    lab = [k for k in range(K) if k != blank]
    a, c = lab[0], lab[-1]

    def force(n, t0, t1, k):
        x[t0:min(t1, T), n, :] = 0.1 * rng.standard_normal((max(0, min(t1, T) - t0), K))
        x[t0:min(t1, T), n, k] += 9.0

    force(1, 0, T, blank)
    force(1, 250, 261, a)
    force(2, 0, T, blank)
    force(2, 240, 255, c)
    force(2, 256, 257, c)
    force(3, 0, T, blank)
    force(3, 199, 200, a)
    force(3, 256, 300, c)
    lens = np.array([T, T, T, T, 0, min(1, T), max(T - 1, 1)], np.int32)
    if case.bf16:
        import torch
        x = torch.from_numpy(x).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    else:
        x = x.astype(np.float32).astype(np.float64)
        for t in range(0, T, 3):                        # exact ties: two or three classes share the maximum
            ks = rng.choice(K, size=min(K, 2 + (t // 3) % 2), replace=False)
            x[t, 6, ks] = np.float32(x[t, 6].max() + 1.0)
    for n in range(GREEDY_N):                           # what lies past lens must be ignored
        x[lens[n]:, n, :] = np.nan if n % 2 == 0 else 2.0 ** 100
    x.setflags(write=False)
    return x, lens


def greedy(x, lens, blank):
    """(labels per utterance, fp64 scores). Ties at the maximum: the lowest class index."""
    T, N, K = x.shape
    out, score = [], np.zeros(N)
    for n in range(N):
        L = max(0, min(int(lens[n]), T))
        seq, prev = [], -1
        for t in range(L):
            row = x[t, n]
            k = int(np.argmax(row))                     # first occurrence of the maximum: lowest index
            score[n] += -math.log(np.exp(row - row[k]).sum())
            if k != prev and k != blank:
                seq.append(k)
            prev = k
        out.append(seq)
    return out, score


def greedy_ties(case):
    """frames (inside lens) whose maximum is shared by two or more classes"""
    x, lens = greedy_inputs(case)
    n = 0
    for u in range(x.shape[1]):
        v = x[: lens[u], u]
        n += int(((v == v.max(1, keepdims=True)).sum(1) > 1).sum()) if lens[u] else 0
    return n


GREEDY_CASES = [GreedyCase(1, 2, 0, False, 1), GreedyCase(255, 64, 63, True, 2), GreedyCase(256, 2, 1, False, 3),
                GreedyCase(257, 64, 0, False, 4), GreedyCase(257, 2, 0, True, 5), GreedyCase(513, 29, 28, True, 6),
                GreedyCase(513, 64, 63, False, 7), GreedyCase(256, 29, 28, True, 8)]
