// CTC prefix beam search on the GPU (SURVEY K15 "beam later"; VERDICT r5 missing item 4).
//
// The host version (runtime/decoder.cpp PrefixBeamSearch) keeps a trie in a hash map and, with
// a near-uniform frame (a young model, all 29 classes within the prune window), creates ~450 trie
// nodes per frame per stream; with 32 streams that host loop, plus the per-chunk log-prob copy
// and sync, made beam-16 cost 2.6x the greedy decode in streaming inference. Here the beams stay
// on the device between chunks and one wave64 decodes one stream:
//
//   * lane i < nbeam holds hypothesis i (trie node, last label, parent node, log p ending in
//     blank / non-blank, and the 64-bit fingerprints of its prefix and of its parent's prefix);
//     lane k < K holds class k's log-prob of the frame;
//   * merging needs no hash map: distinct hypotheses have distinct prefixes, so the extension
//     of hypothesis j by label k reaches an existing prefix only when some hypothesis i has
//     parent_key(i) == key(j) and last(i) == k; it then adds into i's "stay" entry (CPU: the
//     same get(node) slot), otherwise it is a new prefix whose trie node is created only if it
//     survives the top-W selection;
//   * lane k scores the W extensions by class k (the hypotheses broadcast with readlane), the
//     selection is W rounds of a wave arg-max (ties: lower candidate id; stays before
//     extensions), and the survivors' new trie nodes (parent, label) are appended to the
//     stream's node table, which the backtrack kernel walks at the end.
//
// Every score is a log_add of at most two terms (own stay + one merged extension) or one term,
// so the float results do not depend on accumulation order; they equal the host decoder's up
// to the ulps of expf / log1pf. Reference semantics: tf.nn.ctc_beam_search_decoder (the
// reference itself decodes greedily, src/deepSpeech_test.py:212-215).
//
// Prefix identity. A prefix is identified by its fingerprint, never by its trie node: key of a
// prefix = mix(key of its parent, label), key of the empty prefix = 0, carried in lane registers
// and stored beside the beam state between launches (registers only, no loads in the frame loop).
// A trie node id does not identify a live prefix: when a prefix P is pruned while a longer
// Q = P + x stays live and P is then created again from its own parent, P gets a fresh node and Q
// still points to the old one; a node-id test then no longer sees that P + x is Q, the beam holds Q
// twice and Q's probability is split. Small alphabets meet this within tens of frames (K = 3,
// W = 3), and LM weights reorder a K = 29 beam enough to meet it within 30 frames
// (tests/beam_cases.py, the stale cases). The trie nodes are only what the backtrack walks: two
// nodes of one prefix spell the same labels. Two different live prefixes one label apart collide
// with probability 2^-64 per comparison.
//
// Shallow LM fusion (ctc_beam_kernel<true>; deepspeech_amd/lm.py): the LM is a backoff-expanded
// automaton packed as int2 rows lm[state][k] = (w, next) with w = alpha * ln P(k | state) + beta
// as fp32 bits. Each hypothesis carries its state in a lane register beside its node; at the top
// of a frame lane k loads row state_j, column k for every live j (W coalesced 8-byte loads whose
// latency overlaps the merge scan and the frame's own log-prob load), every extension term gets
// (base + p) + w, and when (j, k) is selected the survivor's state is a readlane of the `next`
// lane k already holds: nothing loads inside the serial selection. The <false> instantiation is
// the same search without the LM terms.
#include "common.h"

using namespace ds2;

namespace {

constexpr int BM_MAXW = 32;   // beam width bound (lane registers per class lane)

__device__ __forceinline__ float log_add(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const float m = fmaxf(a, b);
  return m + log1pf(expf(-fabsf(a - b)));
}

struct BeamArgs {
  const float* lp;     // [T][B][K] log-probs (time-major)
  const int* frames;   // [B] frames of this call per stream (<= T), nullptr: T for every stream
  int T, B, K, W, blank;
  float prune;         // classes below (frame max + prune) are not extended (<= 0)
  int* node;           // [B][W] trie node of each hypothesis (0 = empty prefix)
  int* last;           // [B][W] last label (-1: empty prefix)
  int* parent;         // [B][W] parent trie node (-1: empty prefix)
  float* pb;           // [B][W] log p(prefix, ends in blank)
  float* pnb;          // [B][W] log p(prefix, ends in a label)
  int* nbeam;          // [B] live hypotheses
  int2* nodes;         // [B][cap] trie nodes: (parent, label)
  int* nnodes;         // [B] nodes used
  int cap;
  unsigned* err;       // bit 1: node table full (host sizes it: 1 + W * frames)
  unsigned long long* key;     // [B][W][2] fingerprint of each hypothesis' prefix and of its parent's
  const int2* lm;      // LM only: [S][K] (w fp32 bits, next state; column blank: (w of </s>, -1))
  int* lmstate;        // LM only: [B][W] LM state of each hypothesis
  int S;
};

__device__ __forceinline__ unsigned long long bcast(unsigned long long v, int l) {
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
         (unsigned)__builtin_amdgcn_readlane((int)v, l);
}

// fingerprint of prefix + label (splitmix64 finaliser over parent key and label)
__device__ __forceinline__ unsigned long long key_extend(unsigned long long parent, int label) {
  unsigned long long x = parent + (unsigned long long)(label + 1) * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

template <bool LM>
__global__ __launch_bounds__(256) void ctc_beam_kernel(BeamArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= a.B) return;                                // the whole wave leaves together
  const int W = a.W, K = a.K;
  const size_t bo = (size_t)b * W;
  int nb = a.nbeam[b];
  int nn = a.nnodes[b];
  int h_node = 0, h_last = -1, h_par = -1;
  float h_pb = -INFINITY, h_pnb = -INFINITY;
  int h_state = 0;
  unsigned long long h_key = 0ull, h_pkey = 0ull;
  if constexpr (LM) {
    if (lane < nb) h_state = min(max(a.lmstate[bo + lane], 0), a.S - 1);
  }
  if (lane < nb) {
    h_key = a.key[(bo + lane) * 2];
    h_pkey = a.key[(bo + lane) * 2 + 1];
    h_node = a.node[bo + lane];
    h_last = a.last[bo + lane];
    h_par = a.parent[bo + lane];
    h_pb = a.pb[bo + lane];
    h_pnb = a.pnb[bo + lane];
  }
  int2* const tab = a.nodes + (size_t)b * a.cap;
  const int T = a.frames ? min(a.frames[b], a.T) : a.T;
  for (int t = 0; t < T; ++t) {
    if (nn + W > a.cap) {                              // cannot happen when the host sized it
      if (lane == 0) atomicOr(a.err, 1u);
      break;
    }
    // lane k: (w, next) of every live hypothesis j's LM state for class k
    int2 wn[LM ? BM_MAXW : 1];
    if constexpr (LM) {
#pragma unroll
      for (int j = 0; j < BM_MAXW; ++j) {
        wn[j] = make_int2(0, 0);
        if (j < nb) {
          const int sj = bcast(h_state, j);
          if (lane < K) wn[j] = a.lm[(size_t)sj * K + lane];
        }
      }
    }
    const float p = lane < K ? a.lp[((size_t)t * a.B + b) * K + lane] : -INFINITY;
    float mx = p;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const unsigned long long cmask = __ballot(lane < K && p >= mx + a.prune);
    const bool live = lane < nb;
    const float tot = live ? log_add(h_pb, h_pnb) : -INFINITY;
    // merge source of my hypothesis: the live hypothesis whose prefix is my prefix' parent, so
    // that its extension by my last label is my prefix (h_last < 0: the empty prefix has none)
    int msrc = -1;
    for (int i = 0; i < nb; ++i) {
      const unsigned long long ki = bcast(h_key, i);
      if (live && h_last >= 0 && ki == h_pkey) msrc = i;
    }
    // the same relation seen from the class lanes: bit j of lane k says that the extension of
    // hypothesis j by class k is an existing hypothesis (it merges into that one's stay entry)
    unsigned kmask = 0u;
    for (int i = 0; i < nb; ++i) {
      const int mi = bcast(msrc, i), li = bcast(h_last, i);
      if (mi >= 0 && li == lane) kmask |= 1u << mi;
    }
    // LM weight of the merged extension: row state(msrc), column my last label
    float m_w = 0.f;
    if constexpr (LM) {
      const int m_state = __shfl(h_state, msrc >= 0 ? msrc : 0, 64);
      if (msrc >= 0 && h_last >= 0) m_w = __int_as_float(a.lm[(size_t)m_state * K + h_last].x);
    }
    // stay entry of my hypothesis: blank, a repeat of the last label, and the merged extension
    const float pblank = __shfl(p, a.blank, 64);
    const float plast = __shfl(p, h_last >= 0 ? h_last : 0, 64);
    const int ms = msrc >= 0 ? msrc : 0;
    const float m_pb = __shfl(h_pb, ms, 64), m_tot = __shfl(tot, ms, 64);
    const int m_last = __shfl(h_last, ms, 64);
    float s_pb = -INFINITY, s_pnb = -INFINITY;
    if (live) {
      if ((cmask >> a.blank) & 1ull) s_pb = tot + pblank;
      if (h_last >= 0 && ((cmask >> h_last) & 1ull)) {
        s_pnb = h_pnb + plast;
        if constexpr (LM) {
          if (msrc >= 0) s_pnb = log_add(s_pnb, ((m_last == h_last ? m_pb : m_tot) + plast) + m_w);
        } else {
          if (msrc >= 0) s_pnb = log_add(s_pnb, (m_last == h_last ? m_pb : m_tot) + plast);
        }
      }
    }
    float stay = live ? log_add(s_pb, s_pnb) : -INFINITY;
    // lane k: the extensions of every hypothesis j by class k that are new prefixes
    float ext[BM_MAXW];
    const bool kc = lane < K && lane != a.blank && ((cmask >> lane) & 1ull);
#pragma unroll
    for (int j = 0; j < BM_MAXW; ++j) {
      ext[j] = -INFINITY;
      if (j < nb) {
        const float tj = bcast(tot, j), pj = bcast(h_pb, j);
        const int lj = bcast(h_last, j);
        if constexpr (LM) {
          if (kc && !((kmask >> j) & 1u)) ext[j] = ((lane == lj ? pj : tj) + p) + __int_as_float(wn[j].x);
        } else {
          if (kc && !((kmask >> j) & 1u)) ext[j] = (lane == lj ? pj : tj) + p;
        }
      }
    }
    // top-W: stays have ids 0..W-1, extension (j, k) id W + j * 64 + k
    int nsel = 0, newn = 0;
    int n_node = 0, n_last = -1, n_par = -1;
    float n_pb = -INFINITY, n_pnb = -INFINITY;
    int n_state = 0;
    int n_src = 0;                                     // the hypothesis my survivor stays on or extends
    bool n_ext = false;
    for (int r = 0; r < W; ++r) {
      float best = stay;
      int bid = live ? lane : 0x7fffffff;
#pragma unroll
      for (int j = 0; j < BM_MAXW; ++j)
        if (ext[j] > best) {                           // ids grow with j: strict > keeps the lowest
          best = ext[j];
          bid = W + j * 64 + lane;
        }
      if (best == -INFINITY) bid = 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bid, o, 64);
        if (ob > best || (ob == best && oi < bid)) {
          best = ob;
          bid = oi;
        }
      }
      bid = __builtin_amdgcn_readfirstlane(bid);
      if (bid == 0x7fffffff) break;                    // fewer than W finite candidates
      if (bid < W) {
        const int j = bid;
        if (lane == j) stay = -INFINITY;
        const int nj = bcast(h_node, j), lj = bcast(h_last, j), pj = bcast(h_par, j);
        const float bj = bcast(s_pb, j), qj = bcast(s_pnb, j);
        if constexpr (LM) {
          const int sj = bcast(h_state, j);            // a stay keeps its state
          if (lane == r) n_state = sj;
        }
        if (lane == r) {
          n_src = j;
          n_node = nj;
          n_last = lj;
          n_par = pj;
          n_pb = bj;
          n_pnb = qj;
        }
      } else {
        const int e = bid - W, j = e >> 6, k = e & 63;
        if (lane == k) {
#pragma unroll
          for (int q = 0; q < BM_MAXW; ++q)
            if (q == j) ext[q] = -INFINITY;
        }
        if constexpr (LM) {
          int nx = 0;
#pragma unroll
          for (int q = 0; q < BM_MAXW; ++q)
            if (q == j) nx = wn[q].y;
          const int sk = min(max(bcast(nx, k), 0), a.S - 1);   // lane k holds next(state_j, k)
          if (lane == r) n_state = sk;
        }
        const int nj = bcast(h_node, j);
        const int id = nn + newn;
        ++newn;
        if (lane == r) {
          n_src = j;
          n_ext = true;
          n_node = id;
          n_last = k;
          n_par = nj;
          n_pb = -INFINITY;
          n_pnb = best;
          tab[id] = make_int2(nj, k);
        }
      }
      ++nsel;
    }
    // the survivors' keys, every lane at once (nothing of this in the serial selection): a stay
    // keeps its keys, the extension of j by k gets (key_extend(key_j, k), key_j)
    const unsigned long long kj = __shfl(h_key, n_src, 64), pkj = __shfl(h_pkey, n_src, 64);
    const unsigned long long n_key = lane >= nsel ? 0ull : n_ext ? key_extend(kj, n_last) : kj;
    const unsigned long long n_pkey = lane >= nsel ? 0ull : n_ext ? kj : pkj;
    nb = nsel;
    nn += newn;
    h_node = n_node;
    h_last = n_last;
    h_par = n_par;
    h_pb = n_pb;
    h_pnb = n_pnb;
    h_key = n_key;
    h_pkey = n_pkey;
    if constexpr (LM) h_state = n_state;
  }
  if constexpr (LM) {
    if (lane < W) a.lmstate[bo + lane] = h_state;
  }
  if (lane < W) {
    a.key[(bo + lane) * 2] = h_key;
    a.key[(bo + lane) * 2 + 1] = h_pkey;
    a.node[bo + lane] = h_node;
    a.last[bo + lane] = h_last;
    a.parent[bo + lane] = h_par;
    a.pb[bo + lane] = h_pb;
    a.pnb[bo + lane] = h_pnb;
  }
  if (lane == 0) {
    a.nbeam[b] = nb;
    a.nnodes[b] = nn;
  }
}

// labels of every live hypothesis: out [B][W][Lcap] (reversed walk written back to front),
// out_len [B][W] (-1: no such hypothesis), score [B][W] = log_add(pb, pnb); with lm (final
// mode) plus the </s> weight of the hypothesis' LM state, lm[state][eos].x
__global__ __launch_bounds__(64) void ctc_beam_backtrack_kernel(const int2* nodes, int cap, const int* node,
                                                                  const int* nbeam, const float* pb, const float* pnb,
                                                                  int B, int W, int* out, int* out_len, float* score,
                                                                  int Lcap, const int2* lm, const int* lmstate, int S,
                                                                  int K, int eos) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * W) return;
  const int b = i / W, h = i - b * W;
  if (h >= nbeam[b]) {
    out_len[i] = -1;
    score[i] = -INFINITY;
    return;
  }
  const int2* tab = nodes + (size_t)b * cap;
  int len = 0;
  for (int n = node[i]; n > 0 && len <= Lcap; n = tab[n].x) ++len;
  const int L = min(len, Lcap);
  int pos = L;
  for (int n = node[i]; n > 0 && pos > 0; n = tab[n].x) out[(size_t)i * Lcap + --pos] = tab[n].y;
  out_len[i] = L;
  float sc = log_add(pb[i], pnb[i]);
  if (lm != nullptr) sc += __int_as_float(lm[(size_t)min(max(lmstate[i], 0), S - 1) * K + eos].x);
  score[i] = sc;
}

}  // namespace

extern "C" int ds2_ctc_beam(const float* lp, const int* frames, int T, int B, int K, int W, int blank, float prune,
                            int* node, int* last, int* parent, float* pb, float* pnb, int* nbeam, void* nodes,
                            int* nnodes, int cap, unsigned* err, unsigned long long* key, hipStream_t st) {
  if (K < 2 || K > 64 || W < 1 || W > BM_MAXW || blank < 0 || blank >= K || B < 1 || T < 0 || cap < 1) return -50;
  if (key == nullptr) return -51;
  if (T == 0) return 0;
  BeamArgs a{lp, frames, T, B, K, W, blank, prune, node, last, parent, pb, pnb, nbeam,
             static_cast<int2*>(nodes), nnodes, cap, err, key, nullptr, nullptr, 0};
  ds2_launch(ctc_beam_kernel<false>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

// the same search with the LM automaton lm [S][K] int2 and the per-hypothesis states lmstate [B][W]
extern "C" int ds2_ctc_beam_lm(const float* lp, const int* frames, int T, int B, int K, int W, int blank, float prune,
                               int* node, int* last, int* parent, float* pb, float* pnb, int* nbeam, void* nodes,
                               int* nnodes, int cap, unsigned* err, const void* lm, int S, int* lmstate,
                               unsigned long long* key, hipStream_t st) {
  if (K < 2 || K > 64 || W < 1 || W > BM_MAXW || blank < 0 || blank >= K || B < 1 || T < 0 || cap < 1) return -50;
  if (lm == nullptr || lmstate == nullptr || key == nullptr || S < 1 || (long long)S * K >= (1ll << 31))
    return -51;
  if (T == 0) return 0;
  BeamArgs a{lp, frames, T, B, K, W, blank, prune, node, last, parent, pb, pnb, nbeam,
             static_cast<int2*>(nodes), nnodes, cap, err, key, static_cast<const int2*>(lm), lmstate, S};
  ds2_launch(ctc_beam_kernel<true>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

extern "C" int ds2_ctc_beam_backtrack(const void* nodes, int cap, const int* node, const int* nbeam, const float* pb,
                                      const float* pnb, int B, int W, int* out, int* out_len, float* score, int Lcap,
                                      hipStream_t st) {
  if (B < 1 || W < 1 || Lcap < 1) return -50;
  ds2_launch(ctc_beam_backtrack_kernel, dim3((unsigned)((B * W + 63) / 64)), dim3(64), 0, st,
             static_cast<const int2*>(nodes), cap, node, nbeam, pb, pnb, B, W, out, out_len, score, Lcap,
             static_cast<const int2*>(nullptr), static_cast<const int*>(nullptr), 0, 0, 0);
  return (int)hipGetLastError();
}

// final mode: score additionally gets the </s> weight lm[lmstate][blank].x (the host sorts again)
extern "C" int ds2_ctc_beam_backtrack_lm(const void* nodes, int cap, const int* node, const int* nbeam,
                                         const float* pb, const float* pnb, int B, int W, int* out, int* out_len,
                                         float* score, int Lcap, const void* lm, int S, int K, int blank,
                                         const int* lmstate, hipStream_t st) {
  if (B < 1 || W < 1 || Lcap < 1) return -50;
  if (lm == nullptr || lmstate == nullptr || S < 1 || K < 2 || blank < 0 || blank >= K) return -51;
  ds2_launch(ctc_beam_backtrack_kernel, dim3((unsigned)((B * W + 63) / 64)), dim3(64), 0, st,
             static_cast<const int2*>(nodes), cap, node, nbeam, pb, pnb, B, W, out, out_len, score, Lcap,
             static_cast<const int2*>(lm), lmstate, S, K, blank);
  return (int)hipGetLastError();
}
