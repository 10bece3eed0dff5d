// CTC forced alignment for gfx950: the best (Viterbi) path of a label sequence through the
// frame-wise log-probabilities, with per-frame classes, per-label frame spans and scores.
// Same lattice as ctc.hip's alpha recursion (blank = any class, time-major emissions), with max
// in place of the 3-way log-sum-exp, plus 2-bit back-pointers and a backtrack.
//
// Two launches on one stream, no host synchronisation:
//   1. align_lp_kernel    one wave per valid (t, b) frame -> lp[N][T][32] fp32. log_probs != 0:
//                         the emissions as they are (bf16 widened exactly); else their
//                         log-softmax (x - max - logf(sum expf(x - max)), like torch's).
//   2. ctc_align_kernel   ONE WAVE per utterance. Forward: lane l owns lattice states
//                         [l*SPL, l*SPL+SPL) in registers (state s: even = blank, odd = label
//                         s >> 1), the s-1 / s-2 neighbours across a lane boundary come by DPP
//                         wave_shr:1, lp rows are staged through LDS 64 frames at a time.
//                           v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), [v_{t-1}(s-2)]) + lp_t(class(s))
//                         in plain fp32 (compare / select, then ONE add, natural-log units), so a
//                         CPU oracle doing the same fp32 operations gets the same bits.
//                         TIE RULE: on equal values the path stays (s), then takes s-1, then s-2
//                         (strict > in that order); at the end state 2L wins over 2L-1.
//                         Back-pointers (0 stay, 1 from s-1, 2 from s-2), 2 bits per state, are
//                         packed per lane and frame (one 32-bit word for SPL <= 16, two for
//                         SPL = 32) and streamed to bp_ws[N][T][64][W].
//                         Backtrack (same wave, after a fence): back-pointer rows come back
//                         through LDS 64 frames at a time (coalesced loads, all 64 in flight,
//                         the next chunk's issued before this one is walked), the serial walk
//                         t = len-1 .. 0 then reads LDS only; the per-frame classes,
//                         label spans and label scores of a chunk are produced by 64 lanes in
//                         parallel from the walked states.
// An utterance without a finite path (len <= 0, fewer frames than labels + adjacent repeats,
// -inf emissions on every path) gets score -inf, path -1 and spans -1; a NaN frame gives score
// NaN (like the CTC loss) with path / spans -1. No inter-workgroup wait anywhere.
#include <type_traits>

#include "common.h"

using namespace ds2;

namespace {

constexpr int KPAD = 32;
constexpr int FR = 64;        // frames per staged chunk (one per lane)
constexpr int LCAP = 1024;    // labels per utterance the widest register tile holds (2L+1 <= 2048)
constexpr float NEG_INF = -INFINITY;

template <typename ET>
__device__ __forceinline__ float ld_em(const ET* p);
template <>
__device__ __forceinline__ float ld_em<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld_em<bf16_t>(const bf16_t* p) { return bf2f(*p); }

// ---------------------------------------------------------------- 1. log-probabilities
template <typename ET>
__global__ __launch_bounds__(256) void align_lp_kernel(const ET* __restrict__ em, const int* __restrict__ lens,
                                                       float* __restrict__ lp_ws, int T, int N, int K, int log_probs) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= T * N) return;
  const int t = w / N, b = w % N;
  if (t >= lens[b]) return;
  const float x = (lane < K) ? ld_em<ET>(em + (size_t)w * K + lane) : NEG_INF;
  float y = x;
  if (!log_probs) {
    const float m = wave_max(x);
    const float sum = wave_sum((lane < K) ? expf(x - m) : 0.f);
    y = x - m - logf(sum);
  }
  if (lane < KPAD) lp_ws[((size_t)b * T + t) * KPAD + lane] = (lane < K) ? y : NEG_INF;
}

// class of lattice state s; a label id outside the 32-wide lp rows maps to the padding column
// (-inf: no finite path through it) instead of indexing out of the row
__device__ __forceinline__ int align_class(const int* labels, int b, int Lmax, int s, int blank) {
  const int c = (s & 1) ? labels[(size_t)b * Lmax + (s >> 1)] : blank;
  DS2_DCHECK(c >= 0 && c < KPAD);                    // label ids index the 32-wide lp rows
  return ((unsigned)c < (unsigned)KPAD) ? c : KPAD;
}

// ---------------------------------------------------------------- 2. Viterbi + backtrack
template <int SPL>
__global__ __launch_bounds__(64) void ctc_align_kernel(const int* __restrict__ lens, const int* __restrict__ labels,
                                                       const int* __restrict__ label_lens,
                                                       const float* __restrict__ lp_ws, unsigned* __restrict__ bp_ws,
                                                       int* __restrict__ path, int* __restrict__ tok_start,
                                                       int* __restrict__ tok_end, float* __restrict__ tok_score,
                                                       float* __restrict__ score, int T, int N, int Lmax, int blank) {
  constexpr int W = SPL > 16 ? 2 : 1;                // back-pointer words per lane and frame
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = min(lens[b], T);
  const int L = max(0, min(label_lens[b], Lmax));    // a label length past the padded width reads no other row
  const int SP = 2 * L + 1;
  int* path_b = path + (size_t)b * T;
  int* ts_b = tok_start + (size_t)b * Lmax;
  int* te_b = tok_end + (size_t)b * Lmax;
  float* tsc_b = tok_score + (size_t)b * Lmax;
  auto no_path = [&](float sc) {
    for (int t = lane; t < T; t += 64) path_b[t] = -1;
    for (int l = lane; l < Lmax; l += 64) {
      ts_b[l] = -1;
      te_b[l] = -1;
      tsc_b[l] = 0.f;
    }
    if (lane == 0) score[b] = sc;
  };
  if (len <= 0 || L > len) {
    no_path(NEG_INF);
    return;
  }
  const int s0 = lane * SPL;
  int cls[SPL];
  unsigned skip = 0;   // bit j: the s-2 transition into state s0+j exists
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    const int s = s0 + j;
    // states past the lattice read the staged rows' padding column KPAD, which holds -inf:
    // their values stay -inf without a per-state select in the frame loop
    cls[j] = (s < SP) ? align_class(labels, b, Lmax, s, blank) : KPAD;
    const bool ok = s < SP && (s & 1) && s >= 2 && cls[j] != align_class(labels, b, Lmax, s - 2, blank);
    skip |= (ok ? 1u : 0u) << j;
  }
  const float* lp = lp_ws + (size_t)b * T * KPAD;
  unsigned* bp = bp_ws + (size_t)b * T * (64 * W);
  // lp rows staged through LDS in chunks of 64 frames (one 128-B row per lane): the per-frame
  // gathers are LDS reads, not global loads queued behind the back-pointer stores
  __shared__ float lps[FR][KPAD + 1];
  lps[lane][KPAD] = NEG_INF;                         // never overwritten by stage()
  // max / compare drop a NaN operand, so the recursion cannot carry a NaN frame to the score:
  // the staged rows are tested instead, off the frame chain
  bool nan = false;
  auto stage = [&](int c0) {   // frames c0 .. c0+63
    const int t = c0 + lane;
    __builtin_amdgcn_wave_barrier();
    if (t < len) {
      const float4* src = reinterpret_cast<const float4*>(lp + (size_t)t * KPAD);
#pragma unroll
      for (int q = 0; q < KPAD / 4; ++q) {
        const float4 v4 = src[q];
        nan = nan || (v4.x != v4.x) || (v4.y != v4.y) || (v4.z != v4.z) || (v4.w != v4.w);
        lps[lane][4 * q + 0] = v4.x; lps[lane][4 * q + 1] = v4.y;
        lps[lane][4 * q + 2] = v4.z; lps[lane][4 * q + 3] = v4.w;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };

  float v[SPL];
  stage(0);
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    const int s = s0 + j;
    v[j] = ((s == 0 || s == 1) && s < SP) ? lps[0][cls[j]] : NEG_INF;
  }
  for (int t = 1; t < len; ++t) {
    if ((t & 63) == 0) stage(t);
    float lcur[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) lcur[j] = lps[t & 63][cls[j]];
    // previous lane's last two states: DPP wave_shr:1 (a VALU move; lane 0 keeps the NEG_INF
    // 'old' operand)
    const float p1 = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(NEG_INF), __float_as_int(v[SPL - 1]),
                                                                0x138, 0xf, 0xf, false));
    const float p2 = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(NEG_INF), __float_as_int(v[SPL - 2]),
                                                                0x138, 0xf, 0xf, false));
    float nv[SPL];
    unsigned w0 = 0, w1 = 0;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      const float a1 = (j >= 1) ? v[j - 1] : p1;
      const float a2r = (j >= 2) ? v[j - 2] : (j == 1 ? p1 : p2);
      const float a2 = ((skip >> j) & 1u) ? a2r : NEG_INF;
      float best = v[j];
      unsigned k = 0;
      if (a1 > best) { best = a1; k = 1; }           // tie rule: stay, then s-1, then s-2
      if (a2 > best) { best = a2; k = 2; }
      nv[j] = best + lcur[j];
      if (j < 16) w0 |= k << (2 * j);
      else w1 |= k << (2 * (j - 16));
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j) v[j] = nv[j];
    if constexpr (W == 1) bp[(size_t)t * 64 + lane] = w0;
    else reinterpret_cast<uint2*>(bp)[(size_t)t * 64 + lane] = make_uint2(w0, w1);
  }

  // end state: 2L, or 2L-1 when strictly better
  float vl = NEG_INF, vp = NEG_INF;
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    if (s0 + j == SP - 1) vl = v[j];
    if (s0 + j == SP - 2) vp = v[j];
  }
  vl = wave_max(vl);
  vp = wave_max(vp);
  int s = (vp > vl) ? SP - 2 : SP - 1;
  const float sc = (vp > vl) ? vp : vl;
  if (__any(nan)) {
    no_path(__builtin_nanf(""));
    return;
  }
  if (!(fabsf(sc) <= 3.402823466e38f)) {            // -inf: no finite path (+inf / NaN out of infinities: reported)
    no_path(sc);
    return;
  }

  // ---- backtrack. The back-pointer rows are this wave's own stores, read back by its other
  // lanes: one workgroup, one CU, one vector L1, so workgroup scope orders them (the stores have
  // completed before the loads issue). An agent-scope fence here adds an L2 write-back and
  // invalidate: 3.7 us per call at the headline shape (profiles/align.md).
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __shared__ unsigned bps[FR][64 * W];
  __shared__ int st[FR + 2];     // st[f+1]: state at frame t_lo+f; st[0] / st[n+1]: its neighbours' (or -1)
  __shared__ float lpv[FR];      // lp of the path's class at frame t_lo+f
  __shared__ int ts_s[LCAP], te_s[LCAP];
  __shared__ float tsc_s[LCAP];
  for (int l = lane; l < Lmax; l += 64) {
    ts_s[l] = -1;
    te_s[l] = -1;
    tsc_s[l] = 0.f;
  }
  int s_above = -1;              // state at frame t_hi+1
  // A chunk's 64 rows travel through registers: all 64 loads are in flight at once (a loop that
  // stores each row to LDS as it arrives waits for memory once per few rows), and the NEXT
  // chunk's loads are issued before this chunk is walked, so the walk hides their latency.
  // Frames past the chunk's top re-read its top row (in bounds, unused).
  typedef typename std::conditional<W == 1, unsigned, uint2>::type row_t;
  row_t rows[FR];
  auto fetch = [&](int hi) {     // rows of frames max(hi-63, 0) .. hi
    const int lo = max(hi - (FR - 1), 0);
    const row_t* src = reinterpret_cast<const row_t*>(bp);
#pragma unroll
    for (int f = 0; f < FR; ++f) rows[f] = src[(size_t)min(lo + f, hi) * 64 + lane];
  };
  fetch(len - 1);
  for (int t_hi = len - 1; t_hi >= 0; t_hi -= FR) {
    const int t_lo = max(t_hi - (FR - 1), 0), n = t_hi - t_lo + 1;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int f = 0; f < FR; ++f) reinterpret_cast<row_t*>(bps[f])[lane] = rows[f];
    if (t_lo > 0) fetch(t_lo - 1);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // the serial walk: every lane walks the same states (LDS broadcast reads)
    int s_lo = s;
    for (int f = n - 1; f >= 0; --f) {
      if (lane == 0) st[f + 1] = s;
      s_lo = s;
      if (t_lo + f > 0) {
        const int ln = s / SPL, j = s - ln * SPL;
        const unsigned wd = (W == 1) ? bps[f][ln] : bps[f][ln * W + (j >> 4)];
        s = max(s - (int)((wd >> (2 * (j & 15))) & 3u), 0);
      }
    }
    if (lane == 0) {
      st[0] = (t_lo > 0) ? s : -1;
      st[n + 1] = s_above;
    }
    s_above = s_lo;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // 64 frames in parallel: class, lp, span ends
    const int t = t_lo + lane;
    int sm = 0;
    if (lane < n) {
      sm = st[lane + 1];
      const int c = align_class(labels, b, Lmax, sm, blank);
      lpv[lane] = lp[(size_t)t * KPAD + min(c, KPAD - 1)];
      path_b[t] = c;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane < n && (sm & 1)) {
      const int sp = st[lane], sn = st[lane + 2];
      const int l = sm >> 1;
      if (sn != sm) te_s[l] = t;
      if (sp != sm) ts_s[l] = t;
      if (lane == 0 || sp != sm) {   // first frame of the label's run inside this chunk: sum the run
        float a = 0.f;
        for (int f = lane; f < n && st[f + 1] == sm; ++f) a += lpv[f];
        tsc_s[l] += a;               // one lane per label and chunk; chunks are a fence apart
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  }
  __builtin_amdgcn_wave_barrier();
  for (int t = len + lane; t < T; t += 64) path_b[t] = -1;
  for (int l = lane; l < Lmax; l += 64) {
    ts_b[l] = ts_s[l];
    te_b[l] = te_s[l];
    tsc_b[l] = tsc_s[l];
  }
  if (lane == 0) score[b] = sc;
}

template <int SPL>
static void launch_align(const int* lens, const int* labels, const int* label_lens, const float* lp_ws, unsigned* bp_ws,
                         int* path, int* tok_start, int* tok_end, float* tok_score, float* score, int T, int N,
                         int Lmax, int blank, hipStream_t st) {
  hipLaunchKernelGGL(ctc_align_kernel<SPL>, dim3(N), dim3(64), 0, st, lens, labels, label_lens, lp_ws, bp_ws, path,
                     tok_start, tok_end, tok_score, score, T, N, Lmax, blank);
}

// States per lane: the smallest instantiation that holds the longest label (the frame loop is
// issue bound on one wave, so every unused state slot costs time); the same set as ctc.hip.
int align_spl(int SPmax) {
  const int need = (SPmax + 63) / 64;
  for (int k : {4, 5, 6, 8, 12, 16, 32}) if (k >= need) return k;
  return -1;
}

}  // namespace

extern "C" {

// workspace bytes: lp [N][T][32] fp32 + back-pointers [N][T][64] words (two words for SPL = 32);
// -1 when the labels do not fit the widest register tile
long long ds2_ctc_align_ws_bytes(int T, int N, int Lmax) {
  const int spl = align_spl(2 * Lmax + 1);
  if (spl < 0) return -1;
  const long long W = spl > 16 ? 2 : 1;
  return (long long)N * T * KPAD * 4 + (long long)N * T * 64 * W * 4;
}

int ds2_ctc_align(const void* em, int em_bf16, int log_probs, const int* lens, const int* labels,
                  const int* label_lens, int* path, int* tok_start, int* tok_end, float* tok_score, float* score,
                  void* ws, int T, int N, int K, int Lmax, int blank, hipStream_t st) {
  if (K > KPAD) return -20;
  const int SPmax = 2 * Lmax + 1;
  if (SPmax > 64 * 32 || Lmax < 1) return -21;      // > 1023 labels per utterance
  if (blank < 0 || blank >= K) return -22;
  if (N <= 0) return 0;
  const int spl = align_spl(SPmax);
  float* lp_ws = static_cast<float*>(ws);
  unsigned* bp_ws = reinterpret_cast<unsigned*>(lp_ws + (size_t)N * T * KPAD);
  const int nw = T * N;
  if (nw > 0) {
    const dim3 g4((nw + 3) / 4);
    if (em_bf16)
      hipLaunchKernelGGL(align_lp_kernel<bf16_t>, g4, dim3(256), 0, st, (const bf16_t*)em, lens, lp_ws, T, N, K,
                         log_probs);
    else
      hipLaunchKernelGGL(align_lp_kernel<float>, g4, dim3(256), 0, st, (const float*)em, lens, lp_ws, T, N, K,
                         log_probs);
  }
#define DS2_ALIGN_CASE(S)                                                                                          \
  case S:                                                                                                          \
    launch_align<S>(lens, labels, label_lens, lp_ws, bp_ws, path, tok_start, tok_end, tok_score, score, T, N, Lmax, \
                    blank, st);                                                                                    \
    break;
  switch (spl) {
    DS2_ALIGN_CASE(4)
    DS2_ALIGN_CASE(5)
    DS2_ALIGN_CASE(6)
    DS2_ALIGN_CASE(8)
    DS2_ALIGN_CASE(12)
    DS2_ALIGN_CASE(16)
    default:
      launch_align<32>(lens, labels, label_lens, lp_ws, bp_ws, path, tok_start, tok_end, tok_score, score, T, N, Lmax,
                       blank, st);
      break;
  }
#undef DS2_ALIGN_CASE
  return (int)hipGetLastError();
}

}  // extern "C"
