// Speed perturbation of training waveforms (ops/speed.py; definition: ops/reference.py
// speed_plan_ref, speed_ref): every utterance of a batch is resampled by its own ratio, drawn per
// (seed, step, global utterance index) from a policy of V <= 8 distinct integer percents, in one
// launch and with nothing read back. Variant p != 100 is the polyphase Kaiser-sinc of
// csrc/resample.hip for the rates p -> 100: L = 100 / gcd, M = p / gcd, n_out = ceil(n L / M) and
//   y[j] = sum_{k = 0 .. K-1} h_p[j M % L, k] * x[j M / L - (K/2 - 1) + k]
// as one chain of fp32 fma in ascending k from +0, x outside [0, n) read as +0 by selection: the
// whole-call launch of the resampling kernel on that row alone, bit for bit, since both run the
// staging and the chain of resample_tile.h. p == 100 is a bit copy (never the L = M = 1 filter,
// which would low-pass the signal).
//
// speed_plan_kernel: one lane per utterance, one Philox4x32-10 block with key seed and counter
// (1, first_utt + b, step_lo, 0x40000000 | step_hi & 0x3fffffff): the noise plan's stream
// (csrc/waveaug.hip) with first word 1, so the two never share a block. v = mulhi(x0, V),
// cand = ceil(n L_v / M_v) (n for 100 %); the row is (pct_v, cand), or (100, n) by selection when
// n == 0, cand < min_out[b] or (max_out > 0 and) cand > max_out. Integers only.
//
// speed_apply_kernel: one workgroup per (row, grid.x-strided tiles of 1024 outputs). It reads its
// row's plan, finds the percent among the policy's records (passed by value: they sit in the
// kernel's argument block and come through the scalar cache) and stages only that variant's
// table in LDS, once, in front of its first tile; the launcher sizes the LDS for the policy's
// largest variant. A 100 % row takes a copy path with no table and no chain (8-byte loads where
// the row allows); tiles at or past the row's count are zeros; out_lens[b] comes from the same
// launch. Plan words come from device memory the launcher cannot see: a percent that is not in
// the policy copies, a count is clamped into [0, n_out] (a copy's also to n), and every read of x
// is selected by the row's length, so a damaged word can change values but never reach outside a
// buffer. No atomics, no MFMA, graph-capturable.
#include "philox.h"
#include "resample_tile.h"

using namespace ds2;

namespace {

constexpr int SP_MAX_V = 8, SP_HOP = 160;
constexpr int SP_MAX_B = 65535, SP_MAX_S = (1 << 30) - 1;

typedef __attribute__((ext_vector_type(2))) float f32x2;

struct SpArgs {
  const void* x;            // [B, S] contiguous
  int S, B;
  const int* lens;          // [B] or null (= S)
  const int* plan;          // [B, 2] = (pct, n_out)
  const float* h;           // the variants' tables back to back
  DS2SpeedTable t;
  float* out;               // [B, n_out]
  int n_out;
  int* out_lens;            // [B]
};

__device__ __forceinline__ int clamp_len(const int* lens, int b, int S) {
  return lens != nullptr ? min(max(lens[b], 0), S) : S;
}

__global__ __launch_bounds__(64) void speed_plan_kernel(const int* __restrict__ lens, const int* __restrict__ min_out,
                                                        int* __restrict__ plan, int B, int S, int max_out,
                                                        DS2SpeedTable t, unsigned seed_lo, unsigned seed_hi,
                                                        unsigned step_lo, unsigned step_hi, unsigned first_utt) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = clamp_len(lens, b, S);
  unsigned x[4];
  philox4x32_10(1u, first_utt + (unsigned)b, step_lo, 0x40000000u | (step_hi & 0x3fffffffu), seed_lo, seed_hi, x);
  const int v = (int)__umulhi(x[0], (unsigned)t.V);
  int pct = 100, L = 1, M = 1;
#pragma unroll
  for (int u = 0; u < SP_MAX_V; ++u) {               // selection: no indexed copy of the records
    if (u == v) pct = t.pct[u], L = t.L[u], M = t.M[u];
  }
  const long long cand = pct == 100 ? (long long)n : ((long long)n * L + M - 1) / M;
  const long long lo = min_out != nullptr ? (long long)min_out[b] : 0;
  const bool back = n == 0 || cand < lo || (max_out > 0 && cand > (long long)max_out);
  plan[2 * (long long)b] = back ? 100 : pct;
  plan[2 * (long long)b + 1] = back ? n : (int)cand;
}

// outputs [j0, j0 + TILE) of a 100 % row, j0 < cnt <= len: a lane owns outputs j0 + 2 tid and the
// next one (an 8-byte store where both rows are aligned)
template <typename IN>
__device__ __forceinline__ void copy_tile(const rs::Row<IN>& w, bool out_vec, int j0) {
  struct alignas(2 * sizeof(IN)) In2 {
    IN v[2];
  };
  const int j = j0 + 2 * (int)threadIdx.x;
  if (w.vec && out_vec && j + 1 < w.S && j + 1 < w.n_out) {
    const In2 p = *reinterpret_cast<const In2*>(w.x + j);          // inside the buffer; selected below
    *reinterpret_cast<f32x2*>(w.out + j) =
        f32x2{j < w.cnt ? rs::to_f32(p.v[0]) : 0.f, j + 1 < w.cnt ? rs::to_f32(p.v[1]) : 0.f};
  } else {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int je = j + e;
      if (je < w.n_out) w.out[je] = je < w.cnt ? rs::to_f32(w.x[je]) : 0.f;
    }
  }
}

template <typename IN>
__global__ __launch_bounds__(rs::THREADS) void speed_apply_kernel(SpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sp_lds[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a.lens, b, a.S));
  const int pct = __builtin_amdgcn_readfirstlane(a.plan[2 * (long long)b]);
  int cnt = __builtin_amdgcn_readfirstlane(min(max(a.plan[2 * (long long)b + 1], 0), a.n_out));

  int L = 1, M = 1, K = 0, off = 0;
  bool copy = true;
#pragma unroll
  for (int v = 0; v < SP_MAX_V; ++v) {
    if (v < a.t.V && a.t.pct[v] == pct && pct != 100) L = a.t.L[v], M = a.t.M[v], K = a.t.K[v], off = a.t.off[v], copy = false;
  }
  if (copy) cnt = min(cnt, len);
  if (blockIdx.x == 0 && tid == 0) a.out_lens[b] = cnt;

  const IN* xrow = reinterpret_cast<const IN*>(a.x) + (long long)b * a.S;
  float* orow = a.out + (long long)b * a.n_out;
  const rs::Filter f{a.h + off, L, M, K, -(K / 2 - 1), 0, rs::span_words(L, M, K)};
  const rs::Row<IN> w{xrow, (reinterpret_cast<uintptr_t>(xrow) & 15) == 0, a.S, len, orow, a.n_out, cnt};
  const bool out_vec = (reinterpret_cast<uintptr_t>(orow) & 7) == 0;
  float* hs = sp_lds;                                  // [L][K + 1] of this row's variant
  float* xs = sp_lds + rs::table_words(L, K);          // [span], 16-byte aligned
  const int ntiles = (a.n_out + rs::TILE - 1) / rs::TILE;
  bool table = false;

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int j0 = t * rs::TILE;
    if (j0 >= cnt) {                                   // padding only
      rs::zero_tile(orow, j0, a.n_out);
    } else if (copy) {
      copy_tile<IN>(w, out_vec, j0);
    } else {
      if (!table) {
        rs::stage_table(hs, f.h, L, K);
        table = true;
      }
      rs::tile<IN, false>(f, w, hs, xs, j0);
    }
  }
}

// the records of a policy are sane and their tables lie inside h[0, h_words)
bool table_ok(const DS2SpeedTable* t, long long h_words) {
  if (t == nullptr || t->V < 1 || t->V > SP_MAX_V) return false;
  for (int v = 0; v < t->V; ++v) {
    const int p = t->pct[v];
    if (p < 50 || p > 200) return false;
    for (int u = 0; u < v; ++u)
      if (t->pct[u] == p) return false;
    if (p == 100) {
      if (t->L[v] != 1 || t->M[v] != 1 || t->K[v] != 0 || t->off[v] != 0) return false;
      continue;
    }
    const int L = t->L[v], M = t->M[v], K = t->K[v], off = t->off[v];
    if (!rs::supported(L, M, K) || (long long)L * p != (long long)M * 100) return false;
    if (off < 0 || (off & 3) || (long long)off + (long long)L * K > h_words) return false;
  }
  return true;
}

int lds_bytes(const DS2SpeedTable* t) {
  int words = 0;
  for (int v = 0; v < t->V; ++v)
    if (t->pct[v] != 100) words = max(words, rs::table_words(t->L[v], t->K[v]) + rs::span_words(t->L[v], t->M[v], t->K[v]));
  return words * 4;
}

}  // namespace

extern "C" int ds2_speed_tile() { return rs::TILE; }

// 1 when the policy lies inside the kernels' contract (160 KB of LDS, K <= 320 per variant)
extern "C" int ds2_speed_supported(const DS2SpeedTable* t, long long h_words) {
  return table_ok(t, h_words) && lds_bytes(t) <= rs::MAX_LDS;
}

// the output width that holds any row of S samples under any variant: a multiple of one hop
extern "C" long long ds2_speed_out_width(const DS2SpeedTable* t, long long S) {
  long long w = S;
  for (int v = 0; v < t->V; ++v)
    if (t->pct[v] != 100) w = max(w, (S * t->L[v] + t->M[v] - 1) / t->M[v]);
  return (w + SP_HOP - 1) / SP_HOP * SP_HOP;
}

extern "C" int ds2_speed_plan(const int* lens, const int* min_out, int* plan, int B, int S, int max_out,
                              const DS2SpeedTable* t, unsigned seed_lo, unsigned seed_hi, unsigned step_lo,
                              unsigned step_hi, unsigned first_utt, hipStream_t st) {
  if (B < 1 || S < 1 || S > SP_MAX_S || max_out < 0) return -130;
  if (!table_ok(t, 1LL << 40)) return -131;
  ds2_launch(speed_plan_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, lens, min_out, plan, B, S, max_out, *t,
             seed_lo, seed_hi, step_lo, step_hi, first_utt);
  return (int)hipGetLastError();
}

extern "C" int ds2_speed_apply(const void* x, int in_i16, int B, int S, const int* lens, const int* plan,
                               const float* h, long long h_words, const DS2SpeedTable* t, float* out, int n_out,
                               int tight, int* out_lens, hipStream_t st) {
  if (B < 1 || B > SP_MAX_B || S < 1 || S > SP_MAX_S || n_out < 1 || n_out > 0x7fffffff - rs::TILE) return -130;
  if (!ds2_speed_supported(t, h_words)) return -131;
  if (!tight && (long long)n_out < ds2_speed_out_width(t, S)) return -132;
  SpArgs a{};
  a.x = x; a.S = S; a.B = B; a.lens = lens; a.plan = plan; a.h = h; a.t = *t;
  a.out = out; a.n_out = n_out; a.out_lens = out_lens;
  static bool attr = false;
  if (!attr) {
    for (const void* kern : {(const void*)speed_apply_kernel<float>, (const void*)speed_apply_kernel<short>})
      DS2_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, rs::MAX_LDS));
    attr = true;
  }
  // a workgroup keeps its table across the tiles it walks: about 2048 workgroups per launch
  const int ntiles = (n_out + rs::TILE - 1) / rs::TILE;
  const dim3 grid((unsigned)max(1, min(ntiles, (2048 + B - 1) / B)), (unsigned)B);
  const unsigned lds = (unsigned)lds_bytes(t);
  if (in_i16) ds2_launch(speed_apply_kernel<short>, grid, dim3(rs::THREADS), lds, st, a);
  else ds2_launch(speed_apply_kernel<float>, grid, dim3(rs::THREADS), lds, st, a);
  return (int)hipGetLastError();
}
