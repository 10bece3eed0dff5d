// One workgroup's share of a polyphase resampling launch, kept once for csrc/resample.hip (one
// filter per launch) and csrc/speed.hip (one filter per row): the tile geometry, the LDS layout,
// the staging of a coefficient table and of a tile's input span, and the ascending-k fma chain
// that is the definition (ops/reference.py resample_ref).
//
// LDS of a workgroup: hs [L][K + 1] (odd row stride: neighbouring outputs' phases differ by
// M mod L, and an odd stride sends distinct phases mod 32 to distinct banks), then, from the next
// 16-byte boundary, xs [span]: a tile's input samples as fp32, staged once by 16-byte loads where
// the row is 16-byte aligned (then from a 16-byte boundary of the row: the span may start up to
// ALIGN_PAD - 1 samples early). Samples outside [0, len) are staged as +0 by selection, so nothing
// at or past a row's length (garbage, NaN) reaches an output. A lane owns outputs tid and
// tid + THREADS of a tile: neighbouring lanes read neighbouring (stride M / L) words of the span
// and each store instruction of a wave covers 256 contiguous bytes of the output row.
#pragma once
#include "common.h"

namespace ds2 {
namespace rs {

constexpr int THREADS = 512;
constexpr int PER_LANE = 2;
constexpr int TILE = THREADS * PER_LANE;         // outputs per tile
constexpr int MAX_TABLE = 24576;                 // L * K words
constexpr int MAX_K = 320;
constexpr int ALIGN_PAD = 8;                     // a staged span may start up to 7 samples early
constexpr int MAX_LDS = 160 * 1024;

// floats of LDS that hold any tile's input span
__host__ __device__ inline int span_words(int L, int M, int K) {
  const long long s = (long long)(TILE - 1) * M / L + 1 + K + ALIGN_PAD;
  return (int)((s + 3) & ~3LL);
}

// floats of LDS in front of the span: the table, up to the next 16-byte boundary
__host__ __device__ inline int table_words(int L, int K) { return (L * (K + 1) + 3) & ~3; }

// 1 when (L, M, K) lies inside the contract of the kernels built on this file
inline int supported(int L, int M, int K) {
  if (L < 1 || M < 1 || K < 2 || (K & 1) || K > MAX_K) return 0;
  if ((long long)L * K > MAX_TABLE) return 0;
  const long long bytes = (((long long)L * (K + 1) + 3) & ~3LL) * 4 + (long long)span_words(L, M, K) * 4;
  return bytes <= MAX_LDS;
}

// one filter and where output 0 of the launch sits on it: output j has t = ph0 + j * M,
// q = t / L, phase t % L and reads x[in_off + q + k], k < K
struct Filter {
  const float* h;          // [L, K] in global memory
  int L, M, K;
  int in_off, ph0;
  int span;                // span_words(L, M, K)
};

// one row of the launch: cnt outputs are computed, columns [cnt, n_out) are zeros
template <typename IN>
struct Row {
  const IN* x;             // the row's samples; x[g] is read only for 0 <= g < len <= S
  bool vec;                // x is 16-byte aligned
  int S, len;
  float* out;
  int n_out, cnt;
};

template <typename IN>
__device__ __forceinline__ float to_f32(IN v) { return (float)v; }   // int16 -> fp32 is exact

// a tile at or past the row's count: zeros
__device__ __forceinline__ void zero_tile(float* out, int j0, int n_out) {
#pragma unroll
  for (int r = 0; r < PER_LANE; ++r) {
    const int j = j0 + (int)threadIdx.x + r * THREADS;
    if (j < n_out) out[j] = 0.f;
  }
}

// h [L, K] -> hs [L][K + 1]; the barrier in front of the first tile's span makes it visible
__device__ __forceinline__ void stage_table(float* hs, const float* h, int L, int K) {
  const int ld = K + 1;
  for (int i = threadIdx.x; i < L * K; i += THREADS) {
    const int ph = i / K;
    hs[ph * ld + (i - ph * K)] = h[i];
  }
}

// Outputs [j0, j0 + TILE) of a row, j0 < cnt. UNI: L == 1, one phase: every lane multiplies by
// the same h[k], which then comes through the scalar cache into an SGPR instead of through an LDS
// read per lane (hs is not read).
template <typename IN, bool UNI>
__device__ __forceinline__ void tile(const Filter& f, const Row<IN>& w, const float* hs, float* xs, int j0) {
  constexpr int V = 16 / (int)sizeof(IN);             // samples per 16-byte load
  const int tid = threadIdx.x;
  const int L = f.L, M = f.M, K = f.K, ld = K + 1;
  // the tile's span: taps of outputs j0 .. jl, global samples [g0, g0 + need)
  const int jl = min(j0 + TILE, w.cnt) - 1;
  const long long q0 = ((long long)f.ph0 + (long long)j0 * M) / L;
  const long long ql = ((long long)f.ph0 + (long long)jl * M) / L;
  long long g0 = (long long)f.in_off + q0;
  const int shift = w.vec ? (int)(((g0 % V) + V) % V) : 0;   // stage from a 16-byte boundary
  g0 -= shift;
  const int need = min((int)(ql - q0) + K + shift, f.span);  // the span holds any tile
  __syncthreads();                                   // the previous tile's reads of xs are done
  if (w.vec) {
    for (int v = tid; v * V < need; v += THREADS) {
      const long long g = g0 + (long long)v * V;
      float e32[V];
      if (g >= 0 && g + V <= w.S) {
        const i32x4 word = *reinterpret_cast<const i32x4*>(w.x + g);
        IN raw[V];
        __builtin_memcpy(raw, &word, 16);
#pragma unroll
        for (int e = 0; e < V; ++e) e32[e] = g + e < w.len ? to_f32(raw[e]) : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const long long ge = g + e;
          e32[e] = 0.f;
          if (ge >= 0 && ge < w.len) e32[e] = to_f32(w.x[ge]);
        }
      }
#pragma unroll
      for (int e = 0; e < V; e += 4) {
        if (v * V + e < f.span)                      // span is a multiple of 4
          *reinterpret_cast<f32x4*>(xs + v * V + e) = f32x4{e32[e], e32[e + 1], e32[e + 2], e32[e + 3]};
      }
    }
  } else {
    for (int i = tid; i < need; i += THREADS) {
      const long long g = g0 + i;
      float v = 0.f;
      if (g >= 0 && g < w.len) v = to_f32(w.x[g]);
      xs[i] = v;
    }
  }
  __syncthreads();

  const float* hp[PER_LANE];
  const float* xp[PER_LANE];
  float acc[PER_LANE];
#pragma unroll
  for (int r = 0; r < PER_LANE; ++r) {
    const int j = min(j0 + tid + r * THREADS, jl);     // lanes past the count recompute jl
    const long long t = (long long)f.ph0 + (long long)j * M;   // 64 bits, once per output
    const long long q = t / L;
    hp[r] = hs + (int)(t - q * L) * ld;
    xp[r] = xs + (int)(q - q0) + shift;
    acc[r] = 0.f;
  }
  if (UNI) {
    const float* __restrict__ hu = f.h;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
      const float hk = hu[k];
#pragma unroll
      for (int r = 0; r < PER_LANE; ++r) acc[r] = __fmaf_rn(hk, xp[r][k], acc[r]);
    }
  } else {
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int r = 0; r < PER_LANE; ++r) acc[r] = __fmaf_rn(hp[r][k], xp[r][k], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < PER_LANE; ++r) {
    const int j = j0 + tid + r * THREADS;
    if (j < w.n_out) w.out[j] = j < w.cnt ? acc[r] : 0.f;
  }
}

}  // namespace rs
}  // namespace ds2
