// Polyphase windowed-sinc resampling of PCM rows (ops/resample.py; oracle: ops/reference.py
// resample_ref). Rates in -> out reduce to L = out / gcd, M = in / gcd; output j of a launch has
// t = ph0 + j * M (64 bits, formed once), q = t / L, ph = t % L and
//   y[j] = sum_{k = 0 .. K-1} h[ph, k] * x[in_off + q + k]
// as one chain of fp32 fma in ascending k from +0, with x outside [0, len) read as +0 by
// selection while the tile is staged, so nothing past a row's length (garbage, NaN) reaches an
// output. in_off is the buffer index of tap 0 of output 0 (negative: the left zero padding) and
// ph0 the phase of output 0: a whole call passes (-(K/2 - 1), 0), a stream push its buffer-
// relative values, so every output is the same chain over the same values however the signal
// was chunked.
//
// One workgroup per (row, grid.x-strided tiles of TILE_OUT outputs). The coefficient table sits in
// LDS for the workgroup's whole life with an odd row stride K + 1: neighbouring outputs' phases
// differ by M mod L, and an odd stride sends distinct phases (mod 32) to distinct banks; with
// L = 1 every lane multiplies by the same word, which the UNI instantiation reads through the
// scalar cache instead (no table in LDS, half the LDS reads). Each tile's input span (at most
// (TILE_OUT - 1) * M / L + K + 1 samples) is staged once, as fp32, by 16-byte loads where the row
// is 16-byte aligned. A lane owns outputs tid and tid + 512: neighbouring lanes read
// neighbouring (stride M / L) words of the span, and each store instruction of a wave covers 256
// contiguous bytes of the row whatever its alignment (an [B, N] fp32 row starts on a 16-byte
// boundary only when N % 4 == 0, so 16-byte stores would need a second path). Columns at or
// past a row's count are written as zeros and out_lens[b] by the same launch. No atomics, no
// MFMA (the ascending-k chain is the definition), nothing read back: the launch can be captured
// in a graph.
#include "common.h"

namespace {

constexpr int RS_THREADS = 512;
constexpr int RS_PER_LANE = 2;
constexpr int RS_TILE = RS_THREADS * RS_PER_LANE;   // ds2_resample_tile()
constexpr int RS_MAX_TABLE = 24576;                 // L * K words
constexpr int RS_MAX_K = 320;
constexpr int RS_ALIGN_PAD = 8;                     // a staged span may start up to 7 samples early

struct RsArgs {
  const void* x;
  long long row_stride;     // samples between rows
  int S, B;                 // row width of the buffer, rows
  const int* lens;          // [B] valid samples of the buffer, or null (= S)
  const float* h;           // [L, K]
  int L, M, K;
  int in_off, ph0;
  int n_out, to_end;        // out is [B, n_out]; to_end: a row's count stops where its samples do
  int span;                 // floats of LDS for a tile's input span
  float* out;
  int* out_lens;            // [B]
};

template <typename IN>
__device__ __forceinline__ float to_f32(IN v) { return (float)v; }   // int16 -> fp32 is exact

// UNI: L == 1, one phase: every lane multiplies by the same h[k], which then comes through the
// scalar cache into an SGPR instead of through an LDS read per lane
template <typename IN, bool UNI>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  constexpr int V = 16 / (int)sizeof(IN);             // samples per 16-byte load
  const int tid = threadIdx.x, b = blockIdx.y;
  const int L = a.L, M = a.M, K = a.K, ld = K + 1;
  float* hs = rs_lds;                                  // [L][K + 1]
  float* xs = rs_lds + ((L * ld + 3) & ~3);            // [span], 16-byte aligned

  int len = a.lens ? a.lens[b] : a.S;
  len = max(0, min(len, a.S));
  // outputs of this row: j counts while the centre sample in_off + K/2 - 1 + q_j is a valid one
  int cnt = a.n_out;
  if (a.to_end) {
    const long long num = ((long long)len - ((long long)a.in_off + K / 2 - 1)) * L - a.ph0;
    const long long c = num <= 0 ? 0 : (num + M - 1) / M;
    cnt = (int)min((long long)a.n_out, c);
  }
  if (blockIdx.x == 0 && tid == 0) a.out_lens[b] = cnt;

  float* orow = a.out + (long long)b * a.n_out;
  const IN* xrow = reinterpret_cast<const IN*>(a.x) + (long long)b * a.row_stride;
  const bool vec = (reinterpret_cast<uintptr_t>(xrow) & 15) == 0;
  const int ntiles = (a.n_out + RS_TILE - 1) / RS_TILE;
  bool table = false;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j0 = tile * RS_TILE;
    if (j0 >= cnt) {                                   // padding only
#pragma unroll
      for (int r = 0; r < RS_PER_LANE; ++r) {
        const int j = j0 + tid + r * RS_THREADS;
        if (j < a.n_out) orow[j] = 0.f;
      }
      continue;
    }
    if (!UNI && !table) {
      for (int i = tid; i < L * K; i += RS_THREADS) {
        const int ph = i / K;
        hs[ph * ld + (i - ph * K)] = a.h[i];
      }
      table = true;
    }
    // the tile's span: taps of outputs j0 .. jl, global samples [g0, g0 + need)
    const int jl = min(j0 + RS_TILE, cnt) - 1;
    const long long q0 = ((long long)a.ph0 + (long long)j0 * M) / L;
    const long long ql = ((long long)a.ph0 + (long long)jl * M) / L;
    long long g0 = (long long)a.in_off + q0;
    const int shift = vec ? (int)(((g0 % V) + V) % V) : 0;   // stage from a 16-byte boundary
    g0 -= shift;
    const int need = min((int)(ql - q0) + K + shift, a.span);  // host sized span for any tile
    __syncthreads();                                   // the previous tile's reads of xs are done
    if (vec) {
      for (int v = tid; v * V < need; v += RS_THREADS) {
        const long long g = g0 + (long long)v * V;
        float f[V];
        if (g >= 0 && g + V <= a.S) {
          const ds2::i32x4 w = *reinterpret_cast<const ds2::i32x4*>(xrow + g);
          IN raw[V];
          __builtin_memcpy(raw, &w, 16);
#pragma unroll
          for (int e = 0; e < V; ++e) f[e] = g + e < len ? to_f32(raw[e]) : 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const long long ge = g + e;
            f[e] = 0.f;
            if (ge >= 0 && ge < len) f[e] = to_f32(xrow[ge]);
          }
        }
#pragma unroll
        for (int e = 0; e < V; e += 4) {
          if (v * V + e < a.span)                      // span is a multiple of 4
            *reinterpret_cast<ds2::f32x4*>(xs + v * V + e) = ds2::f32x4{f[e], f[e + 1], f[e + 2], f[e + 3]};
        }
      }
    } else {
      for (int i = tid; i < need; i += RS_THREADS) {
        const long long g = g0 + i;
        float f = 0.f;
        if (g >= 0 && g < len) f = to_f32(xrow[g]);
        xs[i] = f;
      }
    }
    __syncthreads();

    const float* hp[RS_PER_LANE];
    const float* xp[RS_PER_LANE];
    float acc[RS_PER_LANE];
#pragma unroll
    for (int r = 0; r < RS_PER_LANE; ++r) {
      const int j = min(j0 + tid + r * RS_THREADS, jl);     // lanes past the count recompute jl
      const long long t = (long long)a.ph0 + (long long)j * M;   // 64 bits, once per output
      const long long q = t / L;
      hp[r] = hs + (int)(t - q * L) * ld;
      xp[r] = xs + (int)(q - q0) + shift;
      acc[r] = 0.f;
    }
    if (UNI) {
      const float* __restrict__ hu = a.h;
#pragma unroll 8
      for (int k = 0; k < K; ++k) {
        const float hk = hu[k];
#pragma unroll
        for (int r = 0; r < RS_PER_LANE; ++r) acc[r] = __fmaf_rn(hk, xp[r][k], acc[r]);
      }
    } else {
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int r = 0; r < RS_PER_LANE; ++r) acc[r] = __fmaf_rn(hp[r][k], xp[r][k], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < RS_PER_LANE; ++r) {
      const int j = j0 + tid + r * RS_THREADS;
      if (j < a.n_out) orow[j] = j < cnt ? acc[r] : 0.f;
    }
  }
}

int rs_span(int L, int M, int K) {
  const long long s = (long long)(RS_TILE - 1) * M / L + 1 + K + RS_ALIGN_PAD;
  return (int)((s + 3) & ~3LL);
}

}  // namespace

extern "C" int ds2_resample_tile() { return RS_TILE; }

// 1 when (L, M, K) lies inside the kernel's contract
extern "C" int ds2_resample_supported(int L, int M, int K) {
  if (L < 1 || M < 1 || K < 2 || (K & 1) || K > RS_MAX_K) return 0;
  if ((long long)L * K > RS_MAX_TABLE) return 0;
  const long long bytes = (((long long)L * (K + 1) + 3) & ~3LL) * 4 + (long long)rs_span(L, M, K) * 4;
  return bytes <= 160 * 1024;
}

// x [B, S] fp32 / int16 rows row_stride samples apart, h fp32 [L, K], out fp32 [B, n_out],
// out_lens int32 [B]. -90: shape outside the contract, -91: in_off / ph0 outside their ranges.
extern "C" int ds2_resample(const void* x, int in_i16, long long row_stride, int S, int B, const int* lens,
                            const float* h, int L, int M, int K, int in_off, int ph0, int n_out, int to_end,
                            float* out, int* out_lens, hipStream_t st) {
  if (B <= 0) return 0;
  if (!ds2_resample_supported(L, M, K) || B > 65535 || S < 0 || n_out < 0 || row_stride < S) return -90;
  if (ph0 < 0 || ph0 >= L || in_off < -(K / 2 - 1) || (long long)n_out * M / L + (long long)in_off > (1LL << 31))
    return -91;
  RsArgs a{};
  a.x = x; a.row_stride = row_stride; a.S = S; a.B = B; a.lens = lens; a.h = h;
  a.L = L; a.M = M; a.K = K; a.in_off = in_off; a.ph0 = ph0; a.n_out = n_out; a.to_end = to_end;
  a.span = rs_span(L, M, K);
  a.out = out; a.out_lens = out_lens;
  const int lds = (((L * (K + 1) + 3) & ~3) + a.span) * 4;
  static bool attr = false;
  if (!attr) {
    for (const void* kern : {(const void*)resample_kernel<float, false>, (const void*)resample_kernel<short, false>,
                             (const void*)resample_kernel<float, true>, (const void*)resample_kernel<short, true>})
      DS2_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  // a workgroup keeps its table across the tiles it walks: about 2048 workgroups per launch
  const int ntiles = (n_out + RS_TILE - 1) / RS_TILE;
  const int gx = max(1, min(ntiles, (2048 + B - 1) / B));
  const bool uni = L == 1;
  if (uni && in_i16) hipLaunchKernelGGL((resample_kernel<short, true>), dim3(gx, B), dim3(RS_THREADS), lds, st, a);
  else if (uni) hipLaunchKernelGGL((resample_kernel<float, true>), dim3(gx, B), dim3(RS_THREADS), lds, st, a);
  else if (in_i16) hipLaunchKernelGGL((resample_kernel<short, false>), dim3(gx, B), dim3(RS_THREADS), lds, st, a);
  else hipLaunchKernelGGL((resample_kernel<float, false>), dim3(gx, B), dim3(RS_THREADS), lds, st, a);
  return (int)hipGetLastError();
}
