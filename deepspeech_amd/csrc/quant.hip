// Per-tensor fp8 (OCP e4m3fn) quantisation of the two operands of a projection GEMM
// (BASELINE config 5, `--fp8`): amax -> scale = amax / 448 -> saturating cast, for the input
// activations AND the weights in two launches, scales left on the device for the fp8 MFMA
// GEMM (csrc/gemm8.hip folds them into its epilogue; no host sync).
//
// The torch-level version (abs, amax, divide, clamp, float round trip, cast, for each
// operand) was ~10 launches and ~0.9 ms per config-5 step (profiles/r1_s3_config5_fp8.md),
// more than the fp8 GEMMs saved.
//   1. amax2_kernel   blocks [0, nb) sweep operand a, [nb, 2nb) operand b (16-B loads),
//                     one partial max per block (no zero-initialised accumulator needed);
//   2. quant2_kernel  every block first reduces the partials of its operand (<= 1024
//                     floats, L2-resident), then casts its slice; block 0 publishes
//                     scales = {amax_a / 448, amax_b / 448 * alpha}.
// Direction-sum form (an fp8 bidirectional layer feeding the next fp8 layer, SURVEY K12 /
// src/custom_ops.py:94-95): operand a is given as its two addends a + a2 (the directions'
// outputs); pass 1 writes the bf16 sum (the next layer's saved input, bitwise torch.add: fp32
// add, one rounding) while it takes the amax, and pass 2 casts the sum. No separate add launch
// and no extra read of the sum.
#include <hip/hip_fp8.h>

#include "common.h"

using namespace ds2;

namespace {

constexpr float FP8_MAX = 448.0f;
constexpr int QT = 256;             // threads per block

__device__ __forceinline__ float block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int i = 1; i < QT / 64; ++i) r = fmaxf(r, sh[i]);
  return r;
}

__global__ __launch_bounds__(QT) void amax2_kernel(const bf16_t* __restrict__ a, long long na,
                                                   const bf16_t* __restrict__ b, long long nb_el, int nb,
                                                   float* __restrict__ part, const bf16_t* __restrict__ a2,
                                                   bf16_t* __restrict__ asum) {
  __shared__ float sh[QT / 64];
  const bool second = blockIdx.x >= (unsigned)nb;
  const bf16_t* x = second ? b : a;
  const long long n = second ? nb_el : na;
  const int blk = second ? blockIdx.x - nb : blockIdx.x;
  float m = 0.f;
  const long long n8 = n / 8;
  if (!second && a2 != nullptr) {
    // direction-sum form: s = bf16(a + a2) stored, amax taken of the stored (rounded) sum
    for (long long i = (long long)blk * QT + threadIdx.x; i < n8; i += (long long)nb * QT) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(a + i * 8);
      const bf16x8 w = *reinterpret_cast<const bf16x8*>(a2 + i * 8);
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bf16_t r = f2bf(__fadd_rn(bf2f((bf16_t)v[j]), bf2f((bf16_t)w[j])));
        o[j] = r;
        m = fmaxf(m, fabsf(bf2f(r)));
      }
      *reinterpret_cast<bf16x8*>(asum + i * 8) = o;
    }
    for (long long i = n8 * 8 + (long long)blk * QT + threadIdx.x; i < n; i += (long long)nb * QT) {
      const bf16_t r = f2bf(__fadd_rn(bf2f(a[i]), bf2f(a2[i])));
      asum[i] = r;
      m = fmaxf(m, fabsf(bf2f(r)));
    }
    m = block_max(m, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
    return;
  }
  for (long long i = (long long)blk * QT + threadIdx.x; i < n8; i += (long long)nb * QT) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(bf2f((bf16_t)v[j])));
  }
  for (long long i = n8 * 8 + (long long)blk * QT + threadIdx.x; i < n; i += (long long)nb * QT)
    m = fmaxf(m, fabsf(bf2f(x[i])));
  m = block_max(m, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// Saturating cast. fmaxf / fminf drop a NaN operand (the clamp alone would store NaN as -448, a
// finite value that dequantises to -amax), so the NaN byte is selected back in afterwards: a NaN
// element, or inf * 0 under an infinite amax, reaches the GEMM and the non-finite watch as NaN.
__device__ __forceinline__ unsigned char to_e4m3(float f) {
  const __hip_fp8_e4m3 q(fminf(fmaxf(f, -FP8_MAX), FP8_MAX));
  const unsigned char b = *reinterpret_cast<const unsigned char*>(&q);
  return f != f ? (unsigned char)0x7F : b;
}

// Casts [rows][K] bf16 to [rows][Kp] e4m3 (Kp >= K, K % 8 == 0): the padding columns are
// written as zeros, so a GEMM can run over Kp (gemm8's fp8 k-tiles are 128 deep).
__global__ __launch_bounds__(QT) void quant2_kernel(const bf16_t* __restrict__ a, long long rows_a,
                                                    const bf16_t* __restrict__ b, long long rows_b, int K, int Kp,
                                                    int nb, const float* __restrict__ part, float alpha,
                                                    unsigned char* __restrict__ a8, unsigned char* __restrict__ b8,
                                                    float* __restrict__ scales) {
  __shared__ float sh[QT / 64];
  const bool second = blockIdx.x >= (unsigned)nb;
  // amax of this block's operand from the partials (and of the other for block 0's scales)
  float ma = 0.f, mb = 0.f;
  for (int i = threadIdx.x; i < nb; i += QT) {
    ma = fmaxf(ma, part[i]);
    mb = fmaxf(mb, part[nb + i]);
  }
  ma = block_max(ma, sh);
  mb = block_max(mb, sh);
  const float sa = fmaxf(ma / FP8_MAX, 1e-12f), sb = fmaxf(mb / FP8_MAX, 1e-12f);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scales[0] = sa;
    scales[1] = sb * alpha;
  }
  const bf16_t* x = second ? b : a;
  unsigned char* y = second ? b8 : a8;
  const long long rows = second ? rows_b : rows_a;
  const float inv = 1.f / (second ? sb : sa);
  const int blk = second ? blockIdx.x - nb : blockIdx.x;
  const int cpr = Kp / 8;                      // 8-element output chunks per row
  const long long n8 = rows * cpr;
  for (long long i = (long long)blk * QT + threadIdx.x; i < n8; i += (long long)nb * QT) {
    const long long r = i / cpr;
    const int c = (int)(i - r * cpr);
    unsigned lo = 0, hi = 0;
    if (8 * c < K) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + r * K + 8 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo |= (unsigned)to_e4m3(bf2f((bf16_t)v[j]) * inv) << (8 * j);
        hi |= (unsigned)to_e4m3(bf2f((bf16_t)v[4 + j]) * inv) << (8 * j);
      }
    }
    *reinterpret_cast<uint2*>(y + i * 8) = make_uint2(lo, hi);
  }
}

}  // namespace

extern "C" {

int ds2_fp8_quant_blocks(long long na, long long nb_el) {
  const long long m = na > nb_el ? na : nb_el;
  long long nb = (m / 8 + QT - 1) / QT;
  if (nb > 1024) nb = 1024;
  return (int)(nb < 1 ? 1 : nb);
}

// a [rows_a][K], b [rows_b][K]: bf16 (16-B aligned, K % 8 == 0); a8 [rows_a][Kp], b8
// [rows_b][Kp]: fp8 e4m3fn outputs, Kp % 8 == 0, columns >= K zero; part: 2*nb floats;
// scales: {amax_a / 448, amax_b / 448 * alpha}. a2 / asum (both or neither, [rows_a][K]): the
// operand is a + a2, written to asum (bf16) and quantised from there.
int ds2_fp8_quant2(const void* a, long long rows_a, const void* b, long long rows_b, int K, int Kp, float alpha,
                   void* a8, void* b8, float* part, float* scales, const void* a2, void* asum, hipStream_t st) {
  if (K % 8 || Kp % 8 || Kp < K || ((a2 == nullptr) != (asum == nullptr))) return (int)hipErrorInvalidValue;
  const long long na = rows_a * K, nb_el = rows_b * K;
  const int nb = ds2_fp8_quant_blocks(rows_a * Kp, rows_b * Kp);
  hipLaunchKernelGGL(amax2_kernel, dim3(2 * nb), dim3(QT), 0, st, (const bf16_t*)a, na, (const bf16_t*)b, nb_el, nb,
                     part, (const bf16_t*)a2, (bf16_t*)asum);
  const bf16_t* qa = (const bf16_t*)(asum != nullptr ? asum : a);
  hipLaunchKernelGGL(quant2_kernel, dim3(2 * nb), dim3(QT), 0, st, qa, rows_a, (const bf16_t*)b, rows_b,
                     K, Kp, nb, (const float*)part, alpha, (unsigned char*)a8, (unsigned char*)b8, scales);
  return (int)hipGetLastError();
}

}  // extern "C"
