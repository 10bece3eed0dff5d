// Additive noise at a random signal-to-noise ratio on the waveform (the Deep Speech 2 recipe's
// augmentation; torchaudio.functional.add_noise's definition over the whole utterance).
//
//   x        fp32 or int16 [B, S] contiguous, 16-byte aligned, S % 8 == 0 (so rows are 16-byte
//            multiples for both dtypes), 1 <= B <= 65535, 8 <= S < 2^30; int16 converts exactly
//   lens     int32 [B] or null; n = clamp(lens[b], 0, S) (null: S)
//   bank     data fp32 [Ntot], start / length int32 [C]: clip c is data[start[c] .. + length[c])
//   plan     int32 [B, 4] = (on, clip, off, snr_cdb)
//   part     fp32 [B, ceil(S / 4096), 2] = (sum x^2, sum z^2) of a segment
//   energy   fp64 [B, 2] = (Ex, En); coef fp32 [B] = k; out fp32 [B, S]
//
// z_i = data[start[clip] + (off + i) mod length[clip]] is the clip read as a loop from `off`.
//
// waveaug_plan_kernel: one lane per utterance, one Philox4x32-10 block with key seed and counter
// (0, first_utt + b, step_lo, 0x40000000 | step_hi & 0x3fffffff): bit 30 of the last word keeps
// the stream apart from SpecAugment's (bits 31, 30 clear) and dropout's (bit 31 set). With
// U(w, m) = mulhi(w, m): on = n > 0 && U(x0, 1000000) < p_ppm, clip = U(x1, C),
// off = U(x2, length[clip]), snr_cdb = lo + U(x3, hi - lo + 1). Integers only: ops/reference.py
// waveaug_plan_ref agrees bit for bit.
//
// waveaug_energy_kernel: grid (4096-sample segment, utterance), 256 threads. Thread t owns the
// 8-sample groups t and t + 256 of its segment (one or two 16-byte loads of x each) and sums
// its 16 squares in ascending order as an fma chain from 0 (terms at i >= n are 0 by selection);
// the wave adds its 64 lanes as a butterfly (xor 32, 16, ... 1), the four waves add as
// (w0 + w1) + (w2 + w3): a term passes through at most 16 + 6 + 2 = 24 roundings, in an order
// that depends on its position in the row alone. The noise position takes one modulo per lane
// (the group t; group t + 256 is 2048 mod length further) and a compare per sample. Segments at
// or past n write nothing.
//
// waveaug_coef_kernel: one lane per utterance adds the ceil(n / 4096) partials in fp64,
// ascending, and rounds k = sqrt(Ex / (En 10^(snr_cdb / 1000))) once; k = 0 by selection when
// on == 0, Ex == 0, En == 0 or the value is not finite. Ex, En and k therefore depend on the
// row's content, n, clip and off only: not on the batch, the row index or S.
//
// waveaug_apply_kernel: the same grid and ownership. on: y = x + k z as a rounded product and a
// rounded sum (contraction off: mix());
// not on: a bit copy of x, the noise is not read; i >= n: +0 without reading x. 16-byte stores.
//
// The bank's start and length words and the plan's clip and off words come from device memory
// the launcher cannot see: every kernel clamps them into [0, Ntot) and [0, length) before it
// forms an address, so a damaged word can change values but never reach outside the bank.
#include "common.h"
#include "philox.h"

using namespace ds2;

namespace {

constexpr int NTHR = 256;
constexpr int SEG = 4096;        // samples per workgroup
constexpr int GRP = 8;           // samples per 16-byte group of int16 (two groups of fp32)
constexpr int MAX_B = 65535, MAX_S = (1 << 30) - 8;

struct Bank {
  const float* data;
  const int* start;
  const int* length;
  int C;
  long long Ntot;
};

struct Clip {                    // a plan row's clip, clamped into the bank
  const float* z;                // data + start
  int length, off;               // length 0: nothing to read (z_i = 0)
};

__device__ __forceinline__ int clamp_len(const int* lens, int b, int S) {
  return lens != nullptr ? min(max(lens[b], 0), S) : S;
}

__device__ __forceinline__ Clip clip_of(const Bank& k, const int* plan_row) {
  const int c = min(max(plan_row[1], 0), k.C - 1);
  const long long s = min(max((long long)k.start[c], 0ll), k.Ntot);
  const int len = (int)min((long long)max(k.length[c], 0), k.Ntot - s);
  return {k.data + s, len, len > 0 ? min(max(plan_row[2], 0), len - 1) : 0};
}

struct f32x4s {
  float v[4];
};

// samples [i0, i0 + 8) of a row as fp32; the row is 16-byte aligned and i0 % 8 == 0
template <bool I16>
__device__ __forceinline__ void load8(const void* row, int i0, float (&v)[GRP]) {
  if (I16) {
    const i32x4 w = *reinterpret_cast<const i32x4*>(static_cast<const short*>(row) + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (float)(short)(w[j] & 0xffff);
      v[2 * j + 1] = (float)(short)(w[j] >> 16);
    }
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(static_cast<const float*>(row) + i0);
    const f32x4 b = *reinterpret_cast<const f32x4*>(static_cast<const float*>(row) + i0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j], v[4 + j] = b[j];
  }
}

// z[pos .. pos + 8) of the looped clip (0 <= pos < length); the straight case reads two 4-byte
// aligned 16-byte words
__device__ __forceinline__ void noise8(const Clip& c, int pos, float (&z)[GRP]) {
  if (pos + GRP <= c.length) {
    f32x4s a, b;
    __builtin_memcpy(&a, c.z + pos, 16);
    __builtin_memcpy(&b, c.z + pos + 4, 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = a.v[j], z[4 + j] = b.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < GRP; ++j) {
      int p = pos + j;
      while (p >= c.length) p -= c.length;        // length >= 1; more than once only when length < 8
      z[j] = c.z[p];
    }
  }
}

// fl32(x + fl32(k z)): two roundings. __fmul_rn / __fadd_rn are a plain product and sum to the
// compiler, which fuses the pair into one fma under its default contraction, so the product and
// the sum stand here under a pragma that turns contraction off.
__device__ __forceinline__ float mix(float x, float k, float z) {
#pragma clang fp contract(off)
  const float kz = k * z;
  return x + kz;
}

__global__ __launch_bounds__(64) void waveaug_plan_kernel(const int* __restrict__ lens, const int* __restrict__ length,
                                                          int* __restrict__ plan, int B, int S, int C, int p_ppm,
                                                          int snr_lo, int snr_hi, unsigned seed_lo, unsigned seed_hi,
                                                          unsigned step_lo, unsigned step_hi, unsigned first_utt) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = clamp_len(lens, b, S);
  unsigned x[4];
  philox4x32_10(0u, first_utt + (unsigned)b, step_lo, 0x40000000u | (step_hi & 0x3fffffffu), seed_lo, seed_hi, x);
  const int clip = (int)__umulhi(x[1], (unsigned)C);
  const i32x4 row = {n > 0 && (int)__umulhi(x[0], 1000000u) < p_ppm ? 1 : 0, clip,
                     (int)__umulhi(x[2], (unsigned)max(length[clip], 0)),
                     snr_lo + (int)__umulhi(x[3], (unsigned)(snr_hi - snr_lo) + 1u)};
  *reinterpret_cast<i32x4*>(plan + 4 * (long long)b) = row;
}

template <bool I16>
__global__ __launch_bounds__(NTHR) void waveaug_energy_kernel(const void* __restrict__ x, const int* __restrict__ lens,
                                                              const int* __restrict__ plan, Bank bank,
                                                              float* __restrict__ part, int S) {
  __shared__ float s_w[2][NTHR / 64];
  const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  const int n = clamp_len(lens, b, S);
  if (seg * SEG >= n) return;                      // uniform: before the barrier
  const Clip c = clip_of(bank, plan + 4 * (long long)b);
  const char* row = static_cast<const char*>(x) + (long long)b * S * (I16 ? 2 : 4);
  const int step = c.length > 0 ? (NTHR * GRP) % c.length : 0;        // uniform
  int pos = 0;
  float ex = 0.f, en = 0.f;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int i0 = seg * SEG + (g * NTHR + tid) * GRP;
    if (c.length > 0) {
      if (g == 0) {
        pos = (int)(((unsigned)c.off + (unsigned)i0) % (unsigned)c.length);   // off + i0 < 2^31
      } else {
        pos += step;
        if (pos >= c.length) pos -= c.length;
      }
    }
    if (i0 >= n) continue;                         // i0 < S too: S % 8 == 0 and n <= S
    float v[GRP], z[GRP];
    load8<I16>(row, i0, v);
    if (c.length > 0) {
      noise8(c, pos, z);
    } else {
#pragma unroll
      for (int j = 0; j < GRP; ++j) z[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < GRP; ++j) {
      const bool in = i0 + j < n;
      const float xv = in ? v[j] : 0.f, zv = in ? z[j] : 0.f;
      ex = __fmaf_rn(xv, xv, ex);
      en = __fmaf_rn(zv, zv, en);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ex = __fadd_rn(ex, __shfl_xor(ex, o, 64));
    en = __fadd_rn(en, __shfl_xor(en, o, 64));
  }
  if ((tid & 63) == 0) s_w[0][tid >> 6] = ex, s_w[1][tid >> 6] = en;
  __syncthreads();
  if (tid < 2) {
    const float* w = s_w[tid];
    part[((long long)b * gridDim.x + seg) * 2 + tid] = __fadd_rn(__fadd_rn(w[0], w[1]), __fadd_rn(w[2], w[3]));
  }
}

__global__ __launch_bounds__(64) void waveaug_coef_kernel(const int* __restrict__ lens, const int* __restrict__ plan,
                                                          const float* __restrict__ part, double* __restrict__ energy,
                                                          float* __restrict__ coef, int B, int S, int nseg) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = clamp_len(lens, b, S);
  const int ns = (n + SEG - 1) / SEG;              // <= nseg
  const float* p = part + (long long)b * nseg * 2;
  double ex = 0.0, en = 0.0;
  for (int s = 0; s < ns; ++s) {
    ex += (double)p[2 * s];
    en += (double)p[2 * s + 1];
  }
  energy[2 * (long long)b] = ex;
  energy[2 * (long long)b + 1] = en;
  const int on = plan[4 * (long long)b], snr = plan[4 * (long long)b + 3];
  const float k = (float)sqrt(ex / (en * pow(10.0, (double)snr / 1000.0)));
  coef[b] = (on != 0 && ex != 0.0 && en != 0.0 && isfinite(k)) ? k : 0.f;
}

template <bool I16>
__global__ __launch_bounds__(NTHR) void waveaug_apply_kernel(const void* __restrict__ x, const int* __restrict__ lens,
                                                             const int* __restrict__ plan, const float* __restrict__ coef,
                                                             Bank bank, float* __restrict__ out, int S) {
  const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  const int n = clamp_len(lens, b, S);
  const int* prow = plan + 4 * (long long)b;
  const bool on = prow[0] != 0;
  Clip c{nullptr, 0, 0};
  float k = 0.f;
  if (on) {                                        // uniform
    c = clip_of(bank, prow);
    k = coef[b];
  }
  const char* row = static_cast<const char*>(x) + (long long)b * S * (I16 ? 2 : 4);
  float* orow = out + (long long)b * S;
  const int step = c.length > 0 ? (NTHR * GRP) % c.length : 0;
  int pos = 0;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int i0 = seg * SEG + (g * NTHR + tid) * GRP;
    if (c.length > 0) {
      if (g == 0) {
        pos = (int)(((unsigned)c.off + (unsigned)i0) % (unsigned)c.length);
      } else {
        pos += step;
        if (pos >= c.length) pos -= c.length;
      }
    }
    if (i0 >= S) continue;
    float y[GRP];
    if (i0 >= n) {
#pragma unroll
      for (int j = 0; j < GRP; ++j) y[j] = 0.f;
    } else {
      load8<I16>(row, i0, y);
      if (on) {
        float z[GRP];
        if (c.length > 0) {
          noise8(c, pos, z);
        } else {
#pragma unroll
          for (int j = 0; j < GRP; ++j) z[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < GRP; ++j) y[j] = mix(y[j], k, z[j]);
      }
#pragma unroll
      for (int j = 0; j < GRP; ++j)
        if (i0 + j >= n) y[j] = 0.f;
    }
    *reinterpret_cast<f32x4*>(orow + i0) = f32x4{y[0], y[1], y[2], y[3]};
    *reinterpret_cast<f32x4*>(orow + i0 + 4) = f32x4{y[4], y[5], y[6], y[7]};
  }
}

bool bad_dims(int B, int S) { return B < 1 || B > MAX_B || S < GRP || S > MAX_S || S % GRP != 0; }
bool bad_bank(int C, long long Ntot) { return C < 1 || Ntot < 1 || Ntot >= (1ll << 31); }
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace

extern "C" int ds2_waveaug_segment() { return SEG; }

extern "C" int ds2_waveaug_plan(const int* lens, const int* length, int* plan, int B, int S, int C, int p_ppm,
                                int snr_lo_cdb, int snr_hi_cdb, unsigned seed_lo, unsigned seed_hi, unsigned step_lo,
                                unsigned step_hi, unsigned first_utt, hipStream_t st) {
  if (B < 1 || S < 1 || C < 1) return -120;
  constexpr int BIG = 1 << 20;
  if (p_ppm < 0 || p_ppm > 1000000 || snr_lo_cdb < -BIG || snr_hi_cdb > BIG || snr_lo_cdb > snr_hi_cdb) return -121;
  if (misaligned(plan)) return -122;
  ds2_launch(waveaug_plan_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, lens, length, plan, B, S, C, p_ppm,
             snr_lo_cdb, snr_hi_cdb, seed_lo, seed_hi, step_lo, step_hi, first_utt);
  return (int)hipGetLastError();
}

extern "C" int ds2_waveaug_energy(const void* x, int in_i16, const int* lens, const int* plan, const float* data,
                                  const int* start, const int* length, int C, long long Ntot, float* part, int B, int S,
                                  hipStream_t st) {
  if (bad_dims(B, S) || bad_bank(C, Ntot)) return -120;
  if (misaligned(x)) return -122;
  const Bank bank{data, start, length, C, Ntot};
  const dim3 grid((unsigned)((S + SEG - 1) / SEG), (unsigned)B);
  if (in_i16) ds2_launch(waveaug_energy_kernel<true>, grid, dim3(NTHR), 0, st, x, lens, plan, bank, part, S);
  else ds2_launch(waveaug_energy_kernel<false>, grid, dim3(NTHR), 0, st, x, lens, plan, bank, part, S);
  return (int)hipGetLastError();
}

extern "C" int ds2_waveaug_coef(const int* lens, const int* plan, const float* part, double* energy, float* coef,
                                int B, int S, hipStream_t st) {
  if (bad_dims(B, S)) return -120;
  ds2_launch(waveaug_coef_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, lens, plan, part, energy, coef, B, S,
             (S + SEG - 1) / SEG);
  return (int)hipGetLastError();
}

extern "C" int ds2_waveaug_apply(const void* x, int in_i16, const int* lens, const int* plan, const float* coef,
                                 const float* data, const int* start, const int* length, int C, long long Ntot,
                                 float* out, int B, int S, hipStream_t st) {
  if (bad_dims(B, S) || bad_bank(C, Ntot)) return -120;
  if (misaligned(x) || misaligned(out)) return -122;
  const Bank bank{data, start, length, C, Ntot};
  const dim3 grid((unsigned)((S + SEG - 1) / SEG), (unsigned)B);
  if (in_i16) ds2_launch(waveaug_apply_kernel<true>, grid, dim3(NTHR), 0, st, x, lens, plan, coef, bank, out, S);
  else ds2_launch(waveaug_apply_kernel<false>, grid, dim3(NTHR), 0, st, x, lens, plan, coef, bank, out, S);
  return (int)hipGetLastError();
}
