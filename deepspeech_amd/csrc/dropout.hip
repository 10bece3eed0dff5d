// Dropout between recurrent layers: a stateless mask from a counter-based generator.
//
//   x, out   bf16 [T, N, H] contiguous, H % 8 == 0, 16-byte aligned, T * N * (H / 8) < 2^31
//   ctr      int32 [2] on the device = (step mod 2^32, first_utt mod 2^32), read by the kernel: a
//            captured launch replays with whatever the words hold at that time
//
// Element (t, b, i) belongs to group g = i >> 3, slot e = i & 7. One Philox4x32-10 block serves
// a group: key = seed, counter = (locked ? 0 : t, first_utt + b, step,
// 0x80000000 | locked << 30 | site << 16 | g). Bit 31 of the last word keeps these streams apart
// from SpecAugment's under the same seed (its last word is step >> 32). With output words
// x0..x3, r = (x[e >> 1] >> (16 * (e & 1))) & 0xffff and the element is kept iff r >= thr:
// the drop probability is exactly thr / 65536. A kept element becomes bf16(float(x) * scale)
// (one fp32 product, round to nearest even), a dropped one +0 by selection, so an inf or a NaN
// under a dropped element does not survive. The backward pass is the same map on the gradient.
//
// seq_dropout_kernel: one lane per group: one 16-byte load, one Philox block, eight selections,
// one 16-byte store. (t, b, g) come from the flat group index by two multiplications with
// host-computed 64-bit reciprocals (exact for every index < 2^31); no division, no LDS, no
// atomics. In place (x == out) a lane reads its 16 bytes before it writes them and touches no
// other lane's.
#include "common.h"
#include "philox.h"

using namespace ds2;

namespace {

constexpr int NTHR = 256;

struct Drop {
  const i32x4* x;
  i32x4* out;
  const unsigned* ctr;
  unsigned ngroups;                // T * N * (H / 8)
  unsigned G8, N;                  // groups per row, rows per frame
  unsigned long long mG8, mN;      // ceil(2^64 / G8), ceil(2^64 / N); 0 for a divisor of 1
  unsigned seed_lo, seed_hi, c3;   // c3 without the group
  unsigned thr;
  float scale;
  int locked;
};

// q / d for q < 2^31 with m = ceil(2^64 / d): the error term q * (m * d - 2^64) < 2^31 * d < 2^64
__device__ __forceinline__ unsigned div_magic(unsigned q, unsigned long long m) {
  return m == 0 ? q : (unsigned)__umul64hi((unsigned long long)q, m);
}

__device__ __forceinline__ unsigned drop2(unsigned v, unsigned w, unsigned thr, float scale) {
  const unsigned r0 = w & 0xffffu, r1 = w >> 16;
  const float lo = __fmul_rn(bf2f((bf16_t)(v & 0xffffu)), scale), hi = __fmul_rn(bf2f((bf16_t)(v >> 16)), scale);
  const unsigned o0 = r0 >= thr ? (unsigned)f2bf(lo) : 0u, o1 = r1 >= thr ? (unsigned)f2bf(hi) : 0u;
  return o0 | (o1 << 16);
}

__global__ __launch_bounds__(NTHR) void seq_dropout_kernel(Drop a) {
  const unsigned q = blockIdx.x * NTHR + threadIdx.x;
  if (q >= a.ngroups) return;
  const unsigned step = a.ctr[0], first_utt = a.ctr[1];
  const unsigned row = div_magic(q, a.mG8), g = q - row * a.G8;
  const unsigned t = div_magic(row, a.mN), b = row - t * a.N;
  unsigned w[4];
  philox4x32_10(a.locked ? 0u : t, first_utt + b, step, a.c3 | g, a.seed_lo, a.seed_hi, w);
  const i32x4 v = a.x[q];
  i32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (int)drop2((unsigned)v[j], w[j], a.thr, a.scale);
  a.out[q] = o;
}

unsigned long long magic(unsigned d) { return d <= 1 ? 0ull : ~0ull / d + 1ull; }

}  // namespace

extern "C" int ds2_seq_dropout(const void* x, void* out, const int* ctr, int T, int N, int H, unsigned seed_lo,
                               unsigned seed_hi, int site, int thr, float scale, int locked, hipStream_t st) {
  if (T < 1 || N < 1 || H < 8 || H % 8 != 0 || H / 8 > 65536) return -80;
  const long long ng = (long long)T * N * (H / 8);
  if (ng >= (1ll << 31)) return -80;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(ctr) & 3) != 0)
    return -81;
  if (site < 0 || site >= 16384 || thr < 1 || thr > 65535 || !(scale >= 1.f)) return -82;
  const unsigned G8 = (unsigned)(H / 8);
  const Drop a{static_cast<const i32x4*>(x), static_cast<i32x4*>(out), reinterpret_cast<const unsigned*>(ctr),
               (unsigned)ng, G8, (unsigned)N, magic(G8), magic((unsigned)N), seed_lo, seed_hi,
               0x80000000u | (locked ? 1u << 30 : 0u) | ((unsigned)site << 16), (unsigned)thr, scale, locked ? 1 : 0};
  ds2_launch(seq_dropout_kernel, dim3((unsigned)((ng + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, a);
  return (int)hipGetLastError();
}
