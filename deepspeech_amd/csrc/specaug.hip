// SpecAugment (Park et al., 2019) for stored feature frames: a time warp, frequency masks and
// time masks per utterance, drawn from a counter-based generator.
//
//   x, out   fp32 [B, T, F] contiguous, 1 <= F <= 1024, 1 <= T <= 32767 (t * w0 stays in 32 bits)
//   lens     int32 [B]; L = clamp(lens[b], 0, T); frames t >= L are padding and are copied
//   plan     int32 [B, 2 + 2 nF + 2 nT] = (w0, w, f0_0, fw_0, ..., t0_0, tw_0, ...)
//   mean     fp32 [B, F] (fill = mean) or absent (fill = zero)
//
// specaug_plan_kernel: one lane per utterance. Philox4x32-10 keyed by the seed, counter
// (block j, utterance u = first_utt + b, step): its words are x[4j .. 4j+3], consumed in the
// order warp (2), two per frequency mask, two per time mask. A uniform integer in [0, n) is
// mulhi(x, n): integer arithmetic only, so the host oracle agrees bit for bit.
//   warp   n0 = L - 2W - 2; W == 0 or n0 < 1: w0 = w = 0 (identity); else
//          w0 = W + 1 + mulhi(x0, n0), w = mulhi(x1, 2W + 1) - W; d0 = w0 + w lies in [1, L-2]
//   freq   fw = mulhi(x, min(Fw, F) + 1), f0 = mulhi(x', F - fw + 1)
//   time   c = min(Tw, L * p_ppm / 1000000), tw = mulhi(x, c + 1), t0 = mulhi(x', L - tw + 1)
//
// specaug_mean_kernel: mean[b, f] over frames t < L of the input, one workgroup per (utterance,
// tile of 16 bins). Thread (s, f) sums frames s, s + 32, s + 64, ... in ascending order, the 32
// partials of a bin are added pairwise ((p0 + p1) + (p2 + p3)) + ... through LDS and the total is
// divided by float(L) (0 when L == 0): the order depends on L alone, so an utterance's mean is
// bitwise the same in any batch and any row. No atomics.
//
// specaug_apply_kernel: grid (time tile of 16 frames, utterance). The workgroup reads its plan
// row once, builds the per-bin keep mask and fill values and the per-frame source (row i, weight
// r / den, or "time masked") in LDS, then walks the tile's flat span of nt * F floats. A row of
// F = 161 floats is 644 bytes, so rows are not 16-byte multiples: the span is cut at the 16-byte
// boundaries of the output (scalar head and tail, aligned 16-byte stores between), the sources
// are read with 4-byte aligned 16-byte loads, and a group of four that straddles two rows goes
// element by element. A time-masked frame is written without being read, an unmasked frame
// reads one source row (r == 0: a bit copy) or two (fma(r / den, b - a, a)). Masked cells take
// the fill by selection, so a NaN under a mask does not survive. The in-place variant (W == 0
// only) reads nothing and writes only the masked cells of frames < L.
#include "common.h"
#include "philox.h"

using namespace ds2;

namespace {

constexpr int NTHR = 256;
constexpr int TT = 16;           // frames per apply tile
constexpr int MAX_NF = 8, MAX_NT = 16, MAX_F = 1024, MAX_T = 32767, MAX_B = 65535;
constexpr int MAX_PLAN = 2 + 2 * MAX_NF + 2 * MAX_NT;
constexpr int MS = 32, MB = 16;  // mean kernel: time slices x bins per workgroup (MS * MB threads)
constexpr int MU = 8;            // mean kernel: loads in flight per thread

struct Policy {
  int nF, Fw, nT, Tw, p_ppm, W;
};

struct Philox {
  unsigned k0, k1, u, s0, s1;
  unsigned x[4];
  int n;
  __device__ __forceinline__ void block(unsigned j) { philox4x32_10(j, u, s0, s1, k0, k1, x); }
  __device__ __forceinline__ unsigned next() {
    if ((n & 3) == 0) block((unsigned)(n >> 2));
    return x[n++ & 3];
  }
};

__device__ __forceinline__ int clamp_len(int l, int T) { return min(max(l, 0), T); }

__global__ __launch_bounds__(64) void specaug_plan_kernel(const int* __restrict__ lens, int* __restrict__ plan, int B,
                                                          int T, int F, Policy p, unsigned seed_lo, unsigned seed_hi,
                                                          unsigned step_lo, unsigned step_hi, unsigned first_utt) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int L = clamp_len(lens[b], T);
  Philox g{seed_lo, seed_hi, first_utt + (unsigned)b, step_lo, step_hi, {0, 0, 0, 0}, 0};
  int* row = plan + (long long)b * (2 + 2 * p.nF + 2 * p.nT);
  const unsigned x0 = g.next(), x1 = g.next();
  const long long n0 = (long long)L - 2ll * p.W - 2;
  int w0 = 0, w = 0;
  if (p.W > 0 && n0 >= 1) {
    w0 = p.W + 1 + (int)__umulhi(x0, (unsigned)n0);
    w = (int)__umulhi(x1, 2u * (unsigned)p.W + 1u) - p.W;
  }
  row[0] = w0;
  row[1] = w;
  for (int k = 0; k < p.nF; ++k) {
    const unsigned xa = g.next(), xb = g.next();
    const int fw = (int)__umulhi(xa, (unsigned)min(p.Fw, F) + 1u);
    row[2 + 2 * k] = (int)__umulhi(xb, (unsigned)(F - fw) + 1u);
    row[3 + 2 * k] = fw;
  }
  const int c = (int)min((long long)p.Tw, (long long)L * p.p_ppm / 1000000ll);
  for (int k = 0; k < p.nT; ++k) {
    const unsigned xa = g.next(), xb = g.next();
    const int tw = (int)__umulhi(xa, (unsigned)c + 1u);
    row[2 + 2 * p.nF + 2 * k] = (int)__umulhi(xb, (unsigned)(L - tw) + 1u);
    row[3 + 2 * p.nF + 2 * k] = tw;
  }
}

__global__ __launch_bounds__(MS * MB) void specaug_mean_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                            float* __restrict__ mean, int T, int F) {
  __shared__ float part[MS][MB + 1];
  const int b = blockIdx.y, fl = threadIdx.x % MB, s = threadIdx.x / MB;
  const int f = blockIdx.x * MB + fl;
  const int L = clamp_len(lens[b], T);
  float acc = 0.f;
  if (f < F) {
    const float* p = x + (long long)b * T * F + f;
    int t = s;
    for (; t + (MU - 1) * MS < L; t += MU * MS) {
      float v[MU];
#pragma unroll
      for (int i = 0; i < MU; ++i) v[i] = p[(long long)(t + i * MS) * F];
#pragma unroll
      for (int i = 0; i < MU; ++i) acc = __fadd_rn(acc, v[i]);
    }
    for (; t < L; t += MS) acc = __fadd_rn(acc, p[(long long)t * F]);
  }
  part[s][fl] = acc;
#pragma unroll
  for (int h = 1; h < MS; h *= 2) {
    __syncthreads();                 // level h reads what level h / 2 wrote to other rows
    if (s % (2 * h) == 0) part[s][fl] = __fadd_rn(part[s][fl], part[s + h][fl]);
  }
  if (s == 0 && f < F) mean[(long long)b * F + f] = L > 0 ? __fdiv_rn(part[0][fl], (float)L) : 0.f;
}

struct Apply {
  const float* x;
  float* out;
  const int* lens;
  const int* plan;
  const float* mean;     // [B, F] or null (fill = zero)
  int T, F, nF, nT;
  unsigned Fmagic;       // ceil(2^32 / F): e / F = mulhi(e, Fmagic) for every e < TT * F (F > 1)
};

struct f32x4s {
  float v[4];
};

__device__ __forceinline__ bool in_span(int i, int start, int width) {
  return (unsigned)(i - start) < (unsigned)max(width, 0) && i >= start;
}

template <bool INPLACE>
__global__ __launch_bounds__(NTHR) void specaug_apply_kernel(Apply a) {
  __shared__ int s_plan[MAX_PLAN];
  __shared__ float s_fill[MAX_F];
  __shared__ unsigned char s_mask[MAX_F];       // bin f is under a frequency mask
  __shared__ unsigned char s_mask4[MAX_F];      // one of the bins f .. f + 3 is
  // frame k of the tile: .x = source row | padding << 16 (padding: frame >= L, copied whatever
  // the masks say), or -1 for a time-masked frame; .y = the bits of r / den, 0: the source row alone
  __shared__ int2 s_meta[TT];

  const int T = a.T, F = a.F, nF = a.nF, nT = a.nT, tid = threadIdx.x;
  const int b = blockIdx.y, t0 = blockIdx.x * TT;
  const int L = clamp_len(a.lens[b], T);
  int nt = min(TT, T - t0);
  if (INPLACE) {
    nt = min(nt, L - t0);          // padding is left alone
    if (nt <= 0) return;           // uniform: before any barrier
  }
  // the plan row and the fill values do not depend on each other: both loads in flight at once
  const int P = 2 + 2 * nF + 2 * nT;
  if (tid < P) s_plan[tid] = a.plan[(long long)b * P + tid];
  for (int f = tid; f < F; f += NTHR) s_fill[f] = a.mean != nullptr ? a.mean[(long long)b * F + f] : 0.f;
  __syncthreads();
  for (int f = tid; f < F; f += NTHR) {
    bool one = false, any = false;
    for (int k = 0; k < nF; ++k) {
      const int f0 = s_plan[2 + 2 * k], fw = s_plan[3 + 2 * k];
      one = one || in_span(f, f0, fw);
      any = any || (f + 3 >= f0 && in_span(max(f, f0), f0, fw));    // [f, f + 3] meets [f0, f0 + fw)
    }
    s_mask[f] = one;
    s_mask4[f] = any;
  }
  if (tid < nt) {
    const int t = t0 + tid;
    int code = t | (1 << 16);      // padding
    float wgt = 0.f;
    if (t < L) {
      bool masked = false;
      for (int k = 0; k < nT; ++k) masked = masked || in_span(t, s_plan[2 + 2 * nF + 2 * k], s_plan[3 + 2 * nF + 2 * k]);
      const int w0 = s_plan[0], d0 = s_plan[0] + s_plan[1];
      code = masked ? -1 : t;
      if (!masked && !INPLACE && w0 >= 1 && w0 <= L - 2 && d0 >= 1 && d0 <= L - 2) {   // else: the identity
        int num, den, base;
        if (t <= d0) num = t * w0, den = d0, base = 0;
        else num = (t - d0) * (L - 1 - w0), den = L - 1 - d0, base = w0;
        const int q = num / den, r = num - q * den;
        code = min(base + q, L - 1);
        if (r != 0 && code + 1 <= L - 1) wgt = __fdiv_rn((float)r, (float)den);
      }
    }
    s_meta[tid] = int2{code, (int)__float_as_uint(wgt)};
  }
  __syncthreads();

  const float* xb = a.x + (long long)b * T * F;      // offsets inside an utterance fit 32 bits (T * F < 2^25)
  float* ob = a.out + ((long long)b * T + t0) * F;
  const int n = nt * F;
  auto frame_of = [&](int e) { return F == 1 ? e : (int)__umulhi((unsigned)e, a.Fmagic); };

  // one cell of the tile; INPLACE: written only when masked
  auto cell = [&](int e, int k, int f) {
    const int2 m = s_meta[k];
    if (INPLACE) {
      if (m.x < 0 || s_mask[f]) ob[e] = s_fill[f];
      return;
    }
    float v;
    if (m.x < 0) {
      v = s_fill[f];
    } else {
      const float* row = xb + (unsigned)((m.x & 0xffff) * F + f);
      v = row[0];
      const float wgt = __uint_as_float((unsigned)m.y);
      if (wgt != 0.f) v = __fmaf_rn(wgt, __fsub_rn(row[F], v), v);
      if (!(m.x >> 16) && s_mask[f]) v = s_fill[f];
    }
    ob[e] = v;
  };

  const int head = min(n, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(ob) & 15u)) & 15u) >> 2));
  const int nvec = (n - head) >> 2, tail = head + 4 * nvec;
  for (int q = tid; q < nvec; q += NTHR) {
    const int e = head + 4 * q;
    int k = frame_of(e), f = e - k * F;
    if (f + 4 <= F) {
      const int2 m = s_meta[k];
      f32x4s o;
      if (INPLACE) {
        if (m.x < 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) o.v[j] = s_fill[f + j];
          *reinterpret_cast<f32x4*>(ob + e) = f32x4{o.v[0], o.v[1], o.v[2], o.v[3]};
        } else if (s_mask4[f]) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (s_mask[f + j]) ob[e + j] = s_fill[f + j];
        }
        continue;
      }
      if (m.x < 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = s_fill[f + j];
      } else {
        const float* row = xb + (unsigned)((m.x & 0xffff) * F + f);
        __builtin_memcpy(&o, row, 16);                       // 4-byte aligned 16-byte load
        const float wgt = __uint_as_float((unsigned)m.y);
        if (wgt != 0.f) {
          f32x4s nx;
          __builtin_memcpy(&nx, row + F, 16);
#pragma unroll
          for (int j = 0; j < 4; ++j) o.v[j] = __fmaf_rn(wgt, __fsub_rn(nx.v[j], o.v[j]), o.v[j]);
        }
        if (s_mask4[f] && !(m.x >> 16)) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (s_mask[f + j]) o.v[j] = s_fill[f + j];
        }
      }
      *reinterpret_cast<f32x4*>(ob + e) = f32x4{o.v[0], o.v[1], o.v[2], o.v[3]};
    } else {
      for (int j = 0; j < 4; ++j) {
        cell(e + j, k, f);
        if (++f == F) f = 0, ++k;
      }
    }
  }
  for (int q = tid; q < head + (n - tail); q += NTHR) {
    const int e = q < head ? q : tail + (q - head);
    const int k = frame_of(e);
    cell(e, k, e - k * F);
  }
}

bool bad_dims(int B, int T, int F) { return B < 1 || B > MAX_B || T < 1 || T > MAX_T || F < 1 || F > MAX_F; }

}  // namespace

extern "C" int ds2_specaug_plan(const int* lens, int* plan, int B, int T, int F, int nF, int Fw, int nT, int Tw,
                                int p_ppm, int W, unsigned seed_lo, unsigned seed_hi, unsigned step_lo,
                                unsigned step_hi, unsigned first_utt, hipStream_t st) {
  if (B < 1 || T < 1 || F < 1) return -70;
  constexpr int BIG = 1 << 30;
  if (nF < 0 || nF > MAX_NF || nT < 0 || nT > MAX_NT || Fw < 0 || Fw > BIG || Tw < 0 || Tw > BIG || W < 0 ||
      W > BIG || p_ppm < 0 || p_ppm > 1000000)
    return -71;
  const Policy p{nF, Fw, nT, Tw, p_ppm, W};
  ds2_launch(specaug_plan_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, lens, plan, B, T, F, p, seed_lo,
             seed_hi, step_lo, step_hi, first_utt);
  return (int)hipGetLastError();
}

extern "C" int ds2_specaug_mean(const float* x, const int* lens, float* mean, int B, int T, int F, hipStream_t st) {
  if (bad_dims(B, T, F)) return -70;
  ds2_launch(specaug_mean_kernel, dim3((unsigned)((F + MB - 1) / MB), (unsigned)B), dim3(MS * MB), 0, st, x, lens, mean,
             T, F);
  return (int)hipGetLastError();
}

extern "C" int ds2_specaug_apply(const float* x, const int* lens, const int* plan, const float* mean, float* out,
                                 int B, int T, int F, int nF, int nT, int inplace, hipStream_t st) {
  if (bad_dims(B, T, F)) return -70;
  if (nF < 0 || nF > MAX_NF || nT < 0 || nT > MAX_NT) return -71;
  if ((inplace != 0) != (x == out)) return -72;            // in place means out is x, and nothing else does
  const Apply a{x, out, lens, plan, mean, T, F, nF, nT, (unsigned)(((1ull << 32) + (unsigned)F - 1) / (unsigned)F)};
  const dim3 grid((unsigned)((T + TT - 1) / TT), (unsigned)B);
  if (inplace) ds2_launch(specaug_apply_kernel<true>, grid, dim3(NTHR), 0, st, a);
  else ds2_launch(specaug_apply_kernel<false>, grid, dim3(NTHR), 0, st, a);
  return (int)hipGetLastError();
}
