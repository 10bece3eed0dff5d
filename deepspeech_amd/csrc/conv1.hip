// conv1 (C_in = 1) of the DeepSpeech2 front-end for gfx950: forward and weight gradient
// (layouts and the MFMA fragment mapping: conv_common.h).
//
//   conv1 fwd   rows = f1, cols = co, k = (kt, kf' in 0..7) (kf' >= 5 carry zero weights),
//               so a lane's 8 k-values are 8 consecutive input samples.
//   conv1 wgrad rows = co, cols = (kt, kf'), k = positions, input staged de-interleaved
//               (x[t][2p + kf'] as [t][kf'][p]) so the B fragment is one ds_read_b128.
#include "bn_math.h"
#include "conv_common.h"

using namespace ds2;

namespace {

// =====================================================================================
// conv1 forward
// =====================================================================================
struct Conv1Fwd {
  const bf16_t* x;    // [N][T][F0]
  const bf16_t* w;    // [32][1][20][5]
  const float* bias;  // [32] or null
  bf16_t* y;          // [N][T1][F1][32]
  float* part;        // [grid][32][2]
  int N, T, F0, T1, F1;
};
constexpr int C1_KT = 20, C1_KF = 5;
constexpr int C1_XS = 200;     // staged row stride (elements): covers 2*95 + 7
constexpr int C1_ROWS = 4;     // output rows per workgroup (one per wave)
constexpr int C1_IN = 2 * (C1_ROWS - 1) + C1_KT;   // 26 input rows

// stage input rows t0 .. t0+C1_IN-1 of one utterance ([T][F0] bf16, rows 2-B aligned only) into
// LDS rows of C1_XS elements, zero outside the utterance / beyond F0. Loads are unconditional
// (clamped addresses) so all of them are in flight together; the select happens afterwards.
__device__ __forceinline__ void stage_rows(bf16_t* xs, const bf16_t* xu, int t0, int T, int F0) {
  constexpr int NE = C1_IN * C1_XS, K = (NE + 255) / 256;
  bf16_t v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int idx = min((int)threadIdx.x + 256 * k, NE - 1);
    const int r = idx / C1_XS, c = idx - r * C1_XS;
    v[k] = xu[(size_t)min(t0 + r, T - 1) * F0 + min(c, F0 - 1)];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int idx = (int)threadIdx.x + 256 * k;
    const int r = idx / C1_XS, c = idx - r * C1_XS;
    if (idx < NE) xs[idx] = (t0 + r < T && c < F0) ? v[k] : (bf16_t)0;
  }
}

__global__ __launch_bounds__(256) void conv1_fwd_kernel(Conv1Fwd a) {
  __shared__ __attribute__((aligned(16))) bf16_t xs[C1_IN * C1_XS];
  __shared__ __attribute__((aligned(16))) bf16_t ys[C1_ROWS][32 * MT * CC];   // each wave's output row (F1 <= 96)
  __shared__ float statsh[4 * 32 * 2];
  const int tid = threadIdx.x, lane = tid & 63, w = uni(tid >> 6);
  const int hi = lane >> 5, col = lane & 31;
  const int tb = (a.T1 + C1_ROWS - 1) / C1_ROWS;
  const int n = blockIdx.x / tb, t1_0 = (blockIdx.x - n * tb) * C1_ROWS;
  stage_rows(xs, a.x + (size_t)n * a.T * a.F0, 2 * t1_0, a.T, a.F0);
  bf16x8 bfr[10];
#pragma unroll
  for (int s = 0; s < 10; ++s) {
    const int kt = 2 * s + hi;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < C1_KF ? (short)a.w[(col * C1_KT + kt) * C1_KF + j] : (short)0;
    bfr[s] = v;
  }
  const float bco = a.bias ? a.bias[col] : 0.f;
  __syncthreads();
  float ssum = 0.f, ssq = 0.f;
  const int t1 = t1_0 + w;
  if (t1 < a.T1) {
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x16){};
#pragma unroll
    for (int s = 0; s < 10; ++s) {
      const int r = 2 * w + 2 * s + hi;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const unsigned* p = (const unsigned*)(xs + r * C1_XS + 2 * (32 * m + col));
        const unsigned u0 = p[0], u1 = p[1], u2 = p[2], u3 = p[3];
        const bf16x8 av = __builtin_bit_cast(bf16x8, (i32x4){(int)u0, (int)u1, (int)u2, (int)u3});
        acc[m] = mfma32(av, bfr[s], acc[m]);
      }
    }
    // the row goes through this wave's LDS row as bf16 [F1][32], then out in 16-B chunks
    // (48 two-byte stores per lane otherwise)
    bf16_t* yl = ys[w];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f1 = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (f1 < a.F1) {
          const bf16_t b = f2bf(acc[m][r] + bco);
          yl[f1 * CC + col] = b;
          const float vb = bf2f(b);
          ssum += vb;
          ssq += vb * vb;
        }
      }
    copy_row(a.y + ((size_t)n * a.T1 + t1) * a.F1 * CC, yl, a.F1 * 4, lane, 64);
  }
  channel_sums(ssum, ssq, statsh, w, a.part);
}

// =====================================================================================
// conv1 weight gradient
// =====================================================================================
struct Conv1Wgrad {
  const bf16_t* dy;   // [N][T1][F1][32], or null with bn.dz: dy computed while staging
  const bf16_t* x;    // [N][T][F0]
  float* part;        // [grid][5][4][64][4]
  int N, T, F0, T1, F1;
  // all null without conv1's BatchNorm backward applied in the staging (the bn_math.h calls of
  // bn_cl_bwd_apply_kernel, so dy is bitwise the same)
  DS2Conv1WgradBn bn;
  float M;            // N * T1 * F1
};
constexpr int C1W_XP = 88;                       // de-interleaved row stride (positions)
constexpr int C1W_DY = C1_ROWS * 80 * 64;        // dy image bytes (4 rows x 80 positions)
constexpr int C1W_XD = C1_IN * 8 * C1W_XP * 2;   // x image bytes
constexpr int C1W_RED = 4 * 5 * 4 * 64 * 16;     // wave partials
constexpr int C1W_RAW = C1_IN * C1_XS * 2;             // raw input rows
constexpr int C1W_SMEM = (C1W_DY + C1W_XD + C1W_RAW) > C1W_RED ? (C1W_DY + C1W_XD + C1W_RAW) : C1W_RED;

__global__ __launch_bounds__(256) void conv1_wgrad_kernel(Conv1Wgrad a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = uni(tid >> 6);
  const int hi = lane >> 5, col = lane & 31;
  unsigned char* dys = smem;
  bf16_t* xd = (bf16_t*)(smem + C1W_DY);
  bf16_t* raw = (bf16_t*)(smem + C1W_DY + C1W_XD);
  const int tb = (a.T1 + C1_ROWS - 1) / C1_ROWS;
  const int ntiles = a.N * tb;
  const unsigned lofs = tr_lane_ofs(lane);
  const int bkt = col >> 3, bkf = col & 7;

  // fused BN backward: a thread's chunks all hold channels 8 (tid & 3) .. + 7 (256 and 320 are
  // multiples of 4), so their constants stay in registers
  const bool bn = a.bn.dz != nullptr;
  const bf16_t *bdz = (const bf16_t*)a.bn.dz, *by1 = (const bf16_t*)a.bn.y1;
  float bmu[8], bis[8], bg[8], bbt[8], bmdb[8], bmdg[8];
  if (bn) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = (tid & 3) * 8 + j;
      bmu[j] = a.bn.mean[c]; bis[j] = a.bn.invstd[c]; bg[j] = a.bn.gamma[c]; bbt[j] = a.bn.beta[c];
      bmdb[j] = a.bn.dbeta[c] / a.M; bmdg[j] = a.bn.dgamma[c] / a.M;
    }
  }
  f32x16 acc[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) acc[i] = (f32x16){};
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / tb, t1_0 = (tile - n * tb) * C1_ROWS;
    __syncthreads();   // previous tile's reads done
    // dy rows t1_0 .. t1_0+3 -> [row][80][32] (positions >= F1 zero)
    for (int ch = tid; ch < C1_ROWS * 80 * 4; ch += 256) {
      const int r = ch / 320, rem = ch - r * 320, pos = rem >> 2, c4 = rem & 3;
      const int t1 = t1_0 + r;
      i32x4 v = (i32x4){0, 0, 0, 0};
      if (pos < a.F1 && t1 < a.T1) {
        const size_t off = (((size_t)n * a.T1 + t1) * a.F1 + pos) * CC + c4 * 8;
        if (bn) {
          const bf16x8 y = *(const bf16x8*)(by1 + off), d = *(const bf16x8*)(bdz + off);
          bf16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xh = bn_xhat(bf2f((bf16_t)y[j]), bmu[j], bis[j]);
            const float dd = bn_masked(xh, bg[j], bbt[j], bf2f((bf16_t)d[j]));
            o[j] = (short)f2bf(bn_bwd_value(bg[j] * bis[j], dd, xh, bmdb[j], bmdg[j]));
          }
          v = __builtin_bit_cast(i32x4, o);
        } else {
          v = *(const i32x4*)(a.dy + off);
        }
      }
      *(i32x4*)(dys + ch * 16) = v;
    }
    // x rows 2*t1_0 + r: raw rows into LDS, then de-interleaved xd[r][kf'][p] = x[t][2p + kf']
    stage_rows(raw, a.x + (size_t)n * a.T * a.F0, 2 * t1_0, a.T, a.F0);
    __syncthreads();
    // kf fastest: the 8 lanes of one (row, position block) read 8 consecutive raw elements per j
    // (one LDS word for two of them), so a wave's 2-byte reads hit 32 distinct banks; with the
    // position block fastest, lanes sat 32 B apart (8-way bank conflicts: 42 % of the kernel's
    // LDS cycles, PMC SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE)
    for (int ch = tid; ch < C1_IN * 8 * 10; ch += 256) {
      const int kf = ch & 7, q = ch >> 3, r = q / 10, p0 = (q - r * 10) * 8;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (short)raw[r * C1_XS + min(2 * (p0 + j) + kf, C1_XS - 1)];
      *(bf16x8*)(xd + (r * 8 + kf) * C1W_XP + p0) = v;
    }
    __syncthreads();
    const int t1 = t1_0 + w;
    if (t1 < a.T1) {
#pragma unroll
      for (int kk = 0; kk < 5; ++kk) {
        const unsigned k0 = (unsigned)(16 * kk);
        const bf16x8 av = tr_frag(dys + (w * 80 + k0) * 64 + lofs);
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) {
          const int r = 2 * w + 4 * nt + bkt;
          const bf16x8 bv = *(const bf16x8*)(xd + (r * 8 + bkf) * C1W_XP + k0 + 8 * hi);
          acc[nt] = mfma32(av, bv, acc[nt]);
        }
      }
    }
  }
  __syncthreads();
  f32x4* red = (f32x4*)smem;
#pragma unroll
  for (int nt = 0; nt < 5; ++nt)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) red[((w * 5 + nt) * 4 + r4) * 64 + lane] = acc4(acc[nt], r4);
  __syncthreads();
  f32x4* out = (f32x4*)(a.part + (size_t)blockIdx.x * 5 * 1024);
  for (int e = tid; e < 5 * 4 * 64; e += 256) {
    f32x4 v = red[e];
    for (int wv = 1; wv < 4; ++wv) v += red[wv * 5 * 4 * 64 + e];
    out[e] = v;
  }
}

bool conv1_geometry(int T, int F0, int T1, int F1, int F1max) {
  return F1 <= F1max && F1 == (F0 - 5) / 2 + 1 && T1 == (T - 20) / 2 + 1 && T1 >= 1;
}

}  // namespace

extern "C" {

long long ds2_conv1_wgrad_part_floats(int grid) { return (long long)grid * 5 * 1024; }
int ds2_conv1_fwd_grid(int N, int T1) { return N * ((T1 + C1_ROWS - 1) / C1_ROWS); }

int ds2_conv1_fwd(const void* x, const void* w, const float* bias, void* y, float* part, int N, int T, int F0,
                  int T1, int F1, hipStream_t st) {
  if (!conv1_geometry(T, F0, T1, F1, 96)) return CONV1_FWD_GEOMETRY;
  Conv1Fwd a{(const bf16_t*)x, (const bf16_t*)w, bias, (bf16_t*)y, part, N, T, F0, T1, F1};
  hipLaunchKernelGGL(conv1_fwd_kernel, dim3(ds2_conv1_fwd_grid(N, T1)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int ds2_conv1_wgrad(const void* dy, const void* x, float* part, int grid, float* dw, int N, int T, int F0, int T1,
                    int F1, const DS2Conv1WgradBn* bn, hipStream_t st) {
  if (!conv1_geometry(T, F0, T1, F1, 80)) return CONV1_WGRAD_GEOMETRY;
  if ((dy == nullptr) == (bn == nullptr)) return CONV1_WGRAD_DY_XOR_BN;
  DS2_HIP_CHECK((hipError_t)set_smem(conv1_wgrad_kernel, C1W_SMEM));
  Conv1Wgrad a{(const bf16_t*)dy, (const bf16_t*)x, part, N, T, F0, T1, F1, bn ? *bn : DS2Conv1WgradBn{},
               (float)((double)N * T1 * F1)};
  hipLaunchKernelGGL(conv1_wgrad_kernel, dim3(grid), dim3(256), C1W_SMEM, st, a);
  hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(5 * 1024 / 256), dim3(256), 0, st, part, grid, 5 * 1024, dw);
  return (int)hipGetLastError();
}

}  // extern "C"
