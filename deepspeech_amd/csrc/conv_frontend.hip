// DeepSpeech2 conv front-end for gfx950: implicit-GEMM convolutions on MFMA
// (v_mfma_f32_32x32x16_bf16) with channels-last activations, BatchNorm statistics fused
// into the forward epilogues, and channels-last BatchNorm + clipped-ReLU kernels.
//
// Reference graph (src/deepSpeech_NCHW.py:110-168, src/custom_ops.py:99-160):
//   conv1  [20x5] stride (2,2) VALID, 1 -> C   + bias + BN(train, eps 1e-3) + clip(0, 20)
//   conv2  [10x5] stride (2,1) VALID, C -> C   + bias + BN + clip
//   transpose/reshape to time-major [T2, N, C*F2]   (feature index c*F2 + f)
//
// Layouts (C = 32 channels, fixed: the reference's num_filters):
//   feats x0   [N][T][F0]            bf16 (F0 = 161)
//   conv1 y1   [N][T1][F1][C]        bf16, channels-last (F1 = 79)
//   conv2 in   z1 = clip(BN(y1))     same layout
//   conv2 y2   [N][T2][F2][C]        bf16, channels-last (F2 = 75)
//   rnn input  [T2][N][C*F2]         bf16, written by the BN apply through an LDS transpose
//   weights    OIHW bf16 shadows of the fp32 arena (w1 [C][1][20][5], w2 [C][C][10][5])
//
// MFMA mapping (32x32x16 bf16: lane l holds A[row l&31][k 8(l>>5)+j], B[k 8(l>>5)+j][col l&31],
// accumulator reg r -> row (r&3) + 8(r>>2) + 4(l>>5), col l&31):
//   conv2 fwd   rows = 32 output positions f2, cols = 32 co, k = (kt, kf, ci) in 100 k-steps of 16.
//               Persistent: each wave keeps ITS quarter of the weight fragments (25 k-steps) in
//               VGPRs for the whole launch; the 10 input rows of an output row (one contiguous
//               50.5 KB block) are double-buffered in LDS by global_load_lds (XOR-swizzled
//               16-B chunks -> conflict-free ds_read_b128); the 4 K-quarters are summed
//               through LDS in the epilogue, which also adds the bias, stores bf16 and
//               accumulates the BN batch statistics of the stored values.
//   conv2 dgrad rows = 32 input positions f1, cols = 32 ci, k = (kt, kf, co); a tile is the
//               output row pair (2u, 2u+1), whose kt parities read the same 5 rows of dy.
//   conv2 wgrad rows = co, cols = ci, k = positions; both operands are read with
//               ds_read_b64_tr_b16 (hardware transpose) from channels-last LDS images;
//               per-workgroup fp32 partials are summed by a reduce kernel into the arena.
//   conv1 fwd   rows = f1, cols = co, k = (kt, kf' in 0..7) (kf' >= 5 carry zero weights),
//               so a lane's 8 k-values are 8 consecutive input samples.
//   conv1 wgrad rows = co, cols = (kt, kf'), k = positions, input staged de-interleaved
//               (x[t][2p + kf'] as [t][kf'][p]) so the B fragment is one ds_read_b128.
//
// BatchNorm backward in training mode: dbeta = sum(dz*m), dgamma = sum(dz*m*xhat),
// dy = gamma*invstd*(dz*m - dbeta/M - xhat*dgamma/M), m = clip mask. The conv bias gradient
// is identically zero under train-mode BN (the mean subtraction cancels any shift).
#include "common.h"

using namespace ds2;

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

constexpr int CC = 32;          // channels
constexpr float CLIP = 20.0f;
constexpr int MT = 3;           // m-tiles of 32 positions (F1, F2 <= 96)

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// async 16-B global -> LDS copy; lds_wave_base must be wave-uniform (lane L lands at +16L)
__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

// byte offset of 16-B chunk c (0..3) of 64-B LDS position row R in the XOR-swizzled image
__device__ __forceinline__ unsigned swz(unsigned R, unsigned c) { return R * 64u + ((c ^ ((R >> 2) & 3u)) << 4); }

// transposed read: 4 rows x 16 columns of 16-bit elements per 16-lane group (T10)
__device__ __forceinline__ s16x4 tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(p));
}

__device__ __forceinline__ bf16x8 cat8(s16x4 a, s16x4 b) {
  bf16x8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
  r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
  return r;
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// per-workgroup channel statistics: lanes l and l^32 hold the same channel (l & 31)
__device__ __forceinline__ void write_stats(float s, float q, float* sh /* [waves][32][2] */, int nwaves,
                                            float* part) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  s += __shfl_xor(s, 32, 64);
  q += __shfl_xor(q, 32, 64);
  __syncthreads();
  if (lane < 32) {
    sh[(w * 32 + lane) * 2 + 0] = s;
    sh[(w * 32 + lane) * 2 + 1] = q;
  }
  __syncthreads();
  if (tid < 64) {
    const int c = tid >> 1, k = tid & 1;
    float v = 0.f;
    for (int i = 0; i < nwaves; ++i) v += sh[(i * 32 + c) * 2 + k];
    part[(size_t)blockIdx.x * 64 + tid] = v;
  }
}

// =====================================================================================
// conv2 forward
// =====================================================================================
// A tile is one output row t2 (all f2, all 32 co); it reads input rows 2 t2 .. 2 t2 + 9. Wave w
// multiplies k-steps [25 w, 25 w + 25) of the 100 (kt, kf, ci-half), its 25 weight fragments in
// VGPRs for the whole launch; the 4 partial sums meet in wave 0 through a 2-level LDS tree and
// wave 0 adds the bias, stores bf16 and accumulates the BN batch statistics of the stored
// values. The input rows land by global_load_lds in channel-chunk planes: plane (row j, 16-B
// channel chunk c) holds C2F_PL positions at a 16-B stride, so the 16 lanes of a ds_read_b128
// lane group read 16 consecutive 16-B slots (conflict-free) and a fragment address is a lane
// base + a compile-time offset. Positions past F1 read the next plane (or the tail pad): they
// only reach outputs f2 >= F2, which are not stored. Two ~74-KB workgroups per CU, so one's
// reduction and staging overlap the other's MFMA loop; tiles go to XCDs in contiguous ranges
// so the 8 input rows neighbouring tiles share are L2 hits.
struct Conv2Fwd {
  const bf16_t* x;    // z1 [N][T1][F1][32]
  const bf16_t* w;    // [32][32][10][5]
  const float* bias;  // [32] or null
  bf16_t* y;          // [N][T2][F2][32]
  float* part;        // [grid][32][2]
  int N, T1, F1, T2, F2;
  long long* trace;   // optional [8 workgroups][16 tiles][C2_TRACE] s_memrealtime stamps (diagnostics)
};
constexpr int C2_KT = 10, C2_KF = 5;
// per-tile phase stamps of workgroups 0..7 (wave 0, lane 0): tile start, rows landed, MFMA loop
// done, partial sums reduced, outputs stored, next tile's rows issued (tools/conv_timeline.py)
constexpr int C2_TRACE = 6;
__device__ __forceinline__ void c2_stamp(long long* tr, int it, int k) {
  if (tr != nullptr && blockIdx.x < 8 && threadIdx.x == 0 && it < 16)
    tr[((int)blockIdx.x * 16 + it) * C2_TRACE + k] = __builtin_amdgcn_s_memrealtime();
}
constexpr int PR = 80;                           // LDS bytes per position row (64 data + 16 pad; dgrad)
constexpr int C2F_KPW = 25;                      // k-steps per wave
constexpr int C2F_PL = 80;                       // positions per plane (F1 <= 80)
constexpr int C2F_BUF = (C2_KT * 4 * C2F_PL + 20) * 16;   // 40 planes + the last plane's overrun
// after the MFMA loop the row buffer is scratch: 36 partial-sum slots (wave -> owner, m) of
// 64 f32x4, then the bf16 output row
constexpr int C2F_STG = 36 * 64 * 16;
constexpr int C2F_SMEM = C2F_BUF;
static_assert(C2F_STG + 32 * MT * 64 <= C2F_BUF, "partial sums and the output row fit in the row buffer");
static_assert(C2F_SMEM >= 32 * 16 * C2_KT * C2_KF * 2, "one ci half of the weights is staged through LDS");

template <int S0>
__device__ __forceinline__ void conv2_fwd_body(const Conv2Fwd& a);

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv2_fwd_kernel(Conv2Fwd a) {
  DS2_DCHECK(a.T2 == (a.T1 - C2_KT) / 2 + 1 && a.F2 == a.F1 - 4 && a.F1 <= C2F_PL && a.F1 >= 5);
  switch (uni(threadIdx.x >> 6)) {                   // k-step s = kt * 10 + kf * 2 + ci-half
    case 0: conv2_fwd_body<0>(a); break;
    case 1: conv2_fwd_body<C2F_KPW>(a); break;
    case 2: conv2_fwd_body<2 * C2F_KPW>(a); break;
    default: conv2_fwd_body<3 * C2F_KPW>(a); break;
  }
}

// S0: the wave's first k-step (compile-time, so every LDS offset of the loop is an immediate)
template <int S0>
__device__ __forceinline__ void conv2_fwd_body(const Conv2Fwd& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int w = S0 / C2F_KPW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int hi = lane >> 5, col = lane & 31;
  unsigned char* const buf = smem;
  f32x4* red = (f32x4*)smem;                                         // [36 slots][64] after the loop
  unsigned short* stg = (unsigned short*)(smem + C2F_STG);          // [F2][32] bf16 output row

  // weights -> VGPR fragments through LDS, one ci half at a time, as the image [16 ci][32 co][50]
  // (dword copies; consecutive co 100 B apart, so the 16-bit gathers are conflict-free)
  bf16x8 bfr[C2F_KPW];
  {
    const unsigned short* wl = (const unsigned short*)smem;
    const unsigned* wsrc = (const unsigned*)a.w;                     // [32 co][32 ci][25 dwords]
    for (int hh = 0; hh < 2; ++hh) {
      for (int d = tid; d < 32 * 16 * 25; d += 256) {
        const int co = d / 400, rem = d - co * 400, ci = rem / 25, e = rem - ci * 25;
        ((unsigned*)smem)[(ci * 32 + co) * 25 + e] = wsrc[(co * 32 + 16 * hh + ci) * 25 + e];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < C2F_KPW; ++i) {
        const int s = S0 + i;
        if ((s & 1) != hh) continue;
        const int kt = s / 10, kf = (s % 10) >> 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) bfr[i][j] = (short)wl[((8 * hi + j) * 32 + col) * 50 + kt * C2_KF + kf];
      }
      __syncthreads();
    }
  }
  const float bco = a.bias ? a.bias[col] : 0.f;
  const int ntiles = a.N * a.T2;
  const int F1 = a.F1;
  const int X = (gridDim.x % 8 == 0) ? 8 : 1;
  const int per = (int)gridDim.x / X, xi = (int)blockIdx.x % X, wi = (int)blockIdx.x / X;
  const int t_lo = (int)((long long)ntiles * xi / X), t_hi = (int)((long long)ntiles * (xi + 1) / X);

  // stage input rows 2 t2 .. 2 t2 + 9: plane p = (row p >> 2, 16-B channel chunk p & 3), round r
  // = positions 64 r + lane (F1 in (64, 80]: 2 rounds; narrower rows leave round 1 empty and the
  // positions past F1 unstaged). Wave w issues rounds k = w + 4 i of the
  // 80, i.e. planes (w >> 1) + 2 i in round w & 1: every offset but the tile base is a constant.
  constexpr int R = w & 1;
  const bool on = 64 * R + lane < F1;
  auto issue = [&](int t) {
    const int n = t / a.T2, t2 = t - n * a.T2;
    const bf16_t* base = a.x + ((size_t)n * a.T1 + 2 * t2) * F1 * CC + (64 * R + lane) * CC;
    if (on) {
#pragma unroll
      for (int i = 0; i < 20; ++i) {
        const int p = (w >> 1) + 2 * i;
        glds16(base + (size_t)(p >> 2) * F1 * CC + (p & 3) * 8, buf + (p * C2F_PL + 64 * R) * 16);
      }
    }
  };
  const unsigned char* const lbase = buf + col * 16 + hi * C2F_PL * 16;
  auto ldA = [&](int i, bf16x8 (&dst)[MT]) {
    const int s = S0 + i;
    const int kt = s / 10, kf = (s % 10) >> 1;
    const int off = ((kt * 4 + 2 * (s & 1)) * C2F_PL + kf) * 16;       // constant
#pragma unroll
    for (int m = 0; m < MT; ++m) dst[m] = *(const bf16x8*)(lbase + off + m * 32 * 16);
  };

  float ssum = 0.f, ssq = 0.f;
  int it = 0;
  if (t_lo + wi < t_hi) issue(t_lo + wi);
  for (int tile = t_lo + wi; tile < t_hi; tile += per, ++it) {
    const int n = tile / a.T2, t2 = tile - n * a.T2;
    c2_stamp(a.trace, it, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // this tile's rows are in buf
    c2_stamp(a.trace, it, 1);
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x16){};
    bf16x8 af[2][MT];
    ldA(0, af[0]);
#pragma unroll
    for (int i = 0; i < C2F_KPW; ++i) {
      if (i + 1 < C2F_KPW) ldA(i + 1, af[(i + 1) & 1]);
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = mfma32(af[i & 1][m], bfr[i], acc[m]);
    }
    // reduce-scatter: wave w owns accumulator group r4 = w of every m (output rows 32 m + 8 w +
    // 4 hi + 0..3); slot (src, owner rank, m) with the owner's rank among src's 3 partners
    c2_stamp(a.trace, it, 2);
    lds_barrier();                                     // every MFMA read of buf done
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (o == w) continue;
      const int rk = o - (o > w ? 1 : 0);
#pragma unroll
      for (int m = 0; m < MT; ++m)
        red[((w * 3 + rk) * MT + m) * 64 + lane] =
            (f32x4){acc[m][4 * o], acc[m][4 * o + 1], acc[m][4 * o + 2], acc[m][4 * o + 3]};
    }
    lds_barrier();
    f32x4 own[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
      own[m] = (f32x4){acc[m][4 * w], acc[m][4 * w + 1], acc[m][4 * w + 2], acc[m][4 * w + 3]};
#pragma unroll
    for (int src = 0; src < 4; ++src) {
      if (src == w) continue;
      const int rk = w - (w > src ? 1 : 0);
#pragma unroll
      for (int m = 0; m < MT; ++m) own[m] += red[((src * 3 + rk) * MT + m) * 64 + lane];
    }
    c2_stamp(a.trace, it, 3);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int f2 = 32 * m + 8 * w + 4 * hi + e;
        // every m: with F2 < 64 the positions F2..63 hold sums over unstaged LDS, and they must
        // not enter the statistics (the row copy below never stored them)
        if (f2 < a.F2) {
          const bf16_t b = f2bf(own[m][e] + bco);
          stg[f2 * CC + col] = b;
          const float vb = bf2f(b);
          ssum += vb;
          ssq += vb * vb;
        }
      }
    lds_barrier();
    {
      i32x4* dst = (i32x4*)(a.y + ((size_t)n * a.T2 + t2) * a.F2 * CC);
      for (int q = tid; q < a.F2 * 4; q += 256) dst[q] = ((const i32x4*)stg)[q];
    }
    c2_stamp(a.trace, it, 4);
    lds_barrier();                                     // the row copy's reads done: buf is free
    if (tile + per < t_hi) issue(tile + per);
    c2_stamp(a.trace, it, 5);
  }
  __syncthreads();
  write_stats(ssum, ssq, (float*)red, 4, a.part);
}

// =====================================================================================
// conv2 data gradient: dx[n][t1][f1][ci] = sum dy[n][(t1-kt)/2][f1-kf][co] w[co][ci][kt][kf]
// =====================================================================================
// A tile is the output row pair (2u, 2u+1); parity p = t1 & 1 reads dy rows u-ai (ai = 0..4)
// with kt = 2 ai + p. Wave w computes parity w & 1 over half (w >> 1) of that parity's 50
// (ai, kf, co-half) k-steps, its 25 weight fragments in VGPRs for the whole launch; waves 2, 3
// hand their partial sums to waves 0, 1 through LDS (one round), which store. Two ~64-KB
// workgroups per CU, so one's reduction and staging overlap the other's MFMA loop. Each dy row
// lands by global_load_lds in an LDS slot of C2D_PR zero-padded 80-B position rows (positions
// -4 .. 95; the pads are zeroed once and never written), so an A fragment address is one lane
// base + a wave-uniform offset and out-of-range positions read zeros. Tiles go to XCDs in
// contiguous ranges, so the 4 rows neighbouring tiles share are L2 hits. With bn set, waves 0 / 1
// also read conv1's output at the positions they store and accumulate conv1's BatchNorm-backward
// sums (each lane owns one channel), so that reduction pass never re-reads dx.
struct Conv2Dgrad {
  const bf16_t* dy;   // [N][T2][F2][32]
  const bf16_t* w;    // [32][32][10][5]
  bf16_t* dx;         // [N][T1][F1][32]
  int N, T1, F1, T2, F2;
  // optional: conv1's BatchNorm-backward sums over the stored dx (see bn_cl_bwd_reduce_kernel):
  // y1 = conv1's output [N][T1][F1][32], part [grid][32][2] = (sum dz*m, sum dz*m*xhat)
  const bf16_t* y1;
  const float *mean, *invstd, *gamma, *beta;
  float* part;
  long long* trace;   // optional phase stamps, as Conv2Fwd::trace
};
constexpr int C2D_KPW = 25;                      // k-steps per wave (one parity's 50 in halves)
constexpr int C2D_PR = 4 + 32 * MT;              // LDS position rows per dy row (positions -4 .. 95)
constexpr int C2D_BUF = 5 * C2D_PR * PR;         // 40000 B
constexpr int C2D_RED = 4 * 6 * 64 * 16;        // [wave][6 groups it hands over][64] f32x4
constexpr int C2D_ROW = 80 * 64;                 // one bf16 output row [F1 <= 80][32]
constexpr int C2D_SMEM = C2D_BUF + C2D_RED + 2 * C2D_ROW;
static_assert(C2D_SMEM >= 16 * CC * C2_KT * C2_KF * 2, "one co half of the weights is staged through LDS");

template <int W>
__device__ __forceinline__ void conv2_dgrad_body(const Conv2Dgrad& a);

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv2_dgrad_kernel(Conv2Dgrad a) {
  DS2_DCHECK(a.F2 <= 32 * MT - 4 && a.F1 == a.F2 + 4 && a.F1 > 64 && a.F1 <= 80);
  switch (uni(threadIdx.x >> 6)) {
    case 0: conv2_dgrad_body<0>(a); break;
    case 1: conv2_dgrad_body<1>(a); break;
    case 2: conv2_dgrad_body<2>(a); break;
    default: conv2_dgrad_body<3>(a); break;
  }
}

// W: the wave (parity W & 1, K half W >> 1), compile-time so every LDS offset is an immediate
template <int W>
__device__ __forceinline__ void conv2_dgrad_body(const Conv2Dgrad& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int w = W, par = W & 1, kh = W >> 1, S0 = kh * C2D_KPW;   // k-step s = ai*10 + kf*2 + co-half
  const int tid = threadIdx.x, lane = tid & 63;
  const int hi = lane >> 5, col = lane & 31;
  unsigned char* const buf = smem;
  f32x4* red = (f32x4*)(smem + C2D_BUF);
  unsigned short* stg = (unsigned short*)(smem + C2D_BUF + C2D_RED + par * C2D_ROW);   // this parity's row

  // weights -> VGPR fragments through LDS, one co half (51.2 KB of OIHW) at a time: coalesced
  // 16-B global loads, then 16-bit LDS gathers
  bf16x8 bfr[C2D_KPW];
  {
    const unsigned short* wl = (const unsigned short*)smem;
    for (int hh = 0; hh < 2; ++hh) {
      const i32x4* src = (const i32x4*)(a.w + (size_t)hh * 16 * CC * C2_KT * C2_KF);
      for (int o = tid; o < 16 * CC * C2_KT * C2_KF / 8; o += 256) ((i32x4*)smem)[o] = src[o];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < C2D_KPW; ++i) {
        const int s = S0 + i;
        if ((s & 1) != hh) continue;
        const int ai = s / 10, kf = (s % 10) >> 1;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          bfr[i][j] = (short)wl[(((8 * hi + j) * CC + col) * C2_KT + 2 * ai + par) * C2_KF + kf];
      }
      __syncthreads();
    }
  }
  for (int o = tid * 16; o < C2D_BUF; o += 256 * 16) *(i32x4*)(buf + o) = (i32x4){0, 0, 0, 0};

  const int U = (a.T1 + 1) >> 1;
  const int ntiles = a.N * U;
  const int F2 = a.F2, nq = 5 * F2;                        // 16-B chunks per dy row (<= 6 rounds)
  // tiles: X contiguous ranges (one per XCD when the grid is a multiple of 8; workgroup b runs
  // on XCD b % 8), dealt round-robin to that XCD's workgroups
  const int X = (gridDim.x % 8 == 0) ? 8 : 1;
  const int per = (int)gridDim.x / X, xi = (int)blockIdx.x % X, wi = (int)blockIdx.x / X;
  const int t_lo = (int)((long long)ntiles * xi / X), t_hi = (int)((long long)ntiles * (xi + 1) / X);

  // stage dy rows u-4..u of tile t into the 5 slots (rows outside [0, T2) are clamped: their
  // k-steps are skipped); a lane's 16-B chunk q of a slot is position q / 5, chunk q % 5, and
  // chunk 4 (the row's pad column, never read) repeats chunk 3. Wave w issues rounds k = w + 4 i
  // of the 30 (slot k / 6, round k % 6): compile-time slot and LDS offset.
  auto issue = [&](int t) {
    const int n = t / U, u = t - n * U;
    const bf16_t* base = a.dy + (size_t)n * a.T2 * F2 * CC;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = w + 4 * i;
      if (k < 30) {
        const int j = k / 6, r = k % 6;
        const int q = 64 * r + lane;
        if (q < nq) {
          const int pos = (q * 52429) >> 18, c = min(q - 5 * pos, 3);    // q / 5 for q < 2^14
          const int row = min(max(u - 4 + j, 0), a.T2 - 1);
          glds16(base + ((size_t)row * F2 + pos) * CC + c * 8, buf + (j * C2D_PR + 4) * PR + 1024 * r);
        }
      }
    }
  };
  const unsigned char* const lbase = buf + col * PR + hi * 16;
  const bool bn = a.mean != nullptr;
  const float bmu = bn ? a.mean[col] : 0.f, bis = bn ? a.invstd[col] : 0.f;
  const float bg = bn ? a.gamma[col] : 0.f, bbt = bn ? a.beta[col] : 0.f;
  float bs = 0.f, bq = 0.f;
  auto ldA = [&](int i, bf16x8 (&dst)[MT]) {
    const int s = S0 + i;
    const int ai = s / 10, kf = (s % 10) >> 1;
    const int off = ((4 - ai) * C2D_PR + 4 - kf) * PR + (s & 1) * 32;     // >= 0, constant
#pragma unroll
    for (int m = 0; m < MT; ++m) dst[m] = *(const bf16x8*)(lbase + off + m * 32 * PR);
  };

  __syncthreads();                                     // pads zeroed before any staging lands
  int it = 0;
  if (t_lo + wi < t_hi) issue(t_lo + wi);
  for (int tile = t_lo + wi; tile < t_hi; tile += per, ++it) {
    const int n = tile / U, u = tile - n * U;
    c2_stamp(a.trace, it, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // this tile's rows are in buf
    c2_stamp(a.trace, it, 1);
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x16){};
    bf16x8 af[2][MT];
    ldA(0, af[0]);
#pragma unroll
    for (int i = 0; i < C2D_KPW; ++i) {
      if (i + 1 < C2D_KPW) ldA(i + 1, af[(i + 1) & 1]);
      const int t2 = u - (S0 + i) / 10;
      if (t2 >= 0 && t2 < a.T2) {                      // wave-uniform
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = mfma32(af[i & 1][m], bfr[i], acc[m]);
      }
    }
    c2_stamp(a.trace, it, 2);
    // the parity's two K halves reduce-scatter: K half kh owns accumulator groups r4 = 2 kh + j
    // (j = 0, 1) of every m, i.e. output rows 32 m + 8 (2 kh + j) + 4 hi + 0..3, and hands the
    // other two groups to its partner (wave W ^ 2) through red[wave][m][j]
    lds_barrier();                                     // the previous tile's red / row reads done
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int g = 2 * (1 - kh) + j;
        red[((w * MT + m) * 2 + j) * 64 + lane] = (f32x4){acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
      }
    lds_barrier();
    f32x4 own[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int g = 2 * kh + j;
        own[m][j] = (f32x4){acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]} +
                    red[(((w ^ 2) * MT + m) * 2 + j) * 64 + lane];
      }
    c2_stamp(a.trace, it, 3);
    const int t1 = 2 * u + par;
    const bool out = t1 < a.T1;                        // wave-uniform
    const size_t rowoff = ((size_t)n * a.T1 + t1) * a.F1 * CC;
    if (out) {
      // conv1's outputs at the owned positions, loaded before any global store of the tile
      // (one per-lane base, compile-time offsets; the last m-tile clamped to the row)
      unsigned short yv[MT][2][4];
      if (bn) {
        const unsigned short* yb = (const unsigned short*)a.y1 + rowoff + 4 * hi * CC + col;
        const int lastoff = (a.F1 - 1 - 4 * hi) * CC;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int fo = (32 * m + 8 * (2 * kh + j) + e) * CC;
              yv[m][j][e] = m < 2 ? yb[fo] : yb[min(fo, lastoff)];
            }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int f1 = 32 * m + 8 * (2 * kh + j) + 4 * hi + e;
            if (m < 2 || f1 < a.F1) {
              const bf16_t d = f2bf(own[m][j][e]);
              stg[f1 * CC + col] = d;
              if (bn) {
                const float xh = (bf2f(yv[m][j][e]) - bmu) * bis;
                const float zz = xh * bg + bbt;
                const float dd = (zz > 0.f && zz < CLIP) ? bf2f(d) : 0.f;
                bs += dd;
                bq += dd * xh;
              }
            }
          }
    }
    lds_barrier();                                     // both halves of each parity row staged
    if (out) {
      i32x4* dst = (i32x4*)(a.dx + rowoff);
      for (int q = kh * 64 + lane; q < a.F1 * 4; q += 128) dst[q] = ((const i32x4*)stg)[q];
    }
    c2_stamp(a.trace, it, 4);
    // the next tile's rows go out after every LDS access (and conv1 load) of this one: hipcc
    // puts an s_waitcnt vmcnt(0) before any LDS access while LDS-DMA loads are in flight
    if (tile + per < t_hi) issue(tile + per);
    c2_stamp(a.trace, it, 5);
  }
  if (bn) {
    // per-workgroup sums: lanes l, l ^ 32 and all 4 waves share a channel
    bs += __shfl_xor(bs, 32, 64);
    bq += __shfl_xor(bq, 32, 64);
    float* sh = (float*)red;
    __syncthreads();
    if (lane < 32) { sh[(w * 32 + lane) * 2] = bs; sh[(w * 32 + lane) * 2 + 1] = bq; }
    __syncthreads();
    if (tid < 64) a.part[(size_t)blockIdx.x * 64 + tid] = sh[tid] + sh[64 + tid] + sh[128 + tid] + sh[192 + tid];
  }
}

// =====================================================================================
// conv2 weight gradient (per-workgroup fp32 partials in fragment order)
// =====================================================================================
struct Conv2Wgrad {
  const bf16_t* dy;   // [N][T2][F2][32]
  const bf16_t* x;    // z1 [N][T1][F1][32]
  float* part;        // [grid][50][4][64][4]
  int N, T1, F1, T2, F2;
};
constexpr int C2W_PAIRS = C2_KT * C2_KF;   // 50 (kt, kf) output tiles of 32x32
constexpr int C2W_WAVES = 8;
constexpr int C2W_PPW = 7;                 // ceil(50 / 8)

__global__ __launch_bounds__(512) void conv2_wgrad_kernel(Conv2Wgrad a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = uni(tid >> 6);
  const int dyBytes = 80 * 64;
  const int xBytes = (9 * a.F1 + 84) * 64;         // covers row (kt*F1 + pos + kf) for pos < 80
  const int bufBytes = dyBytes + xBytes;
  unsigned char* const buf0 = smem;
  unsigned char* const buf1 = smem + bufBytes;
  // zero the pads that no copy writes: dy positions F2..79, x positions 10*F1 .. 9*F1+83
  for (int b = 0; b < 2; ++b) {
    unsigned char* bb = b ? buf1 : buf0;
    for (int o = a.F2 * 64 + tid * 4; o < dyBytes; o += 512 * 4) *(unsigned*)(bb + o) = 0u;
    for (int o = 10 * a.F1 * 64 + tid * 4; o < xBytes; o += 512 * 4) *(unsigned*)(bb + dyBytes + o) = 0u;
  }
  const int ntiles = a.N * a.T2;
  const int dyChunks = a.F2 * 4, xChunks = 10 * a.F1 * 4;
  auto issue = [&](int t, unsigned char* dst) {
    const int n = t / a.T2, t2 = t - n * a.T2;
    const unsigned char* sdy = (const unsigned char*)(a.dy + ((size_t)n * a.T2 + t2) * a.F2 * CC);
    const unsigned char* sx = (const unsigned char*)(a.x + ((size_t)n * a.T1 + 2 * t2) * a.F1 * CC);
    for (int p0 = w * 64; p0 < dyChunks; p0 += 512) {
      const int p = p0 + lane;
      if (p < dyChunks) glds16(sdy + (size_t)p * 16, dst + (size_t)p0 * 16);
    }
    for (int p0 = w * 64; p0 < xChunks; p0 += 512) {
      const int p = p0 + lane;
      if (p < xChunks) glds16(sx + (size_t)p * 16, dst + dyBytes + (size_t)p0 * 16);
    }
  };
  // transposed-read lane geometry
  const int g = lane >> 4, h = g >> 1, cb = (g & 1) * 16, q = (lane & 15) >> 2, pp = lane & 3;
  const unsigned lofs = (unsigned)((8 * h + q) * 64 + (cb + 4 * pp) * 2);
  const int npairs = (w < C2W_PAIRS - 6 * C2W_WAVES) ? 7 : 6;   // waves 0,1 take pairs 48,49

  f32x16 acc[C2W_PPW];
#pragma unroll
  for (int i = 0; i < C2W_PPW; ++i) acc[i] = (f32x16){};
  __syncthreads();
  int it = 0;
  if ((int)blockIdx.x < ntiles) issue(blockIdx.x, buf0);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, ++it) {
    const unsigned char* cur = (it & 1) ? buf1 : buf0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x, (it & 1) ? buf0 : buf1);
    const unsigned char* xs = cur + dyBytes;
#pragma unroll
    for (int kk = 0; kk < 5; ++kk) {
      const unsigned k0 = (unsigned)(16 * kk) * 64u;
      const bf16x8 av = cat8(tr_read(cur + k0 + lofs), tr_read(cur + k0 + lofs + 4 * 64));
#pragma unroll
      for (int i = 0; i < C2W_PPW; ++i) {
        if (i < npairs) {
          const int P = w + C2W_WAVES * i;
          const int kt = P / 5, kf = P - 5 * (P / 5);
          const unsigned rb = (unsigned)(kt * a.F1 + kf) * 64u + k0 + lofs;
          const bf16x8 bv = cat8(tr_read(xs + rb), tr_read(xs + rb + 4 * 64));
          acc[i] = mfma32(av, bv, acc[i]);
        }
      }
    }
  }
  f32x4* out = (f32x4*)(a.part + (size_t)blockIdx.x * C2W_PAIRS * 1024);
#pragma unroll
  for (int i = 0; i < C2W_PPW; ++i) {
    if (i < npairs) {
      const int P = w + C2W_WAVES * i;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        out[(P * 4 + r4) * 64 + lane] = (f32x4){acc[i][4 * r4], acc[i][4 * r4 + 1], acc[i][4 * r4 + 2], acc[i][4 * r4 + 3]};
    }
  }
}

// sum of per-workgroup partials (fragment order) -> dw in OIHW, KIND 0: conv2 [32][32][10][5],
// KIND 1: conv1 [32][1][20][5]. A block owns 256 consecutive elements (64 f32x4 columns)
// and 4 interleaved groups of partials, so every thread keeps several 16-B loads in flight.
template <int KIND>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int nb, int E,
                                                           float* __restrict__ dw) {
  __shared__ f32x4 sh[4][64];
  const int tid = threadIdx.x, g = tid >> 6, l = tid & 63;
  const int e4 = blockIdx.x * 64 + l, E4 = E >> 2;
  const f32x4* p4 = (const f32x4*)part;
  f32x4 s0 = {}, s1 = {};
  int b = g;
  for (; b + 4 < nb; b += 8) {
    s0 += p4[(size_t)b * E4 + e4];
    s1 += p4[(size_t)(b + 4) * E4 + e4];
  }
  if (b < nb) s0 += p4[(size_t)b * E4 + e4];
  sh[g][l] = s0 + s1;
  __syncthreads();
  if (g != 0) return;
  const f32x4 v = sh[0][l] + sh[1][l] + sh[2][l] + sh[3][l];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = e4 * 4 + j;
    const int P = e >> 10, rem = e & 1023, r4 = rem >> 8, ln = (rem >> 2) & 63;
    const int row = (rem & 3) + 8 * r4 + 4 * (ln >> 5), c = ln & 31;
    if (KIND == 0) {
      const int kt = P / 5, kf = P % 5;
      dw[((row * CC + c) * C2_KT + kt) * C2_KF + kf] = v[j];
    } else {
      const int kt = 4 * P + (c >> 3), kf = c & 7;
      if (kf < 5) dw[(row * 20 + kt) * 5 + kf] = v[j];
    }
  }
}

// =====================================================================================
// conv1 forward (C_in = 1)
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
    i32x4* dst = (i32x4*)(a.y + ((size_t)n * a.T1 + t1) * a.F1 * CC);
    for (int q = lane; q < a.F1 * 4; q += 64) dst[q] = ((const i32x4*)yl)[q];
  }
  write_stats(ssum, ssq, statsh, 4, a.part);
}

// =====================================================================================
// conv1 weight gradient
// =====================================================================================
struct Conv1Wgrad {
  const bf16_t* dy;   // [N][T1][F1][32], or null with bn.dz: dy computed while staging
  const bf16_t* x;    // [N][T][F0]
  float* part;        // [grid][5][4][64][4]
  int N, T, F0, T1, F1;
  // optional: conv1's BatchNorm backward applied in the staging (bn_cl_bwd_apply_kernel's
  // arithmetic, so dy is bitwise the same): dz = dL/d(clip(BN(y1))) [N][T1][F1][32], y1
  const bf16_t *dz, *y1;
  const float *mean, *invstd, *gamma, *beta, *dbeta, *dgamma;
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
  const int g = lane >> 4, h = g >> 1, cb = (g & 1) * 16, q = (lane & 15) >> 2, pp = lane & 3;
  const unsigned lofs = (unsigned)((8 * h + q) * 64 + (cb + 4 * pp) * 2);
  const int bkt = col >> 3, bkf = col & 7;

  // fused BN backward: a thread's chunks all hold channels 8 (tid & 3) .. + 7 (256 and 320 are
  // multiples of 4), so their constants stay in registers
  const bool bn = a.dz != nullptr;
  float bmu[8], bis[8], bg[8], bbt[8], bmdb[8], bmdg[8];
  if (bn) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = (tid & 3) * 8 + j;
      bmu[j] = a.mean[c]; bis[j] = a.invstd[c]; bg[j] = a.gamma[c]; bbt[j] = a.beta[c];
      bmdb[j] = a.dbeta[c] / a.M; bmdg[j] = a.dgamma[c] / a.M;
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
          const bf16x8 y = *(const bf16x8*)(a.y1 + off), d = *(const bf16x8*)(a.dz + off);
          bf16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xh = (bf2f((bf16_t)y[j]) - bmu[j]) * bis[j];
            const float zz = xh * bg[j] + bbt[j];
            const float dd = (zz > 0.f && zz < CLIP) ? bf2f((bf16_t)d[j]) : 0.f;
            o[j] = (short)f2bf(bg[j] * bis[j] * (dd - bmdb[j] - xh * bmdg[j]));
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
        const unsigned char* ab = dys + (w * 80 + k0) * 64 + lofs;
        const bf16x8 av = cat8(tr_read(ab), tr_read(ab + 4 * 64));
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
    for (int r4 = 0; r4 < 4; ++r4)
      red[((w * 5 + nt) * 4 + r4) * 64 + lane] =
          (f32x4){acc[nt][4 * r4], acc[nt][4 * r4 + 1], acc[nt][4 * r4 + 2], acc[nt][4 * r4 + 3]};
  __syncthreads();
  f32x4* out = (f32x4*)(a.part + (size_t)blockIdx.x * 5 * 1024);
  for (int e = tid; e < 5 * 4 * 64; e += 256) {
    f32x4 v = red[e];
    for (int wv = 1; wv < 4; ++wv) v += red[wv * 5 * 4 * 64 + e];
    out[e] = v;
  }
}

// =====================================================================================
// channels-last BatchNorm (+ clipped ReLU)
// =====================================================================================
// part [nb][32][2] -> mean / invstd (+ running stats, unbiased variance, momentum)
__global__ __launch_bounds__(256) void bn_cl_finalize_kernel(const float* __restrict__ part, int nb, double M,
                                                             float eps, float* mean, float* invstd, float* run_mean,
                                                             float* run_var, float momentum) {
  __shared__ double sh[2][4];
  const int c = blockIdx.x, tid = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int b = tid; b < nb; b += 256) {
    s += part[((size_t)b * 32 + c) * 2 + 0];
    q += part[((size_t)b * 32 + c) * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if ((tid & 63) == 0) { sh[0][tid >> 6] = s; sh[1][tid >> 6] = q; }
  __syncthreads();
  if (tid == 0) {
    s = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    q = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    const double mu = s / M;
    double var = q / M - mu * mu;
    if (var < 0) var = 0;
    if (mean) mean[c] = (float)mu;
    if (invstd) invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) {
      const double unb = M > 1 ? var * M / (M - 1) : var;
      run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * mu);
      run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
    }
  }
}

// z = clip(y * sc + sh) elementwise, channels-last in and out (8 channels per thread)
__global__ __launch_bounds__(256) void bn_cl_apply_kernel(const bf16_t* __restrict__ y, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, bf16_t* __restrict__ z,
                                                          long long nchunks) {
  const int c0 = (threadIdx.x & 3) * 8;     // 256 % 4 == 0: a thread keeps its channel octet
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = invstd[c0 + j] * gamma[c0 + j];
    sh[j] = beta[c0 + j] - mean[c0 + j] * sc[j];
  }
  for (long long ch = (long long)blockIdx.x * 256 + threadIdx.x; ch < nchunks; ch += (long long)gridDim.x * 256) {
    const bf16x8 v = *(const bf16x8*)(y + ch * 8);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(fminf(fmaxf(bf2f((bf16_t)v[j]) * sc[j] + sh[j], 0.f), CLIP));
    *(bf16x8*)(z + ch * 8) = o;
  }
}

// rows (n, t) of F positions x 32 channels; time-major output out[t][n][c*F + f]
__global__ __launch_bounds__(256) void bn_cl_apply_tmaj_kernel(const bf16_t* __restrict__ y,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               bf16_t* __restrict__ out, int N, int T, int F) {
  __shared__ bf16_t tr[32 * 97];            // [c][f], stride F+? (F <= 96)
  const int tid = threadIdx.x, c0 = (tid & 3) * 8;
  const int stride = F + 1;
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = invstd[c0 + j] * gamma[c0 + j];
    sh[j] = beta[c0 + j] - mean[c0 + j] * sc[j];
  }
  for (int row = blockIdx.x; row < N * T; row += gridDim.x) {
    const int n = row / T, t = row - n * T;
    const bf16_t* yr = y + (size_t)row * F * CC;
    __syncthreads();
    for (int ch = tid; ch < F * 4; ch += 256) {
      const int f = ch >> 2;
      const bf16x8 v = *(const bf16x8*)(yr + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        tr[(c0 + j) * stride + f] = f2bf(fminf(fmaxf(bf2f((bf16_t)v[j]) * sc[j] + sh[j], 0.f), CLIP));
    }
    __syncthreads();
    bf16_t* orow = out + ((size_t)t * N + n) * CC * F;
    for (int e = tid; e < CC * F; e += 256) {
      const int c = e / F, f = e - c * F;
      orow[e] = tr[c * stride + f];
    }
  }
}

// backward reduce over rows: sums of dz*m and dz*m*xhat per channel; dz either channels-
// last (tmaj == 0) or time-major [T][N][c*F + f] (tmaj == 1)
__global__ __launch_bounds__(256) void bn_cl_bwd_reduce_kernel(const bf16_t* __restrict__ dz,
                                                               const bf16_t* __restrict__ y,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* part,
                                                               int N, int T, int F, int tmaj,
                                                               bf16_t* __restrict__ dz_cl) {
  __shared__ float red[4 * 4 * 8];       // [wave][channel octet][8] per pass
  const int tid = threadIdx.x, c0 = (tid & 3) * 8;
  float mu[8], is[8], g[8], bt[8], s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[c0 + j]; is[j] = invstd[c0 + j]; g[j] = gamma[c0 + j]; bt[j] = beta[c0 + j];
    s[j] = 0.f; q[j] = 0.f;
  }
  auto acc8 = [&](const bf16x8 v, const bf16x8 d) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (bf2f((bf16_t)v[j]) - mu[j]) * is[j];
      const float zz = xh * g[j] + bt[j];
      const float dd = (zz > 0.f && zz < CLIP) ? bf2f((bf16_t)d[j]) : 0.f;
      s[j] += dd;
      q[j] += dd * xh;
    }
  };
  if (!tmaj) {
    // channels-last: one flat stream of 16-B chunks whose channel octet is (chunk & 3) = (tid & 3)
    // (the grid stride is a multiple of 4), 4 chunks of each operand in flight per thread
    const long long total = (long long)N * T * F * 4, step = (long long)gridDim.x * 256;
    const bf16x8* y8 = (const bf16x8*)y;
    const bf16x8* d8 = (const bf16x8*)dz;
    long long e = (long long)blockIdx.x * 256 + tid;
    for (; e + 3 * step < total; e += 4 * step) {
      bf16x8 v[4], d[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] = y8[e + k * step]; d[k] = d8[e + k * step]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc8(v[k], d[k]);
    }
    for (; e < total; e += step) acc8(y8[e], d8[e]);
  } else {
    // time-major dz [T][N][c * F + f]: chunk e of the channels-last stream is (row = n * T + t,
    // position f, channels 8 (e & 3) ..): its 8 dz values are one time-major row's elements
    // c * F + f (a 2-byte gather from one cache-resident row), and the channels-last copy the
    // apply pass reads is written as one 16-B chunk. No LDS and no barriers, so the kernel
    // streams beside the grouped weight-gradient GEMM in the step's tail.
    const long long total = (long long)N * T * F * 4, step = (long long)gridDim.x * 256;
    const bf16x8* y8 = (const bf16x8*)y;
    const int c0 = (tid & 3) * 8;
    for (long long e = (long long)blockIdx.x * 256 + tid; e < total; e += step) {
      const long long rowf = e >> 2;
      const int row = (int)(rowf / F), f = (int)(rowf - (long long)row * F);
      const int n = row / T, t = row - n * T;
      const bf16_t* dr = dz + ((size_t)t * N + n) * CC * F + f;
      bf16x8 d;
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = (short)dr[(c0 + j) * F];
      if (dz_cl != nullptr) ((bf16x8*)dz_cl)[e] = d;
      acc8(y8[e], d);
    }
  }
  // reduce over the 64 threads sharing a channel octet (tid & 3)
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    float* v = pass == 0 ? s : q;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // threads with equal (tid & 3): lanes differ in bits 2..5 within a wave
      float x = v[j];
      x += __shfl_xor(x, 4, 64);
      x += __shfl_xor(x, 8, 64);
      x += __shfl_xor(x, 16, 64);
      x += __shfl_xor(x, 32, 64);
      v[j] = x;
    }
    __syncthreads();
    if ((tid & 63) < 4) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[((tid >> 6) * 4 + (tid & 3)) * 8 + j] = v[j];
    }
    __syncthreads();
    if (tid < 32) {
      const int oc = tid >> 3, j = tid & 7;    // channel = oc*8 + j
      float x = 0.f;
      for (int wv = 0; wv < 4; ++wv) x += red[(wv * 4 + oc) * 8 + j];
      part[((size_t)blockIdx.x * 32 + tid) * 2 + pass] = x;
    }
  }
}

// part [nb][32][2] -> dbeta, dgamma (fp32)
__global__ __launch_bounds__(256) void bn_cl_bwd_finalize_kernel(const float* __restrict__ part, int nb,
                                                                 float* dbeta, float* dgamma) {
  __shared__ double sh[2][4];
  const int c = blockIdx.x, tid = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int b = tid; b < nb; b += 256) {
    s += part[((size_t)b * 32 + c) * 2 + 0];
    q += part[((size_t)b * 32 + c) * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if ((tid & 63) == 0) { sh[0][tid >> 6] = s; sh[1][tid >> 6] = q; }
  __syncthreads();
  if (tid == 0) {
    dbeta[c] = (float)(sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
    dgamma[c] = (float)(sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
  }
}

// dy = gamma*invstd*(dz*m - dbeta/M - xhat*dgamma/M), channels-last out. dz may alias dy
// (each thread reads and writes the same 16 B), so neither is __restrict__.
__global__ __launch_bounds__(256) void bn_cl_bwd_apply_kernel(const bf16_t* dz,
                                                              const bf16_t* __restrict__ y,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ dbeta,
                                                              const float* __restrict__ dgamma,
                                                              bf16_t* dy, int N, int T, int F) {
  const int tid = threadIdx.x, c0 = (tid & 3) * 8;
  const float M = (float)N * T * F;
  float mu[8], is[8], g[8], bt[8], mdb[8], mdg[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[c0 + j]; is[j] = invstd[c0 + j]; g[j] = gamma[c0 + j]; bt[j] = beta[c0 + j];
    mdb[j] = dbeta[c0 + j] / M; mdg[j] = dgamma[c0 + j] / M;
  }
  auto one = [&](const bf16x8 v, const bf16x8 d) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (bf2f((bf16_t)v[j]) - mu[j]) * is[j];
      const float zz = xh * g[j] + bt[j];
      const float dd = (zz > 0.f && zz < CLIP) ? bf2f((bf16_t)d[j]) : 0.f;
      o[j] = (short)f2bf(g[j] * is[j] * (dd - mdb[j] - xh * mdg[j]));
    }
    return o;
  };
  // one flat stream of 16-B chunks, channel octet (chunk & 3) = (tid & 3); 4 in flight
  const long long total = (long long)N * T * F * 4, step = (long long)gridDim.x * 256;
  const bf16x8* y8 = (const bf16x8*)y;
  const bf16x8* d8 = (const bf16x8*)dz;
  bf16x8* o8 = (bf16x8*)dy;
  long long e = (long long)blockIdx.x * 256 + tid;
  for (; e + 3 * step < total; e += 4 * step) {
    bf16x8 v[4], d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = y8[e + k * step]; d[k] = d8[e + k * step]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) o8[e + k * step] = one(v[k], d[k]);
  }
  for (; e < total; e += step) o8[e] = one(y8[e], d8[e]);
}

template <typename K>
int set_smem(K kernel, size_t bytes) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}

int shape_ok(int T1, int F1, int T2, int F2) {
  if (F1 < 5 || F1 > 80 || F2 != F1 - 4) return -40;   // LDS (10*F1*80 + 96 KiB) and staging capacity
  if (T1 < 10 || T2 != (T1 - 10) / 2 + 1) return -41;
  return 0;
}

}  // namespace

extern "C" {

size_t ds2_conv2_fwd_smem(int) { return (size_t)C2F_SMEM; }
size_t ds2_conv2_dgrad_smem(int) { return (size_t)C2D_SMEM; }
size_t ds2_conv2_wgrad_smem(int F1) { return (size_t)2 * (80 * 64 + (9 * F1 + 84) * 64); }
long long ds2_conv2_wgrad_part_floats(int grid) { return (long long)grid * C2W_PAIRS * 1024; }
long long ds2_conv1_wgrad_part_floats(int grid) { return (long long)grid * 5 * 1024; }
int ds2_conv1_fwd_grid(int N, int T1) { return N * ((T1 + C1_ROWS - 1) / C1_ROWS); }

int ds2_conv2_fwd(const void* x, const void* w, const float* bias, void* y, float* part, int grid, int N, int T1,
                  int F1, int T2, int F2, long long* trace, hipStream_t st) {
  if (int e = shape_ok(T1, F1, T2, F2)) return e;
  const size_t smem = ds2_conv2_fwd_smem(F1);
  DS2_HIP_CHECK((hipError_t)set_smem(conv2_fwd_kernel, smem));
  Conv2Fwd a{(const bf16_t*)x, (const bf16_t*)w, bias, (bf16_t*)y, part, N, T1, F1, T2, F2, trace};
  hipLaunchKernelGGL(conv2_fwd_kernel, dim3(grid), dim3(256), smem, st, a);
  return (int)hipGetLastError();
}

int ds2_conv2_dgrad(const void* dy, const void* w, void* dx, int grid, int N, int T1, int F1, int T2, int F2,
                    const DS2Conv2DgradBn* bn, long long* trace, hipStream_t st) {
  if (int e = shape_ok(T1, F1, T2, F2)) return e;
  if (F1 <= 64) return -42;                              // rows 0..63 are stored unchecked
  const size_t smem = ds2_conv2_dgrad_smem(F2);
  DS2_HIP_CHECK((hipError_t)set_smem(conv2_dgrad_kernel, smem));
  Conv2Dgrad a{(const bf16_t*)dy, (const bf16_t*)w, (bf16_t*)dx, N, T1, F1, T2, F2,
               bn ? (const bf16_t*)bn->y1 : nullptr, bn ? bn->mean : nullptr, bn ? bn->invstd : nullptr,
               bn ? bn->gamma : nullptr, bn ? bn->beta : nullptr, bn ? bn->part : nullptr, trace};
  hipLaunchKernelGGL(conv2_dgrad_kernel, dim3(grid), dim3(256), smem, st, a);
  return (int)hipGetLastError();
}

int ds2_conv2_wgrad(const void* dy, const void* x, float* part, int grid, float* dw, int N, int T1, int F1, int T2,
                    int F2, hipStream_t st) {
  if (int e = shape_ok(T1, F1, T2, F2)) return e;
  const size_t smem = ds2_conv2_wgrad_smem(F1);
  DS2_HIP_CHECK((hipError_t)set_smem(conv2_wgrad_kernel, smem));
  Conv2Wgrad a{(const bf16_t*)dy, (const bf16_t*)x, part, N, T1, F1, T2, F2};
  hipLaunchKernelGGL(conv2_wgrad_kernel, dim3(grid), dim3(512), smem, st, a);
  hipLaunchKernelGGL(wgrad_reduce_kernel<0>, dim3(C2W_PAIRS * 1024 / 256), dim3(256), 0, st, part, grid,
                     C2W_PAIRS * 1024, dw);
  return (int)hipGetLastError();
}

int ds2_conv1_fwd(const void* x, const void* w, const float* bias, void* y, float* part, int N, int T, int F0,
                  int T1, int F1, hipStream_t st) {
  if (F1 > 96 || F1 != (F0 - 5) / 2 + 1 || T1 != (T - 20) / 2 + 1 || T1 < 1) return -42;
  Conv1Fwd a{(const bf16_t*)x, (const bf16_t*)w, bias, (bf16_t*)y, part, N, T, F0, T1, F1};
  hipLaunchKernelGGL(conv1_fwd_kernel, dim3(ds2_conv1_fwd_grid(N, T1)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int ds2_conv1_wgrad(const void* dy, const void* x, float* part, int grid, float* dw, int N, int T, int F0, int T1,
                    int F1, const DS2Conv1WgradBn* bn, hipStream_t st) {
  if (F1 > 80 || F1 != (F0 - 5) / 2 + 1 || T1 != (T - 20) / 2 + 1 || T1 < 1) return -43;
  if ((dy == nullptr) == (bn == nullptr)) return -44;     // dy, or the BN backward's inputs
  DS2_HIP_CHECK((hipError_t)set_smem(conv1_wgrad_kernel, C1W_SMEM));
  Conv1Wgrad a{(const bf16_t*)dy, (const bf16_t*)x, part, N, T, F0, T1, F1,
               bn ? (const bf16_t*)bn->dz : nullptr, bn ? (const bf16_t*)bn->y1 : nullptr,
               bn ? bn->mean : nullptr, bn ? bn->invstd : nullptr, bn ? bn->gamma : nullptr,
               bn ? bn->beta : nullptr, bn ? bn->dbeta : nullptr, bn ? bn->dgamma : nullptr,
               (float)((double)N * T1 * F1)};
  hipLaunchKernelGGL(conv1_wgrad_kernel, dim3(grid), dim3(256), C1W_SMEM, st, a);
  hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(5 * 1024 / 256), dim3(256), 0, st, part, grid, 5 * 1024, dw);
  return (int)hipGetLastError();
}

int ds2_bn_cl_finalize(const float* part, int nb, double M, float eps, float* mean, float* invstd, float* run_mean,
                       float* run_var, float momentum, hipStream_t st) {
  hipLaunchKernelGGL(bn_cl_finalize_kernel, dim3(CC), dim3(256), 0, st, part, nb, M, eps, mean, invstd, run_mean,
                     run_var, momentum);
  return (int)hipGetLastError();
}

int ds2_bn_cl_apply(const void* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                    void* out, int N, int T, int F, int tmaj, hipStream_t st) {
  if (F > 96) return -44;
  if (tmaj) {
    const int rows = N * T;
    hipLaunchKernelGGL(bn_cl_apply_tmaj_kernel, dim3(rows < 4096 ? rows : 4096), dim3(256), 0, st, (const bf16_t*)y,
                       mean, invstd, gamma, beta, (bf16_t*)out, N, T, F);
  } else {
    const long long nch = (long long)N * T * F * 4;
    long long nb = (nch + 255) / 256;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(bn_cl_apply_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const bf16_t*)y, mean, invstd,
                       gamma, beta, (bf16_t*)out, nch);
  }
  return (int)hipGetLastError();
}

int ds2_bn_cl_bwd(const void* dz, const void* y, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, float* part, int nb, float* dgamma, float* dbeta, void* dy, int N, int T, int F,
                  int tmaj, int part_ready, hipStream_t st) {
  if (F > 96) return -45;
  if (part_ready && tmaj) return -46;                    // the time-major path transposes in the reduce
  // time-major dz: the reduce pass (which transposes it through LDS anyway) leaves a
  // channels-last copy in dy, and the apply pass then works in place on dy, coalesced
  // (the apply's own per-row LDS transpose ran at ~1/9 of the bandwidth roofline)
  // part_ready: part holds nb partial sums already (conv2_dgrad_kernel's bn epilogue); 2: and
  // no apply pass either (conv1_wgrad_kernel applies the BN backward while staging)
  if (!part_ready)
    hipLaunchKernelGGL(bn_cl_bwd_reduce_kernel, dim3(nb), dim3(256), 0, st, (const bf16_t*)dz, (const bf16_t*)y,
                       mean, invstd, gamma, beta, part, N, T, F, tmaj, tmaj ? (bf16_t*)dy : (bf16_t*)nullptr);
  hipLaunchKernelGGL(bn_cl_bwd_finalize_kernel, dim3(CC), dim3(256), 0, st, part, nb, dbeta, dgamma);
  const int rows = N * T;
  if (part_ready == 2) return (int)hipGetLastError();
  hipLaunchKernelGGL(bn_cl_bwd_apply_kernel, dim3(rows < 4096 ? rows : 4096), dim3(256), 0, st,
                     tmaj ? (const bf16_t*)dy : (const bf16_t*)dz, (const bf16_t*)y, mean, invstd, gamma, beta,
                     dbeta, dgamma, (bf16_t*)dy, N, T, F);
  return (int)hipGetLastError();
}

}  // extern "C"
