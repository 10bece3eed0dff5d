// conv2 of the DeepSpeech2 front-end for gfx950: forward, data gradient and weight gradient
// (layouts and the MFMA fragment mapping: conv_common.h).
//
//   conv2 fwd   rows = 32 output positions f2, cols = 32 co, k = (kt, kf, ci) in 100 k-steps of 16.
//               Persistent: each wave keeps ITS quarter of the weight fragments (25 k-steps) in
//               VGPRs for the whole launch; the 10 input rows of an output row (one contiguous
//               50.5 KB block) are double-buffered in LDS by global_load_lds (channel-chunk
//               planes -> conflict-free ds_read_b128); the 4 K-quarters are summed
//               through LDS in the epilogue, which also adds the bias, stores bf16 and
//               accumulates the BN batch statistics of the stored values.
//   conv2 dgrad rows = 32 input positions f1, cols = 32 ci, k = (kt, kf, co); a tile is the
//               output row pair (2u, 2u+1), whose kt parities read the same 5 rows of dy.
//   conv2 wgrad rows = co, cols = ci, k = positions; both operands are read with
//               ds_read_b64_tr_b16 (hardware transpose) from channels-last LDS images;
//               per-workgroup fp32 partials are summed by a reduce kernel into the arena.
//
// The forward and the data gradient share their skeleton (xcd_tiles, c2_stamp, gather_wfrag,
// acc4, copy_row, channel_sums); their MFMA loops, LDS exchanges and `issue` lambdas differ in
// substance and are written out in each body.
#include "bn_math.h"
#include "conv_common.h"

using namespace ds2;

namespace {

constexpr int PR = 80;                           // LDS bytes per position row (64 data + 16 pad; dgrad)

// A wave's KPW weight fragments out of the LDS image wl of operand half hh: k-step s = S0 + i is
// (kt or ai = s / 10, kf = (s % 10) >> 1, half s & 1), and idx(k-row, col, s / 10, kf) is the
// image's element for B[k-row][col].
template <int KPW, int S0, typename Idx>
__device__ __forceinline__ void gather_wfrag(bf16x8 (&bfr)[KPW], const unsigned short* wl, int hh, int hi, int col,
                                             Idx idx) {
#pragma unroll
  for (int i = 0; i < KPW; ++i) {
    const int s = S0 + i;
    if ((s & 1) != hh) continue;
    const int kt = s / 10, kf = (s % 10) >> 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) bfr[i][j] = (short)wl[idx(8 * hi + j, col, kt, kf)];
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
  long long* trace;   // optional c2_stamp stamps (diagnostics)
};
constexpr int C2F_KPW = 25;                      // k-steps per wave
constexpr int C2F_PL = 80;                       // positions per plane (F1 <= 80)
constexpr int C2F_BUF = (C2_KT * 4 * C2F_PL + 20) * 16;   // 40 planes + the last plane's overrun
// after the MFMA loop the row buffer is scratch: 36 partial-sum slots (wave -> owner, m) of
// 64 f32x4, then the bf16 output row
constexpr int C2F_STG = 36 * 64 * 16;
constexpr int C2F_SMEM = C2F_BUF;
static_assert(C2F_STG + 32 * MT * 64 <= C2F_BUF, "partial sums and the output row fit in the row buffer");
static_assert(C2F_SMEM >= 32 * 16 * C2_KT * C2_KF * 2, "one ci half of the weights is staged through LDS");

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
    const unsigned* wsrc = (const unsigned*)a.w;                     // [32 co][32 ci][25 dwords]
    for (int hh = 0; hh < 2; ++hh) {
      for (int d = tid; d < 32 * 16 * 25; d += 256) {
        const int co = d / 400, rem = d - co * 400, ci = rem / 25, e = rem - ci * 25;
        ((unsigned*)smem)[(ci * 32 + co) * 25 + e] = wsrc[(co * 32 + 16 * hh + ci) * 25 + e];
      }
      __syncthreads();
      gather_wfrag<C2F_KPW, S0>(bfr, (const unsigned short*)smem, hh, hi, col,
                                [](int ci, int co, int kt, int kf) { return (ci * 32 + co) * 50 + kt * C2_KF + kf; });
      __syncthreads();
    }
  }
  const float bco = a.bias ? a.bias[col] : 0.f;
  const int F1 = a.F1;
  const TileRange tr = xcd_tiles(a.N * a.T2);

  // stage input rows 2 t2 .. 2 t2 + 9: plane p = (row p >> 2, 16-B channel chunk p & 3), round r
  // = positions 64 r + lane (F1 in (64, 80]: 2 rounds; narrower rows leave round 1 empty and the
  // positions past F1 unstaged). Wave w issues rounds k = w + 4 i of the
  // 80, i.e. planes (w >> 1) + 2 i in round w & 1: every offset but the tile base is a constant.
  // (The data gradient stages clamped, padded rows in 80-B position rows instead: not shared.)
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
  if (tr.first < tr.hi) issue(tr.first);
  for (int tile = tr.first; tile < tr.hi; tile += tr.per, ++it) {
    const int n = tile / a.T2, t2 = tile - n * a.T2;
    c2_stamp(a.trace, it, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // this tile's rows are in buf
    c2_stamp(a.trace, it, 1);
    // MFMA loop: every k-step multiplies (the data gradient skips k-steps outside [0, T2))
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
    // reduce-scatter among 4 waves (the data gradient's is pairwise): wave w owns accumulator
    // group r4 = w of every m (output rows 32 m + 8 w + 4 hi + 0..3); slot (src, owner rank, m)
    // with the owner's rank among src's 3 partners
    c2_stamp(a.trace, it, 2);
    lds_barrier();                                     // every MFMA read of buf done
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (o == w) continue;
      const int rk = o - (o > w ? 1 : 0);
#pragma unroll
      for (int m = 0; m < MT; ++m) red[((w * 3 + rk) * MT + m) * 64 + lane] = acc4(acc[m], o);
    }
    lds_barrier();
    f32x4 own[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) own[m] = acc4(acc[m], w);
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
    copy_row(a.y + ((size_t)n * a.T2 + t2) * a.F2 * CC, stg, a.F2 * 4, tid, 256);
    c2_stamp(a.trace, it, 4);
    lds_barrier();                                     // the row copy's reads done: buf is free
    if (tile + tr.per < tr.hi) issue(tile + tr.per);
    c2_stamp(a.trace, it, 5);
  }
  __syncthreads();
  channel_sums(ssum, ssq, (float*)red, w, a.part);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv2_fwd_kernel(Conv2Fwd a) {
  DS2_DCHECK(a.T2 == (a.T1 - C2_KT) / 2 + 1 && a.F2 == a.F1 - 4 && a.F1 <= C2F_PL && a.F1 >= 5);
  switch (uni(threadIdx.x >> 6)) {                   // k-step s = kt * 10 + kf * 2 + ci-half
    case 0: conv2_fwd_body<0>(a); break;
    case 1: conv2_fwd_body<C2F_KPW>(a); break;
    case 2: conv2_fwd_body<2 * C2F_KPW>(a); break;
    default: conv2_fwd_body<3 * C2F_KPW>(a); break;
  }
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
  DS2Conv2DgradBn bn;   // all null without the BatchNorm-backward sums (see bn_cl_bwd_reduce_kernel)
  long long* trace;   // optional phase stamps, as Conv2Fwd::trace
};
constexpr int C2D_KPW = 25;                      // k-steps per wave (one parity's 50 in halves)
constexpr int C2D_PR = 4 + 32 * MT;              // LDS position rows per dy row (positions -4 .. 95)
constexpr int C2D_BUF = 5 * C2D_PR * PR;         // 40000 B
constexpr int C2D_RED = 4 * 6 * 64 * 16;        // [wave][6 groups it hands over][64] f32x4
constexpr int C2D_ROW = 80 * 64;                 // one bf16 output row [F1 <= 80][32]
constexpr int C2D_SMEM = C2D_BUF + C2D_RED + 2 * C2D_ROW;
static_assert(C2D_SMEM >= 16 * CC * C2_KT * C2_KF * 2, "one co half of the weights is staged through LDS");

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
  for (int hh = 0; hh < 2; ++hh) {
    const i32x4* src = (const i32x4*)(a.w + (size_t)hh * 16 * CC * C2_KT * C2_KF);
    for (int o = tid; o < 16 * CC * C2_KT * C2_KF / 8; o += 256) ((i32x4*)smem)[o] = src[o];
    __syncthreads();
    gather_wfrag<C2D_KPW, S0>(bfr, (const unsigned short*)smem, hh, hi, col, [](int co, int ci, int ai, int kf) {
      return ((co * CC + ci) * C2_KT + 2 * ai + par) * C2_KF + kf;
    });
    __syncthreads();
  }
  for (int o = tid * 16; o < C2D_BUF; o += 256 * 16) *(i32x4*)(buf + o) = (i32x4){0, 0, 0, 0};

  const int U = (a.T1 + 1) >> 1;
  const int F2 = a.F2, nq = 5 * F2;                        // 16-B chunks per dy row (<= 6 rounds)
  const TileRange tr = xcd_tiles(a.N * U);

  // stage dy rows u-4..u of tile t into the 5 slots (rows outside [0, T2) are clamped: their
  // k-steps are skipped); a lane's 16-B chunk q of a slot is position q / 5, chunk q % 5, and
  // chunk 4 (the row's pad column, never read) repeats chunk 3. Wave w issues rounds k = w + 4 i
  // of the 30 (slot k / 6, round k % 6): compile-time slot and LDS offset.
  // (The forward stages unpadded channel-chunk planes instead: not shared.)
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
  const bool bn = a.bn.mean != nullptr;
  const float bmu = bn ? a.bn.mean[col] : 0.f, bis = bn ? a.bn.invstd[col] : 0.f;
  const float bg = bn ? a.bn.gamma[col] : 0.f, bbt = bn ? a.bn.beta[col] : 0.f;
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
  if (tr.first < tr.hi) issue(tr.first);
  for (int tile = tr.first; tile < tr.hi; tile += tr.per, ++it) {
    const int n = tile / U, u = tile - n * U;
    c2_stamp(a.trace, it, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // this tile's rows are in buf
    c2_stamp(a.trace, it, 1);
    // MFMA loop: k-steps whose dy row lies outside [0, T2) are skipped (the forward has none)
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
    // the parity's two K halves reduce-scatter (pairwise; the forward's is among 4 waves): K half
    // kh owns accumulator groups r4 = 2 kh + j (j = 0, 1) of every m, i.e. output rows
    // 32 m + 8 (2 kh + j) + 4 hi + 0..3, and hands the other two groups to its partner (wave
    // W ^ 2) through red[wave][m][j]
    lds_barrier();                                     // the previous tile's red / row reads done
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j) red[((w * MT + m) * 2 + j) * 64 + lane] = acc4(acc[m], 2 * (1 - kh) + j);
    lds_barrier();
    f32x4 own[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        own[m][j] = acc4(acc[m], 2 * kh + j) + red[(((w ^ 2) * MT + m) * 2 + j) * 64 + lane];
    c2_stamp(a.trace, it, 3);
    const int t1 = 2 * u + par;
    const bool out = t1 < a.T1;                        // wave-uniform
    const size_t rowoff = ((size_t)n * a.T1 + t1) * a.F1 * CC;
    if (out) {
      // conv1's outputs at the owned positions, loaded before any global store of the tile
      // (one per-lane base, compile-time offsets; the last m-tile clamped to the row)
      unsigned short yv[MT][2][4];
      if (bn) {
        const unsigned short* yb = (const unsigned short*)a.bn.y1 + rowoff + 4 * hi * CC + col;
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
                const float xh = bn_xhat(bf2f(yv[m][j][e]), bmu, bis);
                const float dd = bn_masked(xh, bg, bbt, bf2f(d));
                bs += dd;
                bq += dd * xh;
              }
            }
          }
    }
    lds_barrier();                                     // both halves of each parity row staged
    if (out) copy_row(a.dx + rowoff, stg, a.F1 * 4, kh * 64 + lane, 128);
    c2_stamp(a.trace, it, 4);
    // the next tile's rows go out after every LDS access (and conv1 load) of this one: hipcc
    // puts an s_waitcnt vmcnt(0) before any LDS access while LDS-DMA loads are in flight
    if (tile + tr.per < tr.hi) issue(tile + tr.per);
    c2_stamp(a.trace, it, 5);
  }
  if (bn) channel_sums(bs, bq, (float*)red, w, a.bn.part);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv2_dgrad_kernel(Conv2Dgrad a) {
  DS2_DCHECK(a.F2 <= 32 * MT - 4 && a.F1 == a.F2 + 4 && a.F1 > 64 && a.F1 <= 80);
  switch (uni(threadIdx.x >> 6)) {
    case 0: conv2_dgrad_body<0>(a); break;
    case 1: conv2_dgrad_body<1>(a); break;
    case 2: conv2_dgrad_body<2>(a); break;
    default: conv2_dgrad_body<3>(a); break;
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
  const unsigned lofs = tr_lane_ofs(lane);
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
      const bf16x8 av = tr_frag(cur + k0 + lofs);
#pragma unroll
      for (int i = 0; i < C2W_PPW; ++i) {
        if (i < npairs) {
          const int P = w + C2W_WAVES * i;
          const int kt = P / 5, kf = P - 5 * (P / 5);
          acc[i] = mfma32(av, tr_frag(xs + (unsigned)(kt * a.F1 + kf) * 64u + k0 + lofs), acc[i]);
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
      for (int r4 = 0; r4 < 4; ++r4) out[(P * 4 + r4) * 64 + lane] = acc4(acc[i], r4);
    }
  }
}

int shape_ok(int T1, int F1, int T2, int F2) {
  if (F1 < 5 || F1 > 80 || F2 != F1 - 4) return CONV2_F_RANGE;
  if (T1 < 10 || T2 != (T1 - 10) / 2 + 1) return CONV2_T_RANGE;
  return 0;
}

}  // namespace

extern "C" {

const char* ds2_conv_status_str(int rc) {
  switch (rc) {
#define X(name, value, meaning) \
  case value: return meaning;
    DS2_CONV_STATUS(X)
#undef X
  }
  return nullptr;
}

size_t ds2_conv2_fwd_smem(int) { return (size_t)C2F_SMEM; }
size_t ds2_conv2_dgrad_smem(int) { return (size_t)C2D_SMEM; }
size_t ds2_conv2_wgrad_smem(int F1) { return (size_t)2 * (80 * 64 + (9 * F1 + 84) * 64); }
long long ds2_conv2_wgrad_part_floats(int grid) { return (long long)grid * C2W_PAIRS * 1024; }

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
  if (F1 <= 64) return CONV2_DGRAD_NARROW;
  const size_t smem = ds2_conv2_dgrad_smem(F2);
  DS2_HIP_CHECK((hipError_t)set_smem(conv2_dgrad_kernel, smem));
  Conv2Dgrad a{(const bf16_t*)dy, (const bf16_t*)w, (bf16_t*)dx, N, T1, F1, T2, F2,
               bn ? *bn : DS2Conv2DgradBn{}, trace};
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

}  // extern "C"
