// Lookahead (row) convolution above the top recurrent layer of a unidirectional model
// (Deep Speech 2, section 3.7): a per-feature convolution over the next tau recurrent outputs.
//
//   h, r, dr, dh  bf16 [T, B, H] time-major, contiguous, H % 8 == 0, 16-B aligned
//   w             bf16 [H, tau + 1] (the parameter's shadow), 1 <= tau <= 31
//   valid(t, b) = t < min(lens[b], T)
//
//   forward   r[t,b,i]  = valid(t,b) ? sum_{j=0..tau, valid(t+j,b)} w[i,j] h[t+j,b,i] : 0
//   backward  dh[t,b,i] = valid(t,b) ? sum_{j=0..min(tau,t)} w[i,j] dr[t-j,b,i]       : 0
//             dw[i,j]   = sum_b sum_{t : valid(t+j,b)} dr[t,b,i] h[t+j,b,i]
//   stream    s = [hist (tau frames); x (n frames)], out[k] = sum_j w[:,j] s[k+j], hist <- last
//             tau frames of s
//
// window_kernel: forward, data gradient and the streaming step are one sliding window. A lane
// owns the 8 consecutive units of one batch row that a 16-B load brings (column (b, c)) and
// walks a tile of TT outputs: the TT fp32 accumulators stay in registers, the tile's TT + tau
// input frames are each loaded once and every frame is applied to the accumulators it reaches
// (input i of the tile meets output k at tap j = i - k). The forward walks time upwards and the
// data gradient downwards, so for one output the taps arrive in ascending j in both, each an
// fp32 FMA: every kernel here rounds identically and the streaming kernel agrees bitwise with
// the whole-sequence one (a tap the mask drops and a tap that multiplies a zero frame leave the
// same accumulator). The input frames are loaded eight at a time, the next eight in flight while
// these are applied. Measured at 241 x 32 x 800 (profiles/lookahead.md): about 10 us plus
// 0.6 us per tap, against 3.9 us for a copy of the tensor; the tap loop (8 unpacks, 4 packed
// FMAs and one LDS load per frame and output) is what the time is made of. The weights are transposed once per workgroup into LDS ([tau+1][H] bf16
// between TT-1 rows of zeros, a lane reads its 8 units of tap j with one 16-B LDS load); a tile's halo (tau frames) is re-read
// by the next tile's workgroup from L2. Invalid outputs are written as zeros, invalid inputs
// are never used (dr there is not trusted).
//
// wgrad_kernel: thread (bl, cl) of a workgroup owns batch row bg*32 + bl and column cb*8 + cl;
// it holds 8 dr frames and, per block of 8 taps, 8 x 8 accumulators in registers and walks the
// 15 h frames that block meets; the 32 batch rows are then summed in a fixed order through LDS
// into the workgroup's fp32 partial [H, tau+1] slice. The partials [P, H*(tau+1)] (P = time
// groups x groups of 32 batch rows: 31 at the headline shape, col_sum's time grows with P) are
// summed by col_sum (csrc/reduce.hip) in a fixed order: no atomics, bitwise reproducible.
#include "common.h"

using namespace ds2;

namespace {

constexpr int TT = 8;          // outputs per lane and tile (window_kernel), dr frames (wgrad_kernel)
constexpr int NTHR = 256;
constexpr int PF = 8;          // input frames loaded together (window_kernel)
constexpr int SB = 8;          // weight chunks in flight per thread while staging
constexpr int STREAM_TY = 4;   // lanes per column in the streaming step

struct Window {
  const bf16_t* x;             // h (forward), dr (backward), new frames [n, B, H] (stream)
  bf16_t* hist;                // stream: [tau, B, H], read, then rewritten, by the column's lanes
  bf16_t* out;
  const bf16_t* w;             // [H, tau + 1]
  const int* lens;             // [B] (forward / backward)
  int T, B, H, tau;            // T: output frames
};

// 8 bf16 units as 4 fp32 pairs: the pairs go through v_pk_fma_f32, two IEEE FMAs per lane and
// instruction (each half rounds as __fmaf_rn does)
typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ void unpack8(i32x4 v, f32x2* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    f[i] = f32x2{__uint_as_float((unsigned)v[i] << 16), __uint_as_float((unsigned)v[i] & 0xffff0000u)};
}

__device__ __forceinline__ i32x4 pack8(const f32x2* f) {
  i32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (int)((unsigned)f2bf(f[i].x) | ((unsigned)f2bf(f[i].y) << 16));
  return v;
}

__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// w [H, tau+1] -> LDS rows TT-1 .. TT-1+tau of [tau + 2 TT - 1][H], 16-B global loads (H % 8 == 0 makes H*(tau+1) a multiple of 8),
// eight in flight per thread. (i, j) of a thread's element advance by steps: one integer division
// per thread, not eight per chunk.
__device__ __forceinline__ void stage_weights(const bf16_t* __restrict__ w, bf16_t* wl, int H, int tau) {
  const int taps = tau + 1, n8 = H * taps / 8;
  // TT - 1 rows of zeros on either side: taps below 0 and above tau
  const int pad8 = (TT - 1) * H / 8;
  for (int q = threadIdx.x; q < 2 * pad8; q += NTHR)
    reinterpret_cast<i32x4*>(wl)[q < pad8 ? q : q - pad8 + (taps + TT - 1) * (H / 8)] = i32x4{0, 0, 0, 0};
  const int step_i = (NTHR * 8) / taps, step_j = (NTHR * 8) - step_i * taps;      // uniform
  int i = (threadIdx.x * 8) / taps, j = threadIdx.x * 8 - i * taps;
  for (int q0 = threadIdx.x; q0 < n8; q0 += SB * NTHR) {
    i32x4 v[SB];
#pragma unroll
    for (int r = 0; r < SB; ++r)
      v[r] = reinterpret_cast<const i32x4*>(w)[min(q0 + r * NTHR, n8 - 1)];      // unconditional: in flight together
#pragma unroll
    for (int r = 0; r < SB; ++r) {
      if (q0 + r * NTHR < n8) {
        int ii = i, jj = j;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          wl[(jj + TT - 1) * H + ii] = (bf16_t)(((unsigned)v[r][e >> 1] >> (16 * (e & 1))) & 0xffffu);
          if (++jj == taps) {
            jj = 0;
            ++ii;
          }
        }
      }
      i += step_i;
      j += step_j;
      if (j >= taps) {
        j -= taps;
        ++i;
      }
    }
  }
}

// MODE 0: forward, 1: data gradient, 2: streaming step. TY lanes share a column and take its
// time tiles in turn: 1 for the whole-sequence kernels, whose tiles are spread over blockIdx.y;
// 4 for the streaming step, whose few tiles must stay in one workgroup (it rewrites hist after a
// barrier, once every lane of the column has read what it needs).
template <int MODE>
__global__ __launch_bounds__(NTHR) void window_kernel(Window a) {
  constexpr int TY = MODE == 2 ? STREAM_TY : 1;
  constexpr int NCOL = NTHR / TY;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* wl = reinterpret_cast<bf16_t*>(smem);
  stage_weights(a.w, wl, a.H, a.tau);
  __syncthreads();
  const int C = a.H >> 3;
  const int ty = threadIdx.x / NCOL;
  const long long col = (long long)blockIdx.x * NCOL + threadIdx.x % NCOL;
  const bool live = col < (long long)a.B * C;
  const int b = live ? (int)(col / C) : 0, c = live ? (int)(col - (long long)b * C) : 0;
  const int T = a.T, tau = a.tau;
  const long long row = (long long)a.B * a.H;                 // elements per frame
  const long long off = (long long)b * a.H + 8 * c;
  // inputs of the window live in [0, Lin); outputs in [0, Lout)
  int Lout, Lin;
  if (MODE == 2) {
    Lout = T;
    Lin = T + tau;
  } else {
    Lout = Lin = max(0, min(a.lens[b], T));
  }
  // frame s of the window's input (null: outside it, or past this row's length)
  auto frame = [&](int s) -> const bf16_t* {
    if (s < 0 || s >= Lin) return nullptr;
    if (MODE == 2) return s < tau ? a.hist + (long long)s * row + off : a.x + (long long)(s - tau) * row + off;
    return a.x + (long long)s * row + off;
  };
  // Loads are unconditional, so that a group's loads are in flight together (a load under a
  // per-lane condition waits for its data before the next is issued): a frame outside the
  // window or past the row's length reads this column's frame 0 instead, always inside the
  // tensor, and the value is never used.
  const bf16_t* safe = a.x + off;
  const int ntiles = live ? (T + TT - 1) / TT : 0;
  for (int tile = blockIdx.y * TY + ty; tile < ntiles; tile += gridDim.y * TY) {
    const int t0 = tile * TT;
    f32x2 acc[TT][4];
#pragma unroll
    for (int k = 0; k < TT; ++k)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[k][u] = f32x2{0.f, 0.f};
    // input i of the tile: frame t0 + i (upwards) or t0 + TT - 1 - i (downwards); output k: frame
    // t0 + k or t0 + TT - 1 - k; they meet at tap j = i - k. The inputs come in groups of PF
    // loads, the next group in flight while this one is applied.
    const int nin = TT + tau, ngroups = (nin + PF - 1) / PF;
    const bf16_t* pc[PF];
    i32x4 vc[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      pc[q] = q < nin ? frame(MODE == 1 ? t0 + TT - 1 - q : t0 + q) : nullptr;
      vc[q] = *reinterpret_cast<const i32x4*>(pc[q] ? pc[q] : safe);
    }
    for (int g = 0; g < ngroups; ++g) {
      const bf16_t* pn[PF];
      i32x4 vn[PF];
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int i = (g + 1) * PF + q;
        pn[q] = i < nin ? frame(MODE == 1 ? t0 + TT - 1 - i : t0 + i) : nullptr;
        vn[q] = *reinterpret_cast<const i32x4*>(pn[q] ? pn[q] : safe);
      }
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int i = g * PF + q;
        if (pc[q]) {                                          // per lane: lens
          f32x2 xv[4];
          unpack8(vc[q], xv);
          // tap j = i - k sits in LDS row j + TT - 1; the rows of j < 0 and j > tau hold zeros,
          // so all TT outputs take the frame without a branch and the TT LDS loads go out
          // together (a zero tap leaves a finite accumulator as it is)
          const bf16_t* wrow = wl + (long long)(i + TT - 1) * a.H + 8 * c;
#pragma unroll
          for (int k = 0; k < TT; ++k) {
            f32x2 wv[4];
            unpack8(*reinterpret_cast<const i32x4*>(wrow - k * a.H), wv);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[k][u] = fma2(wv[u], xv[u], acc[k][u]);
          }
        }
        pc[q] = pn[q];
        vc[q] = vn[q];
      }
    }
#pragma unroll
    for (int k = 0; k < TT; ++k) {
      const int t = MODE == 1 ? t0 + TT - 1 - k : t0 + k;
      if (t >= T) continue;
      i32x4 v = {0, 0, 0, 0};
      if (t < Lout) v = pack8(acc[k]);
      *reinterpret_cast<i32x4*>(a.out + (long long)t * row + off) = v;
    }
  }
  if (MODE == 2) {
    // hist[m] <- s[T + m]. The column's lanes are all in this workgroup and no other touches the
    // column: lane ty loads frames m = ty, ty + TY, ... (at most 32 / TY) into registers, the
    // barriers put every read of hist (the tiles above and these) before every write
    constexpr int NM = (32 + STREAM_TY - 1) / STREAM_TY;
    i32x4 v[NM];
#pragma unroll
    for (int r = 0; r < NM; ++r) {
      const int m = ty + r * TY;
      v[r] = *reinterpret_cast<const i32x4*>(live && m < tau ? frame(T + m) : safe);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NM; ++r) {
      const int m = ty + r * TY;
      if (live && m < tau) *reinterpret_cast<i32x4*>(a.hist + (long long)m * row + off) = v[r];
    }
  }
}

// ---- weight gradient ---------------------------------------------------------------------
constexpr int WG_CL = 8;       // columns (of 8 units) per workgroup: 128 contiguous bytes of a row
constexpr int WG_BL = 32;      // batch rows per workgroup
constexpr int JT = 8;          // taps per register block
constexpr int RED_STRIDE = NTHR + 1;

struct Wgrad {
  const bf16_t* dr;
  const bf16_t* h;
  const int* lens;
  float* part;                 // [P][H * (tau + 1)], P = time groups x batch groups
  int T, B, H, tau, tpw;       // tpw: time tiles (of TT frames) per workgroup
};

__global__ __launch_bounds__(NTHR) void wgrad_kernel(Wgrad a) {
  __shared__ float red[4 * 8 * RED_STRIDE];                   // [4 taps x 8 units][256 (+1) lanes]
  const int cl = threadIdx.x % WG_CL, bl = threadIdx.x / WG_CL;
  const int C = a.H >> 3;
  const int c = blockIdx.x * WG_CL + cl;
  const int nbg = (a.B + WG_BL - 1) / WG_BL;
  const int tg = blockIdx.y / nbg, bg = blockIdx.y - tg * nbg;
  const int b = bg * WG_BL + bl;
  const bool live = c < C && b < a.B;
  const int tau = a.tau;
  const long long row = (long long)a.B * a.H;
  const long long off = (long long)(live ? b : 0) * a.H + 8 * (live ? c : 0);
  int L = 0;
  if (live) L = max(0, min(a.lens[b], a.T));
  float* part = a.part + (long long)blockIdx.y * a.H * (tau + 1);
  const int ntiles = (a.T + TT - 1) / TT;
  for (int jb = 0; jb <= tau; jb += JT) {
    f32x2 acc[JT][4];
#pragma unroll
    for (int m = 0; m < JT; ++m)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[m][u] = f32x2{0.f, 0.f};
    for (int q = 0; q < a.tpw; ++q) {
      const int tile = tg * a.tpw + q;
      if (tile >= ntiles) break;
      const int t0 = tile * TT;
      if (t0 + jb >= L) continue;                             // nothing valid left for this lane
      f32x2 d[TT][4];
#pragma unroll
      for (int k = 0; k < TT; ++k) {
        // (unconditional loads, in flight together; frames at or past L read frame T - 1 of the
        // column, inside the tensor, and count as zero)
        const i32x4 v = *reinterpret_cast<const i32x4*>(a.dr + (long long)min(t0 + k, a.T - 1) * row + off);
        unpack8(t0 + k < L ? v : i32x4{0, 0, 0, 0}, d[k]);
      }
      // h frame t0 + jb + i meets dr frame t0 + k at tap jb + (i - k)
      // (a frame at or past L is not loaded and adds nothing: valid(t + j, b) fails there)
      i32x4 hv[TT + JT - 1];
#pragma unroll
      for (int i = 0; i < TT + JT - 1; ++i) {
        hv[i] = *reinterpret_cast<const i32x4*>(a.h + (long long)min(t0 + jb + i, a.T - 1) * row + off);
      }
#pragma unroll
      for (int i = 0; i < TT + JT - 1; ++i) {
        if (t0 + jb + i >= L) continue;
        f32x2 xv[4];
        unpack8(hv[i], xv);
#pragma unroll
        for (int k = 0; k < TT; ++k) {
          const int m = i - k;
          if (m < 0 || m >= JT) continue;
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[m][u] = fma2(d[k][u], xv[u], acc[m][u]);
        }
      }
    }
    // the batch rows of the workgroup, summed in the order bl = 0..31, four taps at a time
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __syncthreads();
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int u = 0; u < 8; ++u)
          red[(m * 8 + u) * RED_STRIDE + threadIdx.x] = (u & 1) ? acc[half * 4 + m][u >> 1].y : acc[half * 4 + m][u >> 1].x;
      __syncthreads();
      for (int e = threadIdx.x; e < 4 * 8 * WG_CL; e += NTHR) {
        const int m = e & 3, u = (e >> 2) & 7, ccl = e >> 5;
        const int j = jb + half * 4 + m, cc = blockIdx.x * WG_CL + ccl;
        if (j > tau || cc >= C) continue;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < WG_BL; ++r) s += red[(m * 8 + u) * RED_STRIDE + r * WG_CL + ccl];
        part[(long long)(cc * 8 + u) * (tau + 1) + j] = s;
      }
    }
  }
}

bool bad_shape(int T, int B, int H, int tau) {
  return T < 1 || B < 1 || H < 8 || H % 8 != 0 || tau < 1 || tau > 31 ||
         (long long)T * B * H >= (1ll << 40);
}
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

template <int MODE>
int launch_window(const Window& a, hipStream_t st) {
  const size_t lds = (size_t)(a.tau + 2 * TT - 1) * a.H * sizeof(bf16_t);
  if (lds > 160 * 1024) return -62;
  auto kern = window_kernel<MODE>;
  static size_t granted = 64 * 1024;
  if (lds > granted) {
    DS2_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    granted = 160 * 1024;
  }
  const long long ncol = (long long)a.B * (a.H / 8);
  const int per_wg = MODE == 2 ? NTHR / STREAM_TY : NTHR;
  const unsigned gx = (unsigned)((ncol + per_wg - 1) / per_wg);
  const int ntiles = (a.T + TT - 1) / TT;
  // the streaming step keeps a column's tiles in one workgroup (it rewrites hist afterwards);
  // the others spread the time tiles over up to ~2048 workgroups and loop beyond that
  unsigned gy = 1;
  if (MODE != 2) gy = (unsigned)max(1, min(ntiles, (int)(2048 / gx)));
  ds2_launch(kern, dim3(gx, gy), dim3(NTHR), (unsigned)lds, st, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int ds2_lookahead(const void* x, const void* w, const int* lens, void* out, int T, int B, int H,
                             int tau, int bwd, hipStream_t st) {
  if (bad_shape(T, B, H, tau)) return -60;
  if (misaligned(x) || misaligned(w) || misaligned(out)) return -61;
  Window a{static_cast<const bf16_t*>(x), nullptr, static_cast<bf16_t*>(out), static_cast<const bf16_t*>(w), lens,
           T, B, H, tau};
  return bwd ? launch_window<1>(a, st) : launch_window<0>(a, st);
}

extern "C" int ds2_lookahead_stream(void* hist, const void* x, const void* w, void* out, int n, int B, int H,
                                    int tau, hipStream_t st) {
  if (bad_shape(n, B, H, tau)) return -60;
  if (misaligned(hist) || misaligned(x) || misaligned(w) || misaligned(out)) return -61;
  Window a{static_cast<const bf16_t*>(x), static_cast<bf16_t*>(hist), static_cast<bf16_t*>(out),
           static_cast<const bf16_t*>(w), nullptr, n, B, H, tau};
  return launch_window<2>(a, st);
}

// time tiles per workgroup: one, or as many as keep about 512 workgroups (the partials, which
// col_sum reads again, shrink with it)
extern "C" int ds2_lookahead_wgrad_tpw(int T, int B, int H) {
  if (T < 1 || B < 1 || H < 8) return -60;
  const long long ntiles = (T + TT - 1) / TT, nbg = (B + WG_BL - 1) / WG_BL;
  const long long ncb = (H / 8 + WG_CL - 1) / WG_CL;
  long long tpw = ntiles * nbg * ncb / 512;
  if (tpw < 1) tpw = 1;
  if (tpw > 64) tpw = 64;
  return (int)tpw;
}

extern "C" int ds2_lookahead_wgrad_parts(int T, int B, int H) {
  const int tpw = ds2_lookahead_wgrad_tpw(T, B, H);
  if (tpw < 1) return tpw;
  const int ntiles = (T + TT - 1) / TT;
  return ((ntiles + tpw - 1) / tpw) * ((B + WG_BL - 1) / WG_BL);
}

extern "C" int ds2_lookahead_wgrad(const void* dr, const void* h, const int* lens, float* part, int T, int B, int H,
                                   int tau, hipStream_t st) {
  if (bad_shape(T, B, H, tau)) return -60;
  if (misaligned(dr) || misaligned(h)) return -61;
  const int tpw = ds2_lookahead_wgrad_tpw(T, B, H);
  const int P = ds2_lookahead_wgrad_parts(T, B, H);
  Wgrad a{static_cast<const bf16_t*>(dr), static_cast<const bf16_t*>(h), lens, part, T, B, H, tau, tpw};
  const unsigned gx = (unsigned)((H / 8 + WG_CL - 1) / WG_CL);
  ds2_launch(wgrad_kernel, dim3(gx, (unsigned)P), dim3(NTHR), 0, st, a);
  return (int)hipGetLastError();
}
