// Audio featurizer for gfx950: PCM [B, S] (fp32 or int16) -> [B, T_max, 161] features, the
// device counterpart of data/featurizer.py (which stays the fp64 oracle).
//
// A call is two launches: audio_stats_kernel (per-row mean and 1 / peak, only for
// normalize="utterance") and featurize_kernel, one workgroup per (row, 32-frame tile):
//
//   1. the tile's 31 * 160 + L samples are normalised, pre-emphasised (mfcc) and staged once in
//      LDS. Frames overlap (hop 160 of L = 400 / 320 samples), so the DFT's A operand is read
//      straight from that buffer at a row stride of one hop; a word of padding per hop makes the
//      stride 161, odd, so the 32 lanes of an MFMA A read hit 32 different banks (at 160 they
//      would all hit one).
//   2. the real DFT is an fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32: exact f32, a k-ordered fma
//      chain) against a packed basis [L, 2 * NH]: columns [0, NH) are cos of bins 0 .. NH-1,
//      column NH is cos of the Nyquist bin NH (its sin, like bin 0's, is identically 0) and
//      columns NH + c are sin of bin c. A wave owns the cos and the sin tile of the same 32 bins,
//      so re^2 + im^2 is lane-local. The spectrogram's Hamming window is folded into its basis
//      rows on the host. With a 32-frame tile every basis element is consumed by exactly one
//      wave of the workgroup, so the basis is read from L2 straight into the B operand
//      register: staging it in LDS first would add a hop and no reuse.
//   3. power spectrum -> LDS. spectrogram: log(p + 1e-14) and out. mfcc: frame energy (row sum),
//      banded mel filterbank from a compact table (<= 8 taps per filter; empty filters give an
//      exact 0), eps substitution, log -> LDS; then the DCT-II to 161 cepstra as a second fp32
//      MFMA GEMM from LDS against a [322, 192] table, lifter, c0 = log energy.
//
// Rows at or past an utterance's frame count are written as exact zeros. No atomics and a
// fixed reduction order everywhere: a frame's result does not depend on its tile position, the
// batch or the chunking of a stream. No host synchronisation, so a call can be graph-captured.
#include "common.h"

namespace {

using namespace ds2;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int HOP = 160, TILE = 32, NTHR = 256, NCEP = 161;
constexpr int NFILT = 322, MELW = 8, DCT_LD = 192, LOG_LD = NFILT + 1, DCT_TILES = 6;
constexpr float FEPS = 2.220446049250313e-16f;   // np.finfo(float).eps, as the oracle substitutes

template <int KIND> struct Geo;
template <> struct Geo<0> {   // mfcc: 400-sample rectangular frames, 512-point DFT, 257 bins
  static constexpr int L = 400, NH = 256, NPAIR = 8;
  static constexpr float SCALE = 1.0f / 512.0f;
};
template <> struct Geo<1> {   // spectrogram: 320-sample Hamming frames, 320-point DFT, 161 bins
  static constexpr int L = 320, NH = 160, NPAIR = 5;
  static constexpr float SCALE = 1.0f;
};

template <int KIND> struct Lds {
  static constexpr int NS = (TILE - 1) * HOP + Geo<KIND>::L;
  static constexpr int STAGE = (NS + NS / HOP + 1 + 3) & ~3;
  static constexpr int PW_LD = Geo<KIND>::NH + 1;
  // mfcc: the log mel energies reuse the staging buffer (dead once the DFT has read it)
  static constexpr int FRONT = (KIND == 0 && TILE * LOG_LD > STAGE) ? TILE * LOG_LD : STAGE;
  static constexpr int FLOATS = FRONT + TILE * PW_LD + (KIND == 0 ? TILE : 0);
};

// mode 0: a whole signal (the last frame zero-padded); 1: a stream in flight (complete frames
// only); 2: the end of a stream that has emitted frames already (a padded frame only if it
// holds samples no earlier frame covered)
template <int L>
__device__ __forceinline__ int frame_count(int n, int mode) {
  if (mode == 1) return n < L ? 0 : 1 + (n - L) / HOP;
  if (mode == 2 && n <= L - HOP) return 0;
  return n <= L ? 1 : 1 + (n - L + HOP - 1) / HOP;
}

__device__ __forceinline__ void store_out(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_out(bf16_t* p, float v) { *p = f2bf(v); }

// ---- per-row mean and 1 / max|x - mean| in one pass: sum in fp64, min and max exact, fixed order
template <typename IN>
__global__ __launch_bounds__(1024) void audio_stats_kernel(const IN* __restrict__ pcm, long long row_stride, int S,
                                                           const int* __restrict__ lens,
                                                           float* __restrict__ offset, float* __restrict__ gain) {
  __shared__ double ssum[16];
  __shared__ float smin[16], smax[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = S;
  if (lens) n = min(max(lens[b], 0), S);
  const IN* x = pcm + (size_t)b * row_stride;
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < n; i += 1024) {
    const float v = (float)x[i];
    s += (double)v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    ssum[wave] = s;
    smin[wave] = mn;
    smax[wave] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) {
      t += ssum[w];
      mn = fminf(mn, smin[w]);
      mx = fmaxf(mx, smax[w]);
    }
    const double mean = n > 0 ? t / (double)n : 0.0;
    const double peak = n > 0 ? fmax((double)mx - mean, mean - (double)mn) : 0.0;
    offset[b] = (float)mean;
    gain[b] = peak > 0.0 ? (float)(1.0 / peak) : 1.0f;
  }
}

// One wave's share of a [32, K] x [K, ld] fp32 product on v_mfma_f32_32x32x2_f32: NQ tiles of 32
// columns (128 columns apart: the waves interleave) times NC column blocks (cstride apart),
// accumulated into acc[q][c]. a: this lane's row of the LDS operand (+ its k half), b: the global
// operand at this lane's k half and column. The B values of the next KU k-steps are in flight
// while the current ones feed the MFMAs (two register sets, no LDS hop: each element has one
// consumer). PAD: the LDS row carries one pad word per HOP samples.
template <int K, int NQ, int NC, int KU, bool PAD>
__device__ __forceinline__ void mma_tiles(const float* __restrict__ a, const float* __restrict__ b, int ld,
                                          int cstride, f32x16 (&acc)[2][2]) {
  static_assert((K / 2) % KU == 0 && K % 2 == 0, "K must be a whole number of KU k-steps");
  constexpr int NIT = K / (2 * KU);
  float b0[KU][NQ][NC], b1[KU][NQ][NC];
  auto load = [&](float (&v)[KU][NQ][NC], int it) {
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) v[u][q][c] = b[(size_t)(2 * (it * KU + u)) * ld + q * 128 + c * cstride];
  };
  auto mma = [&](const float (&v)[KU][NQ][NC], int it) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k0 = 2 * (it * KU + u);
      const float av = a[PAD ? k0 + k0 / HOP : k0];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[q][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, v[u][q][c], acc[q][c], 0, 0, 0);
    }
  };
  load(b0, 0);
  int it = 0;
  for (; it + 2 <= NIT; it += 2) {
    load(b1, it + 1);
    mma(b0, it);
    if (it + 2 < NIT) load(b0, it + 2);
    mma(b1, it + 1);
  }
  if (it < NIT) mma(b0, it);
}

template <int KIND, typename IN, typename OUT>
__global__ __launch_bounds__(NTHR) void featurize_kernel(DS2Feat a) {
  using G = Geo<KIND>;
  using M = Lds<KIND>;
  constexpr int L = G::L, NH = G::NH, NCOL = 2 * NH, PW_LD = M::PW_LD;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* stage = lds;
  float* pw = stage + M::FRONT;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, f0 = blockIdx.x * TILE;
  int n = a.S - a.lead;
  if (a.lens) n = min(max(a.lens[b], 0), n);
  const int nf = min(frame_count<L>(n, a.mode), a.T_max);
  if (blockIdx.x == 0 && tid == 0) a.frames[b] = nf;
  OUT* out = reinterpret_cast<OUT*>(a.out) + ((size_t)b * a.T_max + f0) * NCEP;
  const int rows = min(TILE, a.T_max - f0);       // output rows this workgroup owns
  if (f0 >= nf) {                                 // all padding: exact zeros, nothing to compute
    for (int i = tid; i < rows * NCEP; i += NTHR) store_out(out + i, 0.f);
    return;
  }

  // ---- 1. stage (x - offset) * gain, pre-emphasised, zero past the signal's end
  {
    const IN* x = reinterpret_cast<const IN*>(a.pcm) + (size_t)b * a.row_stride + a.lead;
    const float off = a.offset[b], g = a.gain[b];
    const int n0 = f0 * HOP;
    // every load of the tile is issued before the first use (indices clamped into the signal,
    // the selection comes after): a load-use chain per sample would cost a memory latency each
    constexpr int NLD = (M::NS + NTHR - 1) / NTHR;
    float cur[NLD], prv[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      cur[i] = 0.f;
      prv[i] = 0.f;
      if (n > 0) {
        const int mc = min(n0 + tid + i * NTHR, n - 1);
        cur[i] = (float)x[mc];
        if (KIND == 0) prv[i] = (float)x[max(mc - 1, -a.lead)];
      }
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int s = tid + i * NTHR, m = n0 + s;
      if (s < M::NS) {
        float y = 0.f;
        if (m < n) {
          y = (cur[i] - off) * g;
          // y[0] = x[0] only for the signal's true first sample: a stream's later calls carry
          // the sample before their first one (lead = 1)
          if (KIND == 0 && (m > 0 || a.lead)) y = fmaf(-0.97f, (prv[i] - off) * g, y);
        }
        stage[s + s / HOP] = y;
      }
    }
  }
  __syncthreads();

  // ---- 2. DFT: [32 frames, L] x [L, 2 NH]; wave w owns bin tiles w and w + 4 (cos and sin)
  const int col = lane & 31, half = lane >> 5;
  {
    f32x16 acc[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][c][r] = 0.f;
    const float* arow = stage + col * (HOP + 1) + half;
    const float* bp = a.basis + half * NCOL + col + wave * 32;
    if (wave + 4 < G::NPAIR) mma_tiles<L, 2, 2, 4, true>(arow, bp, NCOL, NH, acc);
    else mma_tiles<L, 1, 2, 4, true>(arow, bp, NCOL, NH, acc);
    // power spectrum; column 0's "sin" slot holds the Nyquist bin's cos
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int p = wave + 4 * q;
      if (p < G::NPAIR) {
        const int bin = p * 32 + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
          const float re = acc[q][0][r], im = acc[q][1][r];
          if (bin == 0) {
            pw[row * PW_LD] = re * re * G::SCALE;
            pw[row * PW_LD + NH] = im * im * G::SCALE;
          } else {
            pw[row * PW_LD + bin] = (re * re + im * im) * G::SCALE;
          }
        }
      }
    }
  }
  __syncthreads();

  if constexpr (KIND == 1) {
    for (int i = tid; i < rows * NCEP; i += NTHR) {
      const int row = i / NCEP, c = i - row * NCEP;
      store_out(out + i, f0 + row < nf ? logf(pw[row * PW_LD + c] + 1e-14f) : 0.f);
    }
  } else {
    float* logs = stage;                          // every wave is past the DFT (barrier above)
    float* loge = pw + TILE * PW_LD;
    // ---- 3a. frame energy: wave w sums rows 8w .. 8w+7 over the 257 bins, fixed order
    for (int rr = 0; rr < TILE / 4; ++rr) {
      const int row = wave * (TILE / 4) + rr;
      float e = 0.f;
      for (int c = lane; c <= NH; c += 64) e += pw[row * PW_LD + c];
      e = wave_sum(e);
      if (lane == 0) loge[row] = logf(e == 0.f ? FEPS : e);
    }
    // ---- 3b. banded mel filterbank + log
    // a work item is one filter over 8 rows: its window and 8 weights (zero past its taps, and
    // first + 8 <= 257 by construction of the table) are loaded once, the rows come from LDS
    constexpr int RQ = 8, NITEM = NFILT * (TILE / RQ);
#pragma unroll
    for (int it = 0; it < (NITEM + NTHR - 1) / NTHR; ++it) {
      const int i = tid + it * NTHR;
      if (i < NITEM) {
        const int rq = i / NFILT, j = i - rq * NFILT;
        const int first = min(max(a.mel_idx[2 * j], 0), NH + 1 - MELW);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(a.mel_w + j * MELW);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(a.mel_w + j * MELW + 4);
#pragma unroll
        for (int r = 0; r < RQ; ++r) {
          const float* p = pw + (rq * RQ + r) * PW_LD + first;
          float s = 0.f;
#pragma unroll
          for (int t = 0; t < 4; ++t) s = fmaf(w0[t], p[t], s);
#pragma unroll
          for (int t = 0; t < 4; ++t) s = fmaf(w1[t], p[4 + t], s);
          logs[(rq * RQ + r) * LOG_LD + j] = logf(s == 0.f ? FEPS : s);
        }
      }
    }
    __syncthreads();
    // ---- 3c. DCT-II: [32, 322] x [322, 192]; wave w owns cepstrum tiles w and w + 4 (of 6)
    f32x16 cep[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) cep[q][0][r] = 0.f;
    const float* lrow = logs + col * LOG_LD + half;
    const float* dp = a.dct + half * DCT_LD + col + wave * 32;
    if (wave + 4 < DCT_TILES) mma_tiles<NFILT, 2, 1, 7, false>(lrow, dp, DCT_LD, 0, cep);
    else mma_tiles<NFILT, 1, 1, 7, false>(lrow, dp, DCT_LD, 0, cep);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int t = wave + 4 * q, c = t * 32 + col;
      if (t < DCT_TILES && c < NCEP) {
        const float lf = a.lifter[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
          if (row < rows) {
            const float v = c == 0 ? loge[row] : cep[q][0][r] * lf;
            store_out(out + row * NCEP + c, f0 + row < nf ? v : 0.f);
          }
        }
      }
    }
  }
}

template <int KIND, typename IN, typename OUT>
int launch_featurize(const DS2Feat& a, hipStream_t st) {
  auto kern = featurize_kernel<KIND, IN, OUT>;
  constexpr int bytes = Lds<KIND>::FLOATS * (int)sizeof(float);
  static bool attr = false;
  if (!attr) {
    DS2_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    attr = true;
  }
  const dim3 grid((a.T_max + TILE - 1) / TILE, a.B);
  hipLaunchKernelGGL(kern, grid, dim3(NTHR), bytes, st, a);
  return (int)hipGetLastError();
}

template <int KIND, typename IN>
int launch_featurize_out(const DS2Feat& a, int out_bf16, hipStream_t st) {
  return out_bf16 ? launch_featurize<KIND, IN, bf16_t>(a, st) : launch_featurize<KIND, IN, float>(a, st);
}

}  // namespace

extern "C" int ds2_audio_stats(const void* pcm, int in_i16, long long row_stride, int S, int B, const int* lens,
                               float* offset, float* gain, hipStream_t st) {
  if (B <= 0) return 0;
  if (in_i16)
    hipLaunchKernelGGL(audio_stats_kernel<short>, dim3(B), dim3(1024), 0, st, (const short*)pcm, row_stride, S, lens,
                       offset, gain);
  else
    hipLaunchKernelGGL(audio_stats_kernel<float>, dim3(B), dim3(1024), 0, st, (const float*)pcm, row_stride, S, lens,
                       offset, gain);
  return (int)hipGetLastError();
}

// kind 0 = mfcc, 1 = spectrogram
extern "C" int ds2_featurize(const DS2Feat* a, int kind, int in_i16, int out_bf16, hipStream_t st) {
  if (a->B <= 0 || a->T_max <= 0) return 0;
  if (a->B > 65535) return -1;
  if (kind == 0)
    return in_i16 ? launch_featurize_out<0, short>(*a, out_bf16, st) : launch_featurize_out<0, float>(*a, out_bf16, st);
  if (kind == 1)
    return in_i16 ? launch_featurize_out<1, short>(*a, out_bf16, st) : launch_featurize_out<1, float>(*a, out_bf16, st);
  return -1;
}
