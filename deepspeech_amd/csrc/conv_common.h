// Shared layer of the DeepSpeech2 conv front-end for gfx950 (conv1.hip, conv2.hip, bn_cl.hip):
// implicit-GEMM convolutions on MFMA (v_mfma_f32_32x32x16_bf16) with channels-last activations,
// BatchNorm statistics fused into the forward epilogues, and channels-last BatchNorm +
// clipped-ReLU kernels.
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
// MFMA fragments (32x32x16 bf16): lane l holds A[row l&31][k 8(l>>5)+j], B[k 8(l>>5)+j][col l&31],
// accumulator reg r -> row (r&3) + 8(r>>2) + 4(l>>5), col l&31. Each kernel's own mapping of
// rows, columns and k is described at the top of conv1.hip and conv2.hip.
#pragma once
#include "common.h"

// Refusals of the front-end's host launchers: nothing was launched. X(name, value, meaning);
// ds2_conv_status_str (conv2.hip) hands the meaning to the Python error.
#define DS2_CONV_STATUS(X)                                                                                 \
  X(CONV2_F_RANGE, -40, "conv2 needs 5 <= F1 <= 80 and F2 = F1 - 4 (LDS row planes, staging capacity)")    \
  X(CONV2_T_RANGE, -41, "conv2 needs T1 >= 10 and T2 = (T1 - 10) / 2 + 1")                                  \
  X(CONV2_DGRAD_NARROW, -42, "conv2_dgrad needs F1 > 64: it stores positions 0..63 of a row unchecked")     \
  X(CONV1_WGRAD_GEOMETRY, -43, "conv1_wgrad needs F1 = (F0 - 5) / 2 + 1 <= 80, T1 = (T - 20) / 2 + 1 >= 1") \
  X(CONV1_WGRAD_DY_XOR_BN, -44, "conv1_wgrad takes dy or the BatchNorm backward's inputs, exactly one")     \
  X(BN_CL_BWD_WIDE, -45, "bn_cl_bwd needs F <= 96")                                                         \
  X(BN_CL_BWD_TMAJ_READY, -46, "bn_cl_bwd: part_ready excludes tmaj (that path transposes in its reduce)")  \
  X(CONV1_FWD_GEOMETRY, -47, "conv1_fwd needs F1 = (F0 - 5) / 2 + 1 <= 96, T1 = (T - 20) / 2 + 1 >= 1")     \
  X(BN_CL_APPLY_WIDE, -48, "bn_cl_apply needs F <= 96 (one LDS row of the time-major transpose)")

namespace ds2 {

enum ConvStatus : int {
#define X(name, value, meaning) name = value,
  DS2_CONV_STATUS(X)
#undef X
};

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

constexpr int CC = 32;          // channels
constexpr int MT = 3;           // m-tiles of 32 positions (F1, F2 <= 96)
constexpr int C2_KT = 10, C2_KF = 5;

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// accumulator group g (0..3) of one lane: output rows 8 g + 4 (lane >> 5) + 0..3
__device__ __forceinline__ f32x4 acc4(const f32x16& acc, int g) {
  return (f32x4){acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
}

// async 16-B global -> LDS copy; lds_wave_base must be wave-uniform (lane L lands at +16L)
__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

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

// a lane's byte offset into a channels-last LDS image [position][32] bf16 for the transposed
// fragment read of 16 positions x 32 channels, and the fragment itself (positions +0..3, +4..7
// of the lane's k group). lane by reference: by value, conv1_wgrad_kernel took one more register
// (profiles/conv_shared_layer.md)
__device__ __forceinline__ unsigned tr_lane_ofs(const int& lane) {
  const int g = lane >> 4, h = g >> 1, cb = (g & 1) * 16, q = (lane & 15) >> 2, pp = lane & 3;
  return (unsigned)((8 * h + q) * 64 + (cb + 4 * pp) * 2);
}
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p) { return cat8(tr_read(p), tr_read(p + 4 * 64)); }

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// tiles of a persistent grid: X contiguous ranges (one per XCD when the grid is a multiple of 8;
// workgroup b runs on XCD b % 8), dealt round-robin to that XCD's workgroups, so the input rows
// neighbouring tiles share are L2 hits. This workgroup runs first, first + per, ... < hi.
struct TileRange {
  int first, hi, per;
};
__device__ __forceinline__ TileRange xcd_tiles(int ntiles) {
  const int X = (gridDim.x % 8 == 0) ? 8 : 1;
  const int per = (int)gridDim.x / X, xi = (int)blockIdx.x % X, wi = (int)blockIdx.x / X;
  const int t_lo = (int)((long long)ntiles * xi / X), t_hi = (int)((long long)ntiles * (xi + 1) / X);
  return {t_lo + wi, t_hi, per};
}

// per-tile phase stamps of workgroups 0..7 (wave 0, lane 0) of the persistent conv2 kernels: tile
// start, rows landed, MFMA loop done, partial sums reduced, outputs stored, next tile's rows
// issued (tools/conv_timeline.py); tr: optional [8 workgroups][16 tiles][C2_TRACE]
constexpr int C2_TRACE = 6;
__device__ __forceinline__ void c2_stamp(long long* tr, int it, int k) {
  if (tr != nullptr && blockIdx.x < 8 && threadIdx.x == 0 && it < 16)
    tr[((int)blockIdx.x * 16 + it) * C2_TRACE + k] = __builtin_amdgcn_s_memrealtime();
}

// one bf16 output row out of LDS in 16-B chunks first, first + step, ... < chunks
__device__ __forceinline__ void copy_row(bf16_t* dst, const void* lds_row, int chunks, int first, int step) {
  for (int q = first; q < chunks; q += step) ((i32x4*)dst)[q] = ((const i32x4*)lds_row)[q];
}

// per-workgroup channel sums of two per-lane values (4 waves; lanes l and l ^ 32 hold the same
// channel l & 31) -> part[blockIdx][32][2]; sh: LDS [4][32][2], w: the calling wave
__device__ __forceinline__ void channel_sums(float s, float q, float* sh, int w, float* part) {
  const int tid = threadIdx.x, lane = tid & 63;
  s += __shfl_xor(s, 32, 64);
  q += __shfl_xor(q, 32, 64);
  __syncthreads();
  if (lane < 32) {
    sh[(w * 32 + lane) * 2 + 0] = s;
    sh[(w * 32 + lane) * 2 + 1] = q;
  }
  __syncthreads();
  if (tid < 64) part[(size_t)blockIdx.x * 64 + tid] = sh[tid] + sh[64 + tid] + sh[128 + tid] + sh[192 + tid];
}

template <typename K>
int set_smem(K kernel, size_t bytes) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}

}  // namespace ds2

namespace {

// sum of per-workgroup partials (fragment order) -> dw in OIHW, KIND 0: conv2 [32][32][10][5],
// KIND 1: conv1 [32][1][20][5]. A block owns 256 consecutive elements (64 f32x4 columns)
// and 4 interleaved groups of partials, so every thread keeps several 16-B loads in flight.
// (Each weight-gradient file instantiates its own KIND.)
template <int KIND>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int nb, int E,
                                                           float* __restrict__ dw) {
  using namespace ds2;
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

}  // namespace
