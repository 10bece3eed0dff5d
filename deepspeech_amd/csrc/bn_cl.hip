// Channels-last BatchNorm (+ clipped ReLU) of the DeepSpeech2 conv front-end for gfx950, forward
// and backward, on activations [N][T][F][32] bf16 (layouts: conv_common.h; formulas: bn_math.h).
// The forward statistics come from the conv epilogues as per-workgroup partials part[nb][32][2].
#include "bn_math.h"
#include "conv_common.h"

using namespace ds2;

namespace {

// fp64 sums over b of part[b][c][0] and part[b][c][1] by one 256-thread block; thread 0 hands
// them to tail(s, q), the kernel's own scalar work
template <typename Tail>
__device__ __forceinline__ void part_column_sums(const float* __restrict__ part, int nb, int c, Tail tail) {
  __shared__ double sh[2][4];
  const int tid = threadIdx.x;
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
  if (tid == 0) tail(sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3], sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
}

// one flat stream of the 16-B chunks of y and dz, whose channel octet is (chunk & 3) = (tid & 3)
// (the grid stride is a multiple of 4), 4 chunks of each operand in flight per thread: f(chunk, y, dz)
template <typename F>
__device__ __forceinline__ void stream4(const bf16_t* y, const bf16_t* dz, long long total, F f) {
  const long long step = (long long)gridDim.x * 256;
  const bf16x8 *y8 = (const bf16x8*)y, *d8 = (const bf16x8*)dz;
  long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; e + 3 * step < total; e += 4 * step) {
    bf16x8 v[4], d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = y8[e + k * step]; d[k] = d8[e + k * step]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) f(e + k * step, v[k], d[k]);
  }
  for (; e < total; e += step) f(e, y8[e], d8[e]);
}

// part [nb][32][2] -> mean / invstd (+ running stats, unbiased variance, momentum)
__global__ __launch_bounds__(256) void bn_cl_finalize_kernel(const float* __restrict__ part, int nb, double M,
                                                             float eps, float* mean, float* invstd, float* run_mean,
                                                             float* run_var, float momentum) {
  const int c = blockIdx.x;
  part_column_sums(part, nb, c, [&](double s, double q) {
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
  });
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
  for (int j = 0; j < 8; ++j) bn_scale_shift(mean[c0 + j], invstd[c0 + j], gamma[c0 + j], beta[c0 + j], sc[j], sh[j]);
  for (long long ch = (long long)blockIdx.x * 256 + threadIdx.x; ch < nchunks; ch += (long long)gridDim.x * 256) {
    const bf16x8 v = *(const bf16x8*)(y + ch * 8);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(bn_clip(bf2f((bf16_t)v[j]), sc[j], sh[j]));
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
  for (int j = 0; j < 8; ++j) bn_scale_shift(mean[c0 + j], invstd[c0 + j], gamma[c0 + j], beta[c0 + j], sc[j], sh[j]);
  for (int row = blockIdx.x; row < N * T; row += gridDim.x) {
    const int n = row / T, t = row - n * T;
    const bf16_t* yr = y + (size_t)row * F * CC;
    __syncthreads();
    for (int ch = tid; ch < F * 4; ch += 256) {
      const int f = ch >> 2;
      const bf16x8 v = *(const bf16x8*)(yr + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) tr[(c0 + j) * stride + f] = f2bf(bn_clip(bf2f((bf16_t)v[j]), sc[j], sh[j]));
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
  auto acc8 = [&](long long, const bf16x8 v, const bf16x8 d) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = bn_xhat(bf2f((bf16_t)v[j]), mu[j], is[j]);
      const float dd = bn_masked(xh, g[j], bt[j], bf2f((bf16_t)d[j]));
      s[j] += dd;
      q[j] += dd * xh;
    }
  };
  const long long total = (long long)N * T * F * 4;
  if (!tmaj) {
    stream4(y, dz, total, acc8);
  } else {
    // time-major dz [T][N][c * F + f]: chunk e of the channels-last stream is (row = n * T + t,
    // position f, channels 8 (e & 3) ..): its 8 dz values are one time-major row's elements
    // c * F + f (a 2-byte gather from one cache-resident row), and the channels-last copy the
    // apply pass reads is written as one 16-B chunk. No LDS and no barriers, so the kernel
    // streams beside the grouped weight-gradient GEMM in the step's tail.
    const long long step = (long long)gridDim.x * 256;
    const bf16x8* y8 = (const bf16x8*)y;
    for (long long e = (long long)blockIdx.x * 256 + tid; e < total; e += step) {
      const long long rowf = e >> 2;
      const int row = (int)(rowf / F), f = (int)(rowf - (long long)row * F);
      const int n = row / T, t = row - n * T;
      const bf16_t* dr = dz + ((size_t)t * N + n) * CC * F + f;
      bf16x8 d;
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = (short)dr[(c0 + j) * F];
      if (dz_cl != nullptr) ((bf16x8*)dz_cl)[e] = d;
      acc8(e, y8[e], d);
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
  const int c = blockIdx.x;
  part_column_sums(part, nb, c, [&](double s, double q) {
    dbeta[c] = (float)s;
    dgamma[c] = (float)q;
  });
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
      const float xh = bn_xhat(bf2f((bf16_t)v[j]), mu[j], is[j]);
      const float dd = bn_masked(xh, g[j], bt[j], bf2f((bf16_t)d[j]));
      o[j] = (short)f2bf(bn_bwd_value(g[j] * is[j], dd, xh, mdb[j], mdg[j]));
    }
    return o;
  };
  stream4(y, dz, (long long)N * T * F * 4,
          [&](long long e, const bf16x8 v, const bf16x8 d) { ((bf16x8*)dy)[e] = one(v, d); });
}

}  // namespace

extern "C" {

int ds2_bn_cl_finalize(const float* part, int nb, double M, float eps, float* mean, float* invstd, float* run_mean,
                       float* run_var, float momentum, hipStream_t st) {
  hipLaunchKernelGGL(bn_cl_finalize_kernel, dim3(CC), dim3(256), 0, st, part, nb, M, eps, mean, invstd, run_mean,
                     run_var, momentum);
  return (int)hipGetLastError();
}

int ds2_bn_cl_apply(const void* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                    void* out, int N, int T, int F, int tmaj, hipStream_t st) {
  if (F > 96) return BN_CL_APPLY_WIDE;
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
  if (F > 96) return BN_CL_BWD_WIDE;
  if (part_ready && tmaj) return BN_CL_BWD_TMAJ_READY;
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
