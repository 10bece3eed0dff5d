// Element-level BatchNorm + clipped-ReLU formulas, one definition each, for the channels-last
// kernels (bn_cl.hip), the fused conv epilogues (conv2.hip dgrad, conv1.hip wgrad staging) and
// the NCHW kernels (bn_act.hip). The fused paths are tested bitwise against the separate
// passes, so the operation order written here is part of the contract.
//
// Training-mode backward: dbeta = sum(dz*m), dgamma = sum(dz*m*xhat),
// dy = gamma*invstd*(dz*m - dbeta/M - xhat*dgamma/M), m = clip mask. The conv bias gradient is
// identically zero under train-mode BN (the mean subtraction cancels any shift).
#pragma once
#include "common.h"

namespace ds2 {

constexpr float CLIP = 20.0f;

// forward: z = clip(y * sc + sh) with the per-channel scale and shift
__device__ __forceinline__ void bn_scale_shift(float mean, float invstd, float gamma, float beta, float& sc,
                                               float& sh) {
  sc = invstd * gamma;
  sh = beta - mean * sc;
}
__device__ __forceinline__ float bn_clip(float y, float sc, float sh) { return fminf(fmaxf(y * sc + sh, 0.f), CLIP); }

__device__ __forceinline__ float bn_xhat(float y, float mean, float invstd) { return (y - mean) * invstd; }

// true where the clipped ReLU passes the gradient: 0 < BN(y) < CLIP
__device__ __forceinline__ bool bn_unclipped(float xh, float gamma, float beta) {
  const float z = xh * gamma + beta;
  return z > 0.f && z < CLIP;
}
// dz * m
__device__ __forceinline__ float bn_masked(float xh, float gamma, float beta, float dz) {
  return bn_unclipped(xh, gamma, beta) ? dz : 0.f;
}

// backward apply; k = gamma * invstd, mdb = dbeta / M, mdg = dgamma / M, dd = dz * m
__device__ __forceinline__ float bn_bwd_value(float k, float dd, float xh, float mdb, float mdg) {
  return k * (dd - mdb - xh * mdg);
}

}  // namespace ds2
