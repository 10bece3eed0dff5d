// Device half of the persistent recurrence that the generations share (rnn_xcd.hip,
// rnn_fp8.hip): group placement and start-up, the sentinel / tag hand-off tests, granule
// stores, the fused direction sum, the h pack, the BPTT ring addressing and pair publish, the
// stamps, and the forward memory wave's step schedule. One definition each. Still per kernel,
// because sharing them cost registers or occupancy (profiles/recurrence_shared_layer.md): the
// memory waves' load / put / store bodies and the MFMA chains in front of publish_pair.
// The exchange protocol itself is described once, at the head of rnn_xcd.hip.
#pragma once
#include <type_traits>

#include "common.h"

namespace ds2 {

// Phase stamps (diagnostics; a null stamps pointer costs one uniform branch per phase).
struct Stamps {
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long prev = 0;
  bool on;
  __device__ explicit Stamps(bool o) : on(o) {}
  __device__ __forceinline__ void mark(int i) {
    if (!on) return;
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    if (prev && i >= 0) acc[i] += t - prev;
    prev = t;
  }
  __device__ __forceinline__ void store(unsigned long long* dst, int base) {
    if (!on) return;
    for (int k = 0; k < 6; ++k) dst[(size_t)blockIdx.x * 8 + base + k] = acc[k];
  }
};

// compile-time-off variant: the stamp accumulators would otherwise hold ~14 VGPRs of every
// wave for the whole launch (enough to push a 3-waves-per-SIMD kernel into spilling)
struct NoStamps {
  unsigned long long acc[6];
  bool on = false;
  __device__ explicit NoStamps(bool) {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void store(unsigned long long*, int) {}
};

// End of launch: the recorded MFMA wave (w0) writes its six phase sums and the group's store
// mode, the memory wave (wm) its two. Nothing for NoStamps (its `on` is a constant false, so the
// unconditional flush of the kernels that always carry Stamps is the same code). s_mode is
// the __shared__ word, by reference so that it is read only by the wave that stores it.
template <typename StampT>
__device__ __forceinline__ void stamp_flush(StampT& st, unsigned long long* stamps, int wave, int w0, int wm,
                                            const int& s_mode) {
  if constexpr (std::is_same<StampT, Stamps>::value) {
    if (wave == w0) { st.acc[5] = (unsigned long long)(s_mode + 10); st.store(stamps, 0); }
    if (wave == wm && st.on) { stamps[(size_t)blockIdx.x * 8 + 6] = st.acc[0]; stamps[(size_t)blockIdx.x * 8 + 7] = st.acc[1]; }
  }
}

__device__ __forceinline__ unsigned xcc_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 0xf;
}

// no 16-bit half of the granule is the sentinel 0xFFFF: SWAR "has a zero half" test on the
// complement, (~w - 0x00010001) & w & 0x80008000 (a few VALU ops per dword; this check runs
// on every poll of the latency-critical exchange)
__device__ __forceinline__ bool granule_ready(i32x4 v) {
  unsigned any = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned w = (unsigned)v[i];
    any |= (~w - 0x00010001u) & w & 0x80008000u;
  }
  return any == 0;
}

// no byte of the granule is the e4m3 sentinel 0xFF: SWAR "has a zero byte" on the complement
__device__ __forceinline__ bool granule8_ready(i32x4 v) {
  unsigned any = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned w = ~(unsigned)v[i];
    any |= (w - 0x01010101u) & ~w & 0x80808080u;
  }
  return any == 0;
}

// A ring word carries its use tag in the mantissa LSB (see ring_tag): the fp32 granule is
// ready when all four words carry the expected tag. (Tagged bf16 pairs: granule_tagged16.)
__device__ __forceinline__ bool granule_tagged(i32x4 v, unsigned tag) {
  return (((unsigned)v[0] & 1u) == tag) && (((unsigned)v[1] & 1u) == tag) && (((unsigned)v[2] & 1u) == tag) &&
         (((unsigned)v[3] & 1u) == tag);
}

// plain (the group shares an XCD: L2-resident) or write-through
__device__ __forceinline__ void store_granule(bool plain, __amdgpu_buffer_rsrc_t rs, unsigned off, i32x4 v) {
  if (plain) {
    store_b128(rs, off, v);
  } else {
    store_sc1_b128(rs, off, v);
  }
}

// Explicit vmcnt(0) at a poll's exits. Every load of the poll has been waited for there
// already (the last check consumed it), but the CFG also has an edge from a re-issue to the
// exit, so the waitcnt pass assumed loads in flight and put a vmcnt(0) at the head of the
// NEXT step — behind the step's own h store, whose write acknowledgement then delayed the
// next step's first poll by an L2 round trip. A counted wait here costs nothing (nothing is
// in flight) and tells the pass so.
__device__ __forceinline__ void drain_vm() {
#ifndef DS2_NO_DRAIN          // A/B: build.py --variant nodrain -D DS2_NO_DRAIN
  __builtin_amdgcn_s_waitcnt(0x0F70);
#endif
}

// Group role. xcd_map (host-chosen: <= 8 groups of <= CUs/8 members): group =
// blockIdx % 8, so under round-robin dispatch a group shares one XCD; otherwise groups
// are contiguous block ranges. Returns false for surplus blocks (no role).
__device__ __forceinline__ bool take_role(int xcd_map, int ngroups, int P, int& grp, int& mem) {
  if (xcd_map) {
    const int slot = blockIdx.x & 7;
    if (slot >= ngroups) return false;
    grp = slot;
    mem = blockIdx.x >> 3;
  } else {
    grp = blockIdx.x / P;
    mem = blockIdx.x % P;
  }
  return mem < P;
}

// Every member of the group publishes its XCC id; the group is "local" iff all agree.
// Runs on wave 0; returns 1 (local), 0 (spread) or -1 (timeout).
__device__ inline int group_census(unsigned* census, int grp, int mem, int P, long long timeout, unsigned* err) {
  const int lane = threadIdx.x & 63;
  unsigned* c = census + (size_t)grp * P;
  if (lane == 0) __hip_atomic_store(c + mem, xcc_id(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const long long t0 = __builtin_amdgcn_s_memrealtime();
  while (true) {
    bool ready = true;
    unsigned first = 0xffffffffu;
    bool same = true;
    for (int q = lane; q < P; q += 64) {
      const unsigned v = __hip_atomic_load(c + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ready = ready && (v != 0xffffffffu);
      if (q == lane) first = v;
      same = same && (v == first);
    }
    if (__all(ready)) {
      const unsigned x0 = __shfl(first, 0, 64);
      const bool all_same = __all(same && (lane >= P || first == x0));
      return all_same ? 1 : 0;
    }
    if (__builtin_amdgcn_s_memrealtime() - t0 > timeout) {
      if (lane == 0) atomicOr(err, 2u);
      return -1;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// Start of every persistent kernel: the utterance length of each of the group's rows
// (0 = padding row) into len_s, and wave 0's census result into s_mode (1 = plain stores)
// and s_abort. The caller's next __syncthreads() publishes all three; it returns if s_abort
// is set. a: the kernel's argument struct (lens, census, timeout, err, knobs), read where it
// is used. WT_KNOB: the bit of a.knobs that demotes a local group to write-through (a timing
// knob; 0 for the callers that have none). Kernels that fill other LDS tables between the two
// halves call group_lens and group_mode themselves. rnnq_fwd_kernel keeps the block inline:
// through the helper its ReLU instantiations lose occupancy (see the profile).
template <int ROWS, typename Args>
__device__ __forceinline__ void group_lens(int (&len_s)[ROWS], const Args& a, int r0, int R, int N) {
  const int tid = threadIdx.x;
  if (tid < ROWS) len_s[tid] = (tid < R && r0 + tid < N) ? a.lens[r0 + tid] : 0;
}
template <int WT_KNOB = 0, typename Args>
__device__ __forceinline__ void group_mode(int& s_mode, int& s_abort, const Args& a, int grp, int mem, int P,
                                           int wave) {
  if (wave == 0) {
    int m = group_census(a.census, grp, mem, P, a.timeout, a.err);
    if constexpr (WT_KNOB != 0)
      if ((a.knobs & WT_KNOB) && m > 0) m = 0;
    if ((threadIdx.x & 63) == 0) { s_mode = m; s_abort = (m < 0); }
  }
}
template <int WT_KNOB = 0, int ROWS, typename Args>
__device__ __forceinline__ void group_start(int (&len_s)[ROWS], int& s_mode, int& s_abort, const Args& a, int r0,
                                            int R, int N, int grp, int mem, int P, int wave) {
  group_lens(len_s, a, r0, R, N);
  group_mode<WT_KNOB>(s_mode, s_abort, a, grp, mem, P, wave);
}

// Fused direction sum (reference: the fw + bw outputs summed by the caller,
// src/custom_ops.py:36-96). Position t is produced by the forward direction at step t and by
// the backward one at step L-1-t (padding positions: both at step t). The direction that
// produces it LATER (ties: the backward one) waits for the other's bf16 value in the
// sentinel-filled sum buffer and writes the bf16 sum, rounding exactly like bf16 + bf16 in
// torch; the earlier one writes its value through (sc1: the other direction's groups live on
// other XCDs). No cycle: the later side of a pair only waits for a step the earlier side
// reached first.
// p: this lane's 4 units of the position; o: its own 4 bf16 values; preloaded: what an
// earlier load of *p returned (usually the other direction's value already); a: the kernel's
// argument struct (timeout, err), read only on the timeout path.
template <typename Args>
__device__ __forceinline__ void dirsum_store(unsigned long long* p, uint2 o, const unsigned long long& preloaded,
                                             bool later, const Args& a) {
  auto canon = [](unsigned h) { return (h & 0xffffu) == 0xffffu ? 0x7fc0u : (h & 0xffffu); };
  if (!later) {
    o.x = canon(o.x) | (canon(o.x >> 16) << 16);
    o.y = canon(o.y) | (canon(o.y >> 16) << 16);
    __hip_atomic_store(p, ((unsigned long long)o.y << 32) | o.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    const long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long q = preloaded;
    while (true) {
      const unsigned w0 = (unsigned)q, w1 = (unsigned)(q >> 32);
      const bool ready = ((~w0 - 0x00010001u) & w0 & 0x80008000u) == 0 &&
                         ((~w1 - 0x00010001u) & w1 & 0x80008000u) == 0;
      if (ready) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout) { atomicOr(a.err, 4u); break; }
      __builtin_amdgcn_s_sleep(2);
      q = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned q0 = (unsigned)q, q1 = (unsigned)(q >> 32);
    auto add2 = [](unsigned x, unsigned y) {      // two bf16 pairs -> rounded bf16 sums
      const unsigned lo = f2bf(__uint_as_float(x << 16) + __uint_as_float(y << 16));
      const unsigned hi = f2bf(__uint_as_float(x & 0xffff0000u) + __uint_as_float(y & 0xffff0000u));
      return lo | (hi << 16);
    };
    *reinterpret_cast<uint2*>(p) = make_uint2(add2(o.x, q0), add2(o.y, q1));
  }
}

// New h of this lane -> bf16 (hardware RNE; 0xFFFF, the sentinel and a negative NaN, becomes
// the canonical NaN), then the 16-B exchange granule = 8 consecutive units of one row = 8
// consecutive lanes, assembled with DPP row shifts instead of an LDS round trip + fence. Only
// lanes with lane % 8 == 0 hold a whole granule; they publish it with store_granule.
__device__ __forceinline__ i32x4 pack_h(float hnew) {
  unsigned hq = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)hnew);
  hq = hq == 0xffffu ? 0x7fc0u : hq;
  const unsigned pr = hq | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)hq, 0x101, 0xf, 0xf, false) << 16);
  const int q1 = __builtin_amdgcn_update_dpp(0, (int)pr, 0x102, 0xf, 0xf, false);
  const int q2 = __builtin_amdgcn_update_dpp(0, (int)pr, 0x104, 0xf, 0xf, false);
  const int q3 = __builtin_amdgcn_update_dpp(0, (int)pr, 0x106, 0xf, 0xf, false);
  return i32x4{(int)pr, q1, q2, q3};
}

// BPTT ring. Use tag of P(s): slot s % 3 is written at processing index k = steps-1-s, so
// its uses are k, k+3, k+6, ... and (k / 3) & 1 alternates between consecutive uses; the ring
// is filled with 0xFFFFFFFF (tag 1) and every slot's first use has tag 0.
__device__ __forceinline__ unsigned ring_tag(int steps, int s) { return (unsigned)(((steps - 1 - s) / 3) & 1); }
// Byte offset in the bf16 ring [slot][bg][producer j][unit pair pr of NPR][row of R][g 0..3]
// [8 bf16]: granule (row, g) of pair pr holds units 32 pr + {4g..4g+3, 16+4g..16+4g+3}.
__device__ __forceinline__ unsigned ring_off16(int BG, int bg, int P, int NPR, int R, int slot, int j, int pr,
                                               int row, int g) {
  return (unsigned)((((((size_t)slot * BG + bg) * P + j) * NPR + pr) * R + row) * 4 + g) * 16u;
}

// Publish of one unit pair: two 16x16 accumulators (m-tiles 2p, 2p+1) -> one tagged-bf16
// granule per lane. The store flavour is a compile-time branch of the caller's whole publish
// loop (a runtime one per store cost a select + compare + 3 scalar branches per pair).
template <bool PLAIN>
__device__ __forceinline__ void publish_pair(__amdgpu_buffer_rsrc_t rs, unsigned off, const f32x4& a0,
                                             const f32x4& a1, unsigned tagmask) {
  const i32x4 v = {(int)bf16x2_tagged(a0[0], a0[1], tagmask), (int)bf16x2_tagged(a0[2], a0[3], tagmask),
                   (int)bf16x2_tagged(a1[0], a1[1], tagmask), (int)bf16x2_tagged(a1[2], a1[3], tagmask)};
  if constexpr (PLAIN) store_b128(rs, off, v);
  else store_sc1_b128(rs, off, v);
}

// ------------------------------------------------------------------------------------
// Forward memory wave. It keeps every bulk load and store out of the MFMA waves' vmcnt queues
// (vmcnt retires in order per wave): the step's input projection gx goes two steps ahead into
// registers and one step ahead into a two-slot LDS ring (zero past each utterance's length),
// and a step's outputs leave two steps behind out of a two-slot LDS staging area. Per step s,
// before the step's barrier:   ysum_load(s - 2); put(s + 1); store(s - 2); load(s + 2)
// after the prologue (load 0, put 0, load 1) and before a drain of the last two stores.
// ------------------------------------------------------------------------------------
template <typename LoadFn, typename PutFn>
__device__ __forceinline__ void mw_prologue(int steps, LoadFn&& load, PutFn&& put) {
  load(0);
  put(0);
  if (steps > 1) load(1);
}
template <typename YsumFn, typename PutFn, typename StoreFn, typename LoadFn>
__device__ __forceinline__ void mw_step(int s, int steps, bool ysum, YsumFn&& ysum_load, PutFn&& put, StoreFn&& store,
                                        LoadFn&& load, bool stores = true) {
  if (ysum && s >= 2) ysum_load(s - 2);
  if (s + 1 < steps) put(s + 1);
  if (s >= 2 && stores) store(s - 2);
  if (s + 2 < steps) load(s + 2);
}
template <typename YsumFn, typename StoreFn>
__device__ __forceinline__ void mw_drain(int steps, bool ysum, YsumFn&& ysum_load, StoreFn&& store) {
  if (steps >= 2) {
    if (ysum) ysum_load(steps - 2);
    store(steps - 2);
  }
  if (steps >= 1) {
    if (ysum) ysum_load(steps - 1);
    store(steps - 1);
  }
}

}  // namespace ds2
