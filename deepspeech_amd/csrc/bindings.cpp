// Python bindings of the deepspeech_amd gfx950 kernels (module deepspeech_amd._C).
//
// The .hip translation units expose plain extern "C" launchers that take raw pointers
// and a hipStream_t; this file states what each kernel assumes of each tensor (device,
// dtype, size, layout) in the vocabulary of bind_args.h, the only place a tensor becomes a
// pointer, and launches on PyTorch's current HIP stream, so every op composes with torch
// streams and can be captured into a hipGraph.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "api.h"
#include "bind_args.h"

namespace {

// the conv front-end's launchers: the message also says what was refused
void conv_launched(const Op& op, int rc) {
  const char* why = ds2_conv_status_str(rc);
  TORCH_CHECK(rc == 0, "deepspeech_amd kernel launch failed in ", op.op, " (code ", rc, ")", why ? ": " : "",
              why ? why : "");
}

// ---- cross-stream ordering on one device ------------------------------------------------
// Events keep the default (system-scope) fences: with hipEventReleaseToDevice the next kernel
// on the waiting queue could read lines another XCD's L2 still held stale (the ReLU
// convergence test drifted 6-8 %), and the device-scope marker measured no cheaper (~6 us per
// record or wait either way, tools/probe_event_gap.py). What these helpers save is the event
// object churn of torch's wait_stream.
constexpr unsigned kLightEvent = hipEventDisableTiming;

int64_t event_new(unsigned flags) {
  hipEvent_t e = nullptr;
  TORCH_CHECK(hipEventCreateWithFlags(&e, flags ? flags : kLightEvent) == hipSuccess, "hipEventCreateWithFlags");
  return (int64_t)(intptr_t)e;
}
void event_free(int64_t e) { (void)hipEventDestroy((hipEvent_t)(intptr_t)e); }
void event_record(int64_t e, int64_t stream) {
  TORCH_CHECK(hipEventRecord((hipEvent_t)(intptr_t)e, (hipStream_t)(intptr_t)stream) == hipSuccess, "hipEventRecord");
}
void event_wait(int64_t stream, int64_t e) {
  TORCH_CHECK(hipStreamWaitEvent((hipStream_t)(intptr_t)stream, (hipEvent_t)(intptr_t)e, 0) == hipSuccess,
              "hipStreamWaitEvent");
}
bool event_query(int64_t e) { return hipEventQuery((hipEvent_t)(intptr_t)e) == hipSuccess; }

// The next kernel launched through ds2_launch (the GEMMs, the BPTT, multi_fill) completes event
// e itself (hipExtLaunchKernel stop event) instead of a marker packet recorded behind it.
// disarm_stop_event: True if no launch took it (the op ran elsewhere: record it the usual way).
void arm_stop_event(int64_t e) { ds2_arm_stop_event((hipEvent_t)(intptr_t)e); }
bool disarm_stop_event() { return ds2_take_stop_event() != nullptr; }

// dst waits for everything enqueued on src so far: record + wait back to back, so one cached
// event per host thread and device serves every pair (the wait binds to the record just made)
void stream_wait(int64_t dst, int64_t src) {
  if (dst == src) return;
  static thread_local hipEvent_t evs[64] = {};
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "hipGetDevice");
  if (evs[dev] == nullptr) TORCH_CHECK(hipEventCreateWithFlags(&evs[dev], kLightEvent) == hipSuccess, "event");
  TORCH_CHECK(hipEventRecord(evs[dev], (hipStream_t)(intptr_t)src) == hipSuccess, "hipEventRecord");
  TORCH_CHECK(hipStreamWaitEvent((hipStream_t)(intptr_t)dst, evs[dev], 0) == hipSuccess, "hipStreamWaitEvent");
}

// --------------------------------------------------------------------------- RNN
// Every recurrence descriptor (csrc/api.h) is filled the same way: the geometry from the 12
// integers of ops/rnn.py _geom, the buffers Python allocates stacked [ndir, ...] through
// dir_ptrs, the bias partials through bias_parts. U and bh are separate arena parameters and
// come as per-direction pairs (pair_ptrs).
template <typename D>
D rnn_desc(const Op& op, const std::vector<int64_t>& g, const at::Tensor& lens, const at::Tensor& err, int64_t timeout) {
  TORCH_CHECK(g.size() == 12, "recurrence geometry: the 12 integers of ops/rnn.py _geom");
  D d{};
  static_cast<DS2RnnGeom&>(d) = DS2RnnGeom{(int)g[0], (int)g[1], (int)g[2], (int)g[3], (int)g[4],  (int)g[5],
                                           (int)g[6], (int)g[7], (int)g[8], (int)g[9], (int)g[10], (int)g[11]};
  TORCH_CHECK(d.T >= 0 && d.N >= 1 && d.NP >= d.N && d.BG >= 1 && d.H >= 32 && d.H % 32 == 0 && d.steps <= d.T &&
                  (d.ndir == 1 || d.ndir == 2) && (d.cell == 0 || d.cell == 1),
              "recurrence geometry out of range");
  d.lens = op.i32(lens, "lens", "N", exactly(d.N));
  d.err = op.u32(err, "err", "1", at_least(1));
  d.timeout = timeout;
  return d;
}

// The direction pointers of a stacked buffer [ndir, per_dir elements]: of exactly that size
// (or_more: or larger, for state a longer launch saved; the directions then lie numel / ndir
// apart). Directions past ndir stay null; so do both for None.
template <typename P>
void dir_ptrs(const Op& op, P* (&out)[2], const OptT& t, const char* name, at::ScalarType dtype, int64_t ndir,
              int64_t per_dir, bool or_more = false) {
  char* base = static_cast<char*>(op.raw(t, name, dtype, "ndir, per_dir", Count{ndir * per_dir, or_more}));
  const int64_t n = base ? t->numel() : 0;
  TORCH_CHECK(n % ndir == 0, op.op, ": ", name, " must be ", dtype, " [ndir, per_dir or more]: ", n, " elements do not split into ",
              ndir, " directions");
  for (int i = 0; i < 2; ++i) out[i] = base && i < ndir ? reinterpret_cast<P*>(base + i * (n / ndir) * t->element_size()) : nullptr;
}

// Bias-gradient partials fp32 [k, ndir, BG, G*H] (k = 0 the input bias, k = 1 the GRU's
// recurrent bias) or none: per_dir = BG * G * H
void bias_parts(const Op& op, float* (&bx)[2], float* (&bh)[2], const OptT& parts, int64_t k, int64_t ndir, int64_t per_dir) {
  float* by_k[2];
  dir_ptrs(op, by_k, parts, "bias partials", at::kFloat, k, ndir * per_dir);
  for (int i = 0; i < 2; ++i) {
    bx[i] = (by_k[0] && i < ndir) ? by_k[0] + i * per_dir : nullptr;
    bh[i] = (by_k[1] && i < ndir) ? by_k[1] + i * per_dir : nullptr;
  }
}

// a per-direction parameter pair: U bf16 [G*H, H], bh fp32 [G*H]
template <typename P>
void pair_ptrs(const Op& op, P* (&out)[2], const OptT& f, const OptT& b, const char* name, at::ScalarType dtype,
               const char* shape, int64_t n, int ndir, bool required) {
  out[0] = static_cast<P*>(op.raw(f, name, dtype, shape, exactly(n)));
  out[1] = ndir == 2 ? static_cast<P*>(op.raw(b, name, dtype, shape, exactly(n))) : nullptr;
  TORCH_CHECK(!required || (out[0] && (ndir == 1 || out[1])), op.op, ": ", name, ": a direction's tensor is missing");
}
template <typename D>
void rnn_U(const Op& op, D& d, const OptT& U_f, const OptT& U_b) {
  pair_ptrs(op, d.U, U_f, U_b, "U", at::kBFloat16, "G*H, H", (d.cell == 1 ? 3 : 1) * (int64_t)d.H * d.H, d.ndir, true);
}
template <typename D>
void rnn_bh(const Op& op, D& d, const OptT& bh_f, const OptT& bh_b) {
  pair_ptrs(op, d.bh, bh_f, bh_b, "bh", at::kFloat, "G*H", (d.cell == 1 ? 3 : 1) * (int64_t)d.H, d.ndir, false);
}

// bf16 [T, N, row] activations / gradients beside the recurrence: gx, dy, dgx (or more: the
// projection's output may be the larger buffer of a longer batch)
void* need_seq(const Op& op, const at::Tensor& t, const char* name, const DS2RnnGeom& d, int64_t row, bool exact = false) {
  return op.bf16(t, name, "T, N, row", Count{(int64_t)d.T * d.N * row, !exact});
}

// saved state of the forward: fp32 h [ndir, steps+1, NP, H] and (GRU) gates [ndir, steps, NP, 4H],
// or more (a longer launch's buffers)
template <typename D>
void rnn_saved(const Op& op, D& d, const OptT& hs, const OptT& gates) {
  dir_ptrs(op, d.hsave, hs, "hs", at::kFloat, d.ndir, (int64_t)(d.steps + 1) * d.NP * d.H, true);
  dir_ptrs(op, d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4, true);
  TORCH_CHECK(d.hsave[0] && (d.cell == 0 || d.gates[0]), op.op, ": hs is required, and GRU needs gate buffers");
}

// optional diagnostics: int64 [workgroups, 8] phase stamps
unsigned long long* stamps_ptr(const Op& op, const OptT& stamps, int64_t grid) {
  return reinterpret_cast<unsigned long long*>(op.i64(stamps, "stamps", "workgroups, 8", exactly(grid * 8)));
}

// ---- generation 1 (csrc/rnn_persistent.hip): 16*mt-row tiles, one flag word per workgroup
template <typename D>
D rnn1_desc(const Op& op, const std::vector<int64_t>& g, const at::Tensor& lens, const at::Tensor& err, int64_t timeout,
            int64_t nw, int64_t mt, bool persistent, const at::Tensor& flags, const OptT& stamps) {
  D d = rnn_desc<D>(op, g, lens, err, timeout);
  TORCH_CHECK(d.NP == d.BG * 16 * mt, "NP must equal BG*16*mt");
  d.S = d.H / 16; d.nw = (int)nw; d.mt = (int)mt; d.persistent = persistent ? 1 : 0;
  d.flags = op.u32(flags, "flags", "ndir, BG, S", at_least((int64_t)d.ndir * d.BG * d.S));
  d.stamps = stamps_ptr(op, stamps, (int64_t)d.ndir * d.BG * d.S);
  return d;
}

void rnn_fwd(std::vector<int64_t> geom, int64_t nw, int64_t mt, bool persistent, at::Tensor gx, at::Tensor lens,
             OptT U_f, OptT U_b, OptT bh_f, OptT bh_b, at::Tensor y, at::Tensor hx, at::Tensor hs, OptT gates,
             at::Tensor flags, at::Tensor err, int64_t timeout, OptT stamps) {
  const Op op{"rnn_fwd"};
  DS2RnnFwd d = rnn1_desc<DS2RnnFwd>(op, geom, lens, err, timeout, nw, mt, persistent, flags, stamps);
  d.gx = need_seq(op, gx, "gx", d, d.gstride);
  rnn_U(op, d, U_f, U_b);
  rnn_bh(op, d, bh_f, bh_b);
  dir_ptrs(op, d.y, y, "y", at::kBFloat16, d.ndir, (int64_t)d.T * d.N * d.H);
  dir_ptrs(op, d.hx, hx, "hx", at::kBFloat16, d.ndir, (int64_t)(d.steps + 1) * d.NP * d.H, true);
  rnn_saved(op, d, hs, gates);
  op.launched(d.stamps ? ds2_rnn_fwd_stamps(&d, op.stream()) : ds2_rnn_fwd(&d, op.stream()));
}

void rnn_bwd(std::vector<int64_t> geom, int64_t nw, int64_t mt, bool persistent, at::Tensor dy, at::Tensor lens,
             OptT U_f, OptT U_b, at::Tensor hs, OptT gates, at::Tensor dgh, at::Tensor dgx, OptT carry, OptT parts,
             double dgx_scale, at::Tensor flags, at::Tensor err, int64_t timeout, OptT stamps) {
  const Op op{"rnn_bwd"};
  DS2RnnBwd d = rnn1_desc<DS2RnnBwd>(op, geom, lens, err, timeout, nw, mt, persistent, flags, stamps);
  const int64_t G = d.cell == 1 ? 3 : 1;
  d.dy = need_seq(op, dy, "dy", d, d.H);
  d.dgx = need_seq(op, dgx, "dgx", d, d.gstride);
  d.dgx_scale = (float)dgx_scale;
  rnn_U(op, d, U_f, U_b);
  rnn_saved(op, d, hs, gates);
  dir_ptrs(op, d.dgh, dgh, "dgh", at::kBFloat16, d.ndir, (int64_t)d.steps * d.NP * G * d.H);
  dir_ptrs(op, d.carry, carry, "carry", at::kFloat, d.ndir, (int64_t)d.NP * d.H);
  bias_parts(op, d.dbx_part, d.dbh_part, parts, d.cell == 1 ? 2 : 1, d.ndir, d.BG * G * d.H);
  op.launched(d.stamps ? ds2_rnn_bwd_stamps(&d, op.stream()) : ds2_rnn_bwd(&d, op.stream()));
}

// ---- XCD-local groups of R rows (csrc/rnn_xcd.hip: 32 units per census word, R <= 16;
// csrc/rnn_fp8.hip: 64 units, R <= 8)
template <typename D>
D rnnx_desc(const Op& op, const std::vector<int64_t>& g, const at::Tensor& lens, const at::Tensor& err, int64_t timeout,
            const at::Tensor& census, int units, int max_rows) {
  D d = rnn_desc<D>(op, g, lens, err, timeout);
  TORCH_CHECK(d.NP == d.BG * d.R && d.R >= 1 && d.R <= max_rows, "bad row tiling");
  d.census = op.u32(census, "census", "ndir, BG, H / units", at_least((int64_t)d.ndir * d.BG * (d.H / units)));
  return d;
}
unsigned long long* rnnx_stamps(const Op& op, const OptT& stamps, const DS2RnnX& d) {
  return stamps_ptr(op, stamps, has(stamps) ? ds2_rnnx_grid(d.H, d.cell, d.ndir * d.BG, d.xcd_map) : 0);
}

void rnnx_fwd(std::vector<int64_t> geom, at::Tensor gx, at::Tensor lens, OptT U_f, OptT U_b, OptT bh_f, OptT bh_b,
              OptT y, OptT ysum, at::Tensor hx, at::Tensor hs, OptT gates, at::Tensor census, at::Tensor err,
              int64_t timeout, OptT stamps) {
  const Op op{"rnnx_fwd"};
  DS2RnnX d = rnnx_desc<DS2RnnX>(op, geom, lens, err, timeout, census, 32, 16);
  d.gx = need_seq(op, gx, "gx", d, d.gstride);
  d.dgx_scale = 1.f;
  rnn_U(op, d, U_f, U_b);
  rnn_bh(op, d, bh_f, bh_b);
  // the fused direction sum (generations 4 - 6) is both directions' output
  if (ysum.has_value()) d.y[0] = d.y[1] = d.ysum = need_seq(op, *ysum, "ysum", d, d.H);
  else dir_ptrs(op, d.y, y, "y", at::kBFloat16, d.ndir, (int64_t)d.T * d.N * d.H);
  TORCH_CHECK(d.y[0], "rnnx_fwd needs y or ysum");
  dir_ptrs(op, d.ex, hx, "hx", at::kBFloat16, d.ndir, (int64_t)(d.steps + 1) * d.NP * d.H, true);
  rnn_saved(op, d, hs, gates);
  d.stamps = rnnx_stamps(op, stamps, d);
  op.launched(ds2_rnnx_fwd(&d, op.stream()));
}

// reduce-scatter BPTT (generation 3): dgh is a plain output (or more: the exchange of a longer
// launch), the exchange is the fp32 ring [ndir, ds2_rnnx_ring_floats or more], sentinel-filled
void rnnx_bwd(std::vector<int64_t> geom, at::Tensor dy, at::Tensor lens, OptT U_f, OptT U_b, at::Tensor hs, OptT gates,
              at::Tensor dgh, at::Tensor dgx, OptT parts, double dgx_scale, at::Tensor census, at::Tensor err,
              at::Tensor ring, int64_t timeout, OptT stamps) {
  const Op op{"rnnx_bwd"};
  DS2RnnX d = rnnx_desc<DS2RnnX>(op, geom, lens, err, timeout, census, 32, 16);
  const int64_t G = d.cell == 1 ? 3 : 1;
  d.gx = need_seq(op, dy, "dy", d, d.H);
  d.dgx = need_seq(op, dgx, "dgx", d, d.gstride);
  d.dgx_scale = (float)dgx_scale;
  rnn_U(op, d, U_f, U_b);
  rnn_saved(op, d, hs, gates);
  dir_ptrs(op, d.ex, dgh, "dgh", at::kBFloat16, d.ndir, (int64_t)d.steps * d.NP * G * d.H, true);
  dir_ptrs(op, d.ring, ring, "ring", at::kFloat, d.ndir, ds2_rnnx_ring_floats(d.H, d.BG, d.R), true);
  bias_parts(op, d.dbx_part, d.dbh_part, parts, d.cell == 1 ? 2 : 1, d.ndir, d.BG * G * d.H);
  d.stamps = rnnx_stamps(op, stamps, d);
  op.launched(ds2_rnnx_bwd_rs(&d, op.stream()));
}

// csrc/rnn_fp8.hip: GRU forward with e4m3 U8 [ndir, 3H, H] (per-tensor power-of-two scale, uexp =
// E8M0 exponent per direction on the device, int32 [ndir or more]) and an e4m3 hidden-state exchange
// hq [ndir][steps+1][NP][H] (slot 0 = e4m3 h0, slots 1.. 0xFF); saves hs / gates / bf16 hx like rnnx_fwd.
void rnnf8_fwd(std::vector<int64_t> geom, at::Tensor gx, at::Tensor lens, at::Tensor U8, at::Tensor uexp, OptT bh_f,
               OptT bh_b, at::Tensor y, at::Tensor hq, at::Tensor hx, at::Tensor hs, at::Tensor gates,
               at::Tensor census, at::Tensor err, int64_t timeout) {
  const Op op{"rnnf8_fwd"};
  DS2RnnF8 d = rnnx_desc<DS2RnnF8>(op, geom, lens, err, timeout, census, 64, 8);
  TORCH_CHECK(ds2_rnnf8_supported(d.H, d.N, d.ndir), "rnnf8: unsupported geometry");
  TORCH_CHECK(d.steps >= 1 && d.BG * d.ndir <= 8 && d.gstride >= d.ndir * 3 * d.H, "rnnf8: plan");
  const int64_t hsz = (int64_t)(d.steps + 1) * d.NP * d.H;
  d.gx = need_seq(op, gx, "gx", d, d.gstride);
  dir_ptrs(op, d.U8, U8, "U8", at::kByte, d.ndir, (int64_t)3 * d.H * d.H);
  d.uexp = op.i32(uexp, "uexp", "ndir", at_least(d.ndir));
  rnn_bh(op, d, bh_f, bh_b);
  dir_ptrs(op, d.y, y, "y", at::kBFloat16, d.ndir, (int64_t)d.T * d.N * d.H);
  dir_ptrs(op, d.hq, hq, "hq", at::kByte, d.ndir, hsz);
  dir_ptrs(op, d.hx, hx, "hx", at::kBFloat16, d.ndir, hsz);
  dir_ptrs(op, d.hsave, hs, "hs", at::kFloat, d.ndir, hsz);
  dir_ptrs(op, d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4);
  op.launched(ds2_rnnf8_fwd(&d, op.stream()));
}

// csrc/rnn_fp8.hip fp8 GRU BPTT: U8T [ndir, H, 3H] e4m3 U^T (uexp per direction), saved fp32
// h / gates of the forward, tagged-bf16 reduce-scatter ring [ndir, ring_words or more] filled 0xFF..
void rnnf8_bwd(std::vector<int64_t> geom, at::Tensor dy, at::Tensor lens, at::Tensor U8T, at::Tensor uexp,
               at::Tensor hs, at::Tensor gates, at::Tensor dgh, at::Tensor dgx, OptT parts, double dgx_scale,
               at::Tensor census, at::Tensor err, at::Tensor ring, int64_t timeout) {
  const Op op{"rnnf8_bwd"};
  DS2RnnF8B d = rnnx_desc<DS2RnnF8B>(op, geom, lens, err, timeout, census, 64, 8);
  TORCH_CHECK(ds2_rnnf8_bwd_supported(d.H, d.N, d.ndir), "rnnf8_bwd: unsupported geometry");
  TORCH_CHECK(d.steps >= 1 && d.BG * d.ndir <= 8 && d.gstride >= d.ndir * 3 * d.H, "rnnf8_bwd: plan");
  d.dy = need_seq(op, dy, "dy", d, d.H, true);
  d.dgx = need_seq(op, dgx, "dgx", d, d.gstride, true);
  d.dgx_scale = (float)dgx_scale;
  dir_ptrs(op, d.U8T, U8T, "U8T", at::kByte, d.ndir, (int64_t)3 * d.H * d.H);
  d.uexp = op.i32(uexp, "uexp", "ndir", at_least(d.ndir));
  rnn_saved(op, d, hs, gates);
  dir_ptrs(op, d.dgh, dgh, "dgh", at::kBFloat16, d.ndir, (int64_t)d.steps * d.NP * 3 * d.H);
  dir_ptrs(op, d.ring, ring, "ring", at::kInt, d.ndir, ds2_rnnf8_ring_words(d.H, d.BG, d.R), true);
  bias_parts(op, d.dbx_part, d.dbh_part, parts, 2, d.ndir, (int64_t)d.BG * 3 * d.H);
  op.launched(ds2_rnnf8_bwd(&d, op.stream()));
}

int64_t rnn_kpw(int64_t H, int64_t G, int64_t nw, bool fwd) { return ds2_rnn_kpw((int)H, (int)G, (int)nw, fwd ? 1 : 0); }

// the device words of the power-of-two quantisers: uexp / amax int32 [1 or more]
struct QuantWords {
  int* uexp;
  unsigned* amax;
};
QuantWords quant_words(const Op& op, const at::Tensor& uexp, const at::Tensor& amax) {
  return {op.i32(uexp, "uexp", "1", at_least(1)), op.u32(amax, "amax", "1", at_least(1))};
}

// e4m3 copy of a bf16 tensor scaled by ONE power of two (amax / 2^e <= 448); uexp[0] = 127 + e
void fp8_quant_pow2(at::Tensor x, at::Tensor q, at::Tensor uexp, at::Tensor amax) {
  const Op op{"fp8_quant_pow2"};
  const void* xp = op.bf16(x, "x", "n", whole(x), 16);
  void* qp = op.u8(q, "q", "n", exactly(x.numel()), 8);
  const QuantWords w = quant_words(op, uexp, amax);
  op.launched(ds2_fp8_quant_pow2(xp, x.numel(), qp, w.uexp, w.amax, op.stream()));
}

// csrc/rnn_fp8.hip: e4m3 copies of U_f (and U_b) [rows][cols] bf16 with one power-of-two scale per
// direction: q [ndir, rows, cols] and / or qt [ndir, cols, rows] uint8, uexp int32 [ndir or more],
// part fp32 [ndir * 256 or more] scratch
void fp8_quant_u(at::Tensor U_f, OptT U_b, OptT q, OptT qt, at::Tensor uexp, at::Tensor part) {
  const Op op{"fp8_quant_u"};
  const int ndir = U_b.has_value() ? 2 : 1;
  op.dims(U_f, "U", 2, "rows, cols");
  const int64_t rows = U_f.size(0), cols = U_f.size(1), n = rows * cols;
  const void* px[2] = {op.bf16(U_f, "U", "rows, cols", whole(U_f), 16), nullptr};
  px[1] = ndir == 2 ? op.bf16(*U_b, "U", "rows, cols", exactly(n), 16) : px[0];
  TORCH_CHECK(ndir == 1 || U_b->sizes() == U_f.sizes(), "fp8_quant_u: both directions' U must have one shape");
  TORCH_CHECK(rows % 64 == 0 && cols % 64 == 0, "fp8_quant_u: rows and cols multiples of 64");
  TORCH_CHECK(q.has_value() || qt.has_value(), "fp8_quant_u: q or qt");
  unsigned char* pq = static_cast<unsigned char*>(op.u8(q, "q", "ndir, rows, cols", exactly(ndir * n)));
  unsigned char* pqt = static_cast<unsigned char*>(op.u8(qt, "qt", "ndir, cols, rows", exactly(ndir * n), 16));
  void* pqd[2] = {pq, pq && ndir == 2 ? pq + n : nullptr};
  void* pqtd[2] = {pqt, pqt && ndir == 2 ? pqt + n : nullptr};
  op.launched(ds2_fp8_quant_u(ndir, px, (int)rows, (int)cols, pqd, pqtd, op.i32(uexp, "uexp", "ndir", at_least(ndir)),
                              op.f32(part, "part", "ndir * 256", at_least(ndir * 256)), op.stream()));
}

// csrc/rnn_fp8.hip: transposed e4m3 copy q [cols][rows] of a bf16 [rows][cols] tensor scaled by
// one power of two (the fp8 BPTT's U^T); uexp[0] = 127 + e
void fp8_quant_pow2_t(at::Tensor x, at::Tensor q, at::Tensor uexp, at::Tensor amax) {
  const Op op{"fp8_quant_pow2_t"};
  op.dims(x, "x", 2, "rows, cols");
  const void* xp = op.bf16(x, "x", "rows, cols", whole(x));
  void* qp = op.u8(q, "q", "cols, rows", exactly(x.numel()));
  const QuantWords w = quant_words(op, uexp, amax);
  op.launched(ds2_fp8_quant_pow2_t(xp, (int)x.size(0), (int)x.size(1), qp, w.uexp, w.amax, op.stream()));
}

// --------------------------------------------------------------------------- CTC
int64_t ctc_ws_floats(int64_t T, int64_t N, int64_t Lmax) { return ds2_ctc_ws_floats((int)T, (int)N, (int)Lmax); }

// what the CTC loss, the fused head and the alignment share: lens / label_lens int32 [N], labels int32 [N, Lmax]
struct CtcLabels {
  const int *lens, *labels, *label_lens;
  int Lmax;
};
CtcLabels ctc_labels(const Op& op, const at::Tensor& lens, const at::Tensor& labels, const at::Tensor& label_lens, int64_t N) {
  op.dims(labels, "labels", 2, "N, Lmax");
  const int64_t Lmax = labels.size(1);
  return {op.i32(lens, "lens", "N", exactly(N)), op.i32(labels, "labels", "N, Lmax", exactly(N * Lmax)),
          op.i32(label_lens, "label_lens", "N", exactly(N)), (int)Lmax};
}

// logits [T, N, K] (fp32 / bf16) -> loss fp32 [N], grad like logits; ws fp32 [ctc_ws_floats or more]
void ctc_fused(at::Tensor logits, at::Tensor lens, at::Tensor labels, at::Tensor label_lens, at::Tensor loss,
               at::Tensor grad, at::Tensor ws, int64_t blank, bool zero_inf) {
  const Op op{"ctc_fused"};
  op.dims(logits, "logits", 3, "T, N, K");
  const int T = (int)logits.size(0), N = (int)logits.size(1), K = (int)logits.size(2);
  const Act lg = op.act(logits, "logits", "T, N, K", whole(logits));
  const CtcLabels l = ctc_labels(op, lens, labels, label_lens, N);
  void* gp = op.raw(grad, "grad", logits.scalar_type(), "T, N, K", exactly(logits.numel()));
  op.launched(ds2_ctc_fused(lg.p, lg.bf16, l.lens, l.labels, l.label_lens, op.f32(loss, "loss", "N", exactly(N)), gp,
                            op.f32(ws, "ws", "ctc_ws_floats", at_least(ds2_ctc_ws_floats(T, N, l.Lmax))), T, N, K,
                            l.Lmax, (int)blank, zero_inf ? 1 : 0, op.stream()));
}

// --------------------------------------------------------------------------- CTC forced alignment
int64_t ctc_align_ws_bytes(int64_t T, int64_t N, int64_t Lmax) {
  return ds2_ctc_align_ws_bytes((int)T, (int)N, (int)Lmax);
}

// emissions [T, N, K] (fp32 / bf16) -> path [N, T] int32, tok_start / tok_end [N, Lmax] int32,
// tok_score [N, Lmax] fp32, score [N] fp32 (csrc/align.hip); ws uint8 [ctc_align_ws_bytes or more]
void ctc_align(at::Tensor em, at::Tensor lens, at::Tensor labels, at::Tensor label_lens, at::Tensor path,
               at::Tensor tok_start, at::Tensor tok_end, at::Tensor tok_score, at::Tensor score, at::Tensor ws,
               int64_t blank, bool log_probs) {
  const Op op{"ctc_align"};
  op.dims(em, "emissions", 3, "T, N, K");
  const int T = (int)em.size(0), N = (int)em.size(1), K = (int)em.size(2);
  const Act e = op.act(em, "emissions", "T, N, K", whole(em));
  const CtcLabels l = ctc_labels(op, lens, labels, label_lens, N);
  const int64_t NL = (int64_t)N * l.Lmax;
  TORCH_CHECK(K <= 32, "ctc_align: K <= 32 classes");
  TORCH_CHECK(l.Lmax >= 1 && 2 * (int64_t)l.Lmax + 1 <= 2048, "ctc_align: 1 <= Lmax and 2*Lmax+1 <= 2048 lattice states");
  TORCH_CHECK(blank >= 0 && blank < K, "ctc_align: 0 <= blank < K");
  op.launched(ds2_ctc_align(e.p, e.bf16, log_probs ? 1 : 0, l.lens, l.labels, l.label_lens,
                            op.i32(path, "path", "N, T", exactly((int64_t)N * T)),
                            op.i32(tok_start, "tok_start", "N, Lmax", exactly(NL)),
                            op.i32(tok_end, "tok_end", "N, Lmax", exactly(NL)),
                            op.f32(tok_score, "tok_score", "N, Lmax", exactly(NL)), op.f32(score, "score", "N", exactly(N)),
                            op.u8(ws, "ws", "ctc_align_ws_bytes", at_least(ds2_ctc_align_ws_bytes(T, N, l.Lmax)), 16), T, N,
                            K, l.Lmax, (int)blank, op.stream()));
}

// --------------------------------------------------------------------------- BN
int64_t bn_chunks(int64_t N, int64_t T, int64_t F) { return ds2_bn_chunks((int)N, (int)T, (int)F); }

// y [N, C, T, F] (fp32 / bf16); the per-channel vectors are fp32 [C]; part is fp32 [C, nb, 2] with
// nb = bn_chunks(N, T, F), the grid of the reduce pass
struct BnDims {
  int N, C, T, F, nb;
  Act y;
};
BnDims bn_dims(const Op& op, const at::Tensor& y) {
  op.dims(y, "y", 4, "N, C, T, F");
  const int N = (int)y.size(0), C = (int)y.size(1), T = (int)y.size(2), F = (int)y.size(3);
  return {N, C, T, F, ds2_bn_chunks(N, T, F), op.act(y, "y", "N, C, T, F", whole(y))};
}
float* bn_vec(const Op& op, const OptT& t, const char* name, int C) { return op.f32(t, name, "C", exactly(C)); }
float* bn_part(const Op& op, const at::Tensor& part, const BnDims& d) {
  return op.f32(part, "part", "C, bn_chunks(N, T, F), 2", exactly(2 * (int64_t)d.C * d.nb));
}

void bn_stats(at::Tensor y, at::Tensor part, double eps, at::Tensor mean, at::Tensor invstd, OptT run_mean,
              OptT run_var, double momentum) {
  const Op op{"bn_stats"};
  const BnDims d = bn_dims(op, y);
  TORCH_CHECK(has(run_mean) == has(run_var), "bn_stats: run_mean and run_var go together");
  op.launched(ds2_bn_stats(d.y.p, d.y.bf16, d.N, d.C, d.T, d.F, bn_part(op, part, d), d.nb, (float)eps,
                           bn_vec(op, mean, "mean", d.C), bn_vec(op, invstd, "invstd", d.C),
                           bn_vec(op, run_mean, "run_mean", d.C), bn_vec(op, run_var, "run_var", d.C), (float)momentum,
                           op.stream()));
}

void bn_apply(at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta, at::Tensor out,
              int64_t layout) {
  const Op op{"bn_apply"};
  const BnDims d = bn_dims(op, y);
  const Act o = op.act(out, "out", "N, C, T, F", exactly(y.numel()));
  op.launched(ds2_bn_apply(d.y.p, d.y.bf16, bn_vec(op, mean, "mean", d.C), bn_vec(op, invstd, "invstd", d.C),
                           bn_vec(op, gamma, "gamma", d.C), bn_vec(op, beta, "beta", d.C), o.p, o.bf16, d.N, d.C, d.T,
                           d.F, (int)layout, op.stream()));
}

void bn_bwd(at::Tensor dout, at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta,
            at::Tensor part, at::Tensor dgamma, at::Tensor dbeta, at::Tensor dy, int64_t layout) {
  const Op op{"bn_bwd"};
  const BnDims d = bn_dims(op, y);
  const Act go = op.act(dout, "dout", "N, C, T, F", exactly(y.numel())), gy = op.act(dy, "dy", "N, C, T, F", exactly(y.numel()));
  op.launched(ds2_bn_bwd(go.p, go.bf16, d.y.p, d.y.bf16, bn_vec(op, mean, "mean", d.C), bn_vec(op, invstd, "invstd", d.C),
                         bn_vec(op, gamma, "gamma", d.C), bn_vec(op, beta, "beta", d.C), bn_part(op, part, d), d.nb,
                         bn_vec(op, dgamma, "dgamma", d.C), bn_vec(op, dbeta, "dbeta", d.C), gy.p, gy.bf16, d.N, d.C,
                         d.T, d.F, (int)layout, op.stream()));
}

// --------------------------------------------------------------------------- optimizer
// What the Adam + EMA kernels assume of their arrays (csrc/optim.hip: f32x4 accesses of the fp32
// arrays, uint2 stores of the bf16 copy): n elements each, fp32 16-B and bf16 8-B aligned; hyper
// fp32 {lr_t, ema_keep} [2 or more]
struct AdamArrays {
  long long n;
  float *p, *g, *m, *v, *ema;
  void* p16;
  const float *hyper, *clip;
};
// The clipping state the CLIP kernels read (csrc/optim.hip): fp32 [ds2_clip_state_words() or more]
float* clip_state(const Op& op, const OptT& clip, const char* name) {
  return op.f32(clip, name, "clip_state_words", at_least(ds2_clip_state_words()), 4);
}
AdamArrays adam_arrays(const Op& op, const at::Tensor& p, const at::Tensor& g, const at::Tensor& m, const at::Tensor& v,
                       const OptT& ema, const OptT& p16, const OptT& hyper, const OptT& clip) {
  const Count n = whole(p);
  return {n.n, op.f32(p, "p", "n", n, 16), op.f32(g, "g", "n", n, 16), op.f32(m, "m", "n", n, 16), op.f32(v, "v", "n", n, 16),
          op.f32(ema, "ema", "n", n, 16), op.bf16(p16, "p16", "n", n, 8), op.f32(hyper, "hyper", "2", at_least(2)),
          clip_state(op, clip, "clip")};
}

void adam_ema(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, OptT ema, OptT p16, double lr_t, double b1,
              double b2, double eps, double gscale, double ema_keep, OptT skip, int64_t max_grid, OptT hyper,
              int64_t lds_reserve, OptT clip) {
  const Op op{"adam_ema"};
  TORCH_CHECK(lds_reserve >= 0 && lds_reserve <= 65536, "adam_ema: lds_reserve in [0, 64 KB]");
  const AdamArrays a = adam_arrays(op, p, g, m, v, ema, p16, hyper, clip);
  op.launched(ds2_adam_ema(a.p, a.g, a.m, a.v, a.ema, a.p16, a.n, (float)lr_t, (float)b1, (float)b2, (float)eps,
                           (float)gscale, (float)ema_keep, op.i32(skip, "skip", "1", at_least(1)), (int)max_grid, a.hyper,
                           (int)lds_reserve, a.clip, op.stream()));
}

// Adam + EMA over several (lo, hi) element ranges of whole-arena buffers in one launch
void adam_ema_ranges(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, OptT ema, OptT p16,
                     std::vector<int64_t> lohi, double lr_t, double b1, double b2, double eps, double gscale,
                     double ema_keep, OptT hyper, OptT clip) {
  const Op op{"adam_ema_ranges"};
  const AdamArrays a = adam_arrays(op, p, g, m, v, ema, p16, hyper, clip);
  TORCH_CHECK(lohi.size() % 2 == 0, "adam_ema_ranges: (lo, hi) pairs");
  for (size_t i = 0; i < lohi.size(); ++i) TORCH_CHECK(lohi[i] >= 0 && lohi[i] <= a.n, "adam_ema_ranges: range");
  // two ranges sharing an element would be updated by two threads at once
  std::vector<std::pair<int64_t, int64_t>> sorted;
  for (size_t i = 0; i + 1 < lohi.size(); i += 2)
    if (lohi[i + 1] > lohi[i]) sorted.emplace_back(lohi[i], lohi[i + 1]);
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 1; i < sorted.size(); ++i)
    TORCH_CHECK(sorted[i].first >= sorted[i - 1].second, "adam_ema_ranges: ranges overlap");
  std::vector<long long> r(lohi.begin(), lohi.end());
  op.launched(ds2_adam_ema_ranges(a.p, a.g, a.m, a.v, a.ema, a.p16, r.data(), (int)(r.size() / 2), (float)lr_t, (float)b1,
                                  (float)b2, (float)eps, (float)gscale, (float)ema_keep, a.hyper, a.clip, op.stream()));
}

int64_t grad_norm_blocks(int64_t n) { return ds2_grad_norm_blocks(n); }

// part fp32 [1 or more]: as many block partials as it has elements
void grad_norm(at::Tensor g, double gscale, at::Tensor part, at::Tensor bad) {
  const Op op{"grad_norm"};
  op.launched(ds2_grad_norm(op.f32(g, "g", "n", whole(g)), g.numel(), (float)gscale, op.f32(part, "part", "blocks", at_least(1)),
                            (int)part.numel(), op.i32(bad, "bad", "1", exactly(1)), op.stream()));
}

int64_t grad_sumsq_segment() { return ds2_grad_sumsq_segment(); }

// part[ceil(n / segment)] = fixed-order partial sums of (fl32(g gscale))^2, one per segment of g.
// nontemporal (the default, as measured: profiles/clip.md) only changes the load instruction, never a partial.
void grad_sumsq(at::Tensor g, double gscale, at::Tensor part, int64_t max_grid, bool nontemporal) {
  const Op op{"grad_sumsq"};
  const int64_t seg = ds2_grad_sumsq_segment();
  TORCH_CHECK(max_grid >= 0 && max_grid <= 65535, "grad_sumsq: max_grid in [0, 65535]");
  op.launched(ds2_grad_sumsq(op.f32(g, "g", "n", whole(g), 16), g.numel(), (float)gscale,
                             op.f32(part, "part", "ceil(n / segment)", exactly((g.numel() + seg - 1) / seg)), (int)max_grid,
                             nontemporal ? 1 : 0, op.stream()));
}

// state = {S, norm, coef | bad, steps, clipped_steps, skipped_steps, spare} from the partials and max_norm
void clip_finalize(at::Tensor part, double max_norm, at::Tensor state) {
  const Op op{"clip_finalize"};
  TORCH_CHECK(max_norm > 0, "clip_finalize: max_norm must be > 0 (inf: measure only)");
  op.launched(ds2_clip_finalize(op.f32(part, "part", "segments", whole(part)), part.numel(), (float)max_norm,
                                clip_state(op, state, "state"), op.stream()));
}

void cast_bf16(at::Tensor x, at::Tensor y) {
  const Op op{"cast_bf16"};
  op.launched(ds2_cast_bf16(op.f32(x, "x", "n", whole(x)), op.bf16(y, "y", "n", exactly(x.numel())), x.numel(), op.stream()));
}

// --------------------------------------------------------------------------- conv front-end
// Activations are channels-last bf16 [N, T, F, 32] (conv1's input: [N, T, F0]); conv1's BatchNorm
// vectors are fp32 [32]; part buffers are fp32 workspaces of the stated size or more.
struct Nhwc {
  const void* p;
  int N, T, F;
};
Nhwc conv_act(const Op& op, const at::Tensor& t, const char* name, int64_t N = -1) {
  op.dims(t, name, 4, "N, T, F, 32");
  TORCH_CHECK(t.size(3) == 32 && (N < 0 || t.size(0) == N), op.op, ": ", name, " must be bf16 [N, T, F, 32] of batch ", N,
              ", got ", t.sizes());
  return {op.bf16(t, name, "N, T, F, 32", whole(t)), (int)t.size(0), (int)t.size(1), (int)t.size(2)};
}
Nhwc conv_input(const Op& op, const at::Tensor& t, const char* name) {
  op.dims(t, name, 3, "N, T, F0");
  return {op.bf16(t, name, "N, T, F0", whole(t)), (int)t.size(0), (int)t.size(1), (int)t.size(2)};
}
float* vec32(const Op& op, const OptT& t, const char* name) { return op.f32(t, name, "32", exactly(32)); }
float* conv_part(const Op& op, const OptT& t, int64_t n) { return op.f32(t, "part", "workspace", at_least(n)); }
// per-tile phase stamps of workgroups 0..7 (optional int64 [8 * 16 * 6 or more], tools/conv_timeline.py)
long long* trace_ptr(const Op& op, const OptT& trace) { return op.i64(trace, "trace", "8, 16, 6", at_least(8 * 16 * 6)); }

// x [N,T,F0] bf16, w [32,1,20,5] bf16 -> y [N,T1,F1,32] bf16, part [grid, 64] f32
void conv1_fwd(at::Tensor x, at::Tensor w, OptT bias, at::Tensor y, at::Tensor part) {
  const Op op{"conv1_fwd"};
  const Nhwc X = conv_input(op, x, "x"), Y = conv_act(op, y, "y", X.N);
  conv_launched(op, ds2_conv1_fwd(X.p, op.bf16(w, "w", "32, 1, 20, 5", exactly(32 * 100)), vec32(op, bias, "bias"), (void*)Y.p,
                                  conv_part(op, part, (int64_t)ds2_conv1_fwd_grid(X.N, Y.T) * 64), X.N, X.T, X.F, Y.T, Y.F,
                                  op.stream()));
}
int64_t conv1_fwd_grid(int64_t N, int64_t T1) { return ds2_conv1_fwd_grid((int)N, (int)T1); }

const void* conv2_w(const Op& op, const at::Tensor& w) { return op.bf16(w, "w", "32, 32, 10, 5", exactly(32 * 32 * 50)); }

// x [N,T1,F1,32], w [32,32,10,5] -> y [N,T2,F2,32], part [grid, 64]
void conv2_fwd(at::Tensor x, at::Tensor w, OptT bias, at::Tensor y, at::Tensor part, int64_t grid, OptT trace) {
  const Op op{"conv2_fwd"};
  TORCH_CHECK(grid > 0, "grid");
  const Nhwc X = conv_act(op, x, "x"), Y = conv_act(op, y, "y", X.N);
  conv_launched(op, ds2_conv2_fwd(X.p, conv2_w(op, w), vec32(op, bias, "bias"), (void*)Y.p, conv_part(op, part, grid * 64),
                                  (int)grid, X.N, X.T, X.F, Y.T, Y.F, trace_ptr(op, trace), op.stream()));
}

// dy [N,T2,F2,32], w [32,32,10,5] -> dx [N,T1,F1,32]
// bn (optional, all or none): y1 = conv1's output (dx's shape), conv1's BN mean / invstd / gamma
// / beta, and part [grid * 64] fp32 that receives per-workgroup BN-backward sums over dx
void conv2_dgrad(at::Tensor dy, at::Tensor w, at::Tensor dx, int64_t grid, OptT y1, OptT mean, OptT invstd,
                 OptT gamma, OptT beta, OptT part, OptT trace) {
  const Op op{"conv2_dgrad"};
  TORCH_CHECK(grid > 0, "grid");
  const Nhwc DX = conv_act(op, dx, "dx"), DY = conv_act(op, dy, "dy", DX.N);
  DS2Conv2DgradBn bn{};
  const bool with_bn = y1.has_value();
  if (with_bn) {
    TORCH_CHECK(mean && invstd && gamma && beta && part, "conv2_dgrad: the BN arguments come all or none");
    TORCH_CHECK(y1->sizes() == dx.sizes(), "conv2_dgrad: y1 must have dx's shape");
    bn = DS2Conv2DgradBn{conv_act(op, *y1, "y1").p, vec32(op, mean, "mean"), vec32(op, invstd, "invstd"),
                         vec32(op, gamma, "gamma"), vec32(op, beta, "beta"), conv_part(op, part, grid * 64)};
  }
  conv_launched(op, ds2_conv2_dgrad(DY.p, conv2_w(op, w), (void*)DX.p, (int)grid, DX.N, DX.T, DX.F, DY.T, DY.F,
                                    with_bn ? &bn : nullptr, trace_ptr(op, trace), op.stream()));
}

// dy [N,T2,F2,32], x [N,T1,F1,32] -> dw (fp32, 32*32*10*5), part scratch
void conv2_wgrad(at::Tensor dy, at::Tensor x, at::Tensor part, at::Tensor dw, int64_t grid) {
  const Op op{"conv2_wgrad"};
  TORCH_CHECK(grid > 0, "grid");
  const Nhwc X = conv_act(op, x, "x"), DY = conv_act(op, dy, "dy", X.N);
  conv_launched(op, ds2_conv2_wgrad(DY.p, X.p, conv_part(op, part, ds2_conv2_wgrad_part_floats((int)grid)), (int)grid,
                                    op.f32(dw, "dw", "32, 32, 10, 5", exactly(32 * 32 * 50)), X.N, X.T, X.F, DY.T, DY.F,
                                    op.stream()));
}

// dy [N,T1,F1,32], x [N,T,F0] -> dw (fp32, 32*20*5)
// bn (optional, all or none): dy is then dz = dL/d(clip(BN(y1))) and the kernel applies conv1's
// BatchNorm backward (batch statistics mean / invstd, affine gamma / beta, dbeta / dgamma sums)
// while staging it, bitwise as bn_cl_bwd's apply pass
void conv1_wgrad(at::Tensor dy, at::Tensor x, at::Tensor part, at::Tensor dw, int64_t grid, OptT y1, OptT mean,
                 OptT invstd, OptT gamma, OptT beta, OptT dbeta, OptT dgamma) {
  const Op op{"conv1_wgrad"};
  TORCH_CHECK(grid > 0, "grid");
  const Nhwc X = conv_input(op, x, "x"), DY = conv_act(op, dy, "dy", X.N);
  DS2Conv1WgradBn bn{};
  const bool with_bn = y1.has_value();
  if (with_bn) {
    TORCH_CHECK(mean && invstd && gamma && beta && dbeta && dgamma, "conv1_wgrad: the BN arguments come all or none");
    TORCH_CHECK(y1->sizes() == dy.sizes(), "conv1_wgrad: y1 must have dz's shape");
    bn = DS2Conv1WgradBn{DY.p, conv_act(op, *y1, "y1").p, vec32(op, mean, "mean"), vec32(op, invstd, "invstd"),
                         vec32(op, gamma, "gamma"), vec32(op, beta, "beta"), vec32(op, dbeta, "dbeta"),
                         vec32(op, dgamma, "dgamma")};
  }
  conv_launched(op, ds2_conv1_wgrad(with_bn ? nullptr : DY.p, X.p, conv_part(op, part, ds2_conv1_wgrad_part_floats((int)grid)),
                                    (int)grid, op.f32(dw, "dw", "32, 1, 20, 5", exactly(32 * 100)), X.N, X.T, X.F, DY.T, DY.F,
                                    with_bn ? &bn : nullptr, op.stream()));
}
int64_t conv2_wgrad_part_floats(int64_t grid) { return ds2_conv2_wgrad_part_floats((int)grid); }
int64_t conv1_wgrad_part_floats(int64_t grid) { return ds2_conv1_wgrad_part_floats((int)grid); }

void bn_cl_finalize(at::Tensor part, int64_t nb, double M, double eps, at::Tensor mean, at::Tensor invstd,
                    OptT run_mean, OptT run_var, double momentum) {
  const Op op{"bn_cl_finalize"};
  conv_launched(op, ds2_bn_cl_finalize(conv_part(op, part, nb * 64), (int)nb, M, (float)eps, vec32(op, mean, "mean"),
                                       vec32(op, invstd, "invstd"), vec32(op, run_mean, "run_mean"),
                                       vec32(op, run_var, "run_var"), (float)momentum, op.stream()));
}

// y [N,T,F,32] -> out [N,T,F,32] (tmaj=0) or [T,N,32*F] (tmaj=1)
void bn_cl_apply(at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta, at::Tensor out,
                 bool tmaj) {
  const Op op{"bn_cl_apply"};
  const Nhwc Y = conv_act(op, y, "y");
  conv_launched(op, ds2_bn_cl_apply(Y.p, vec32(op, mean, "mean"), vec32(op, invstd, "invstd"), vec32(op, gamma, "gamma"),
                                    vec32(op, beta, "beta"), op.bf16(out, "out", "N, T, F, 32", exactly(y.numel())), Y.N, Y.T,
                                    Y.F, tmaj ? 1 : 0, op.stream()));
}

// part_ready: part already holds nb partial sums (conv2_dgrad's bn epilogue), skip the reduce pass;
// 2: also skip the apply pass (dgamma / dbeta only: conv1_wgrad applies the backward itself)
void bn_cl_bwd(at::Tensor dz, at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta,
               at::Tensor part, int64_t nb, at::Tensor dgamma, at::Tensor dbeta, at::Tensor dy, bool tmaj,
               int64_t part_ready) {
  const Op op{"bn_cl_bwd"};
  const Nhwc Y = conv_act(op, y, "y");
  const Count n = whole(y);
  conv_launched(op, ds2_bn_cl_bwd(op.bf16(dz, "dz", "N, T, F, 32", n), Y.p, vec32(op, mean, "mean"), vec32(op, invstd, "invstd"),
                                  vec32(op, gamma, "gamma"), vec32(op, beta, "beta"), conv_part(op, part, nb * 64), (int)nb,
                                  vec32(op, dgamma, "dgamma"), vec32(op, dbeta, "dbeta"), op.bf16(dy, "dy", "N, T, F, 32", n),
                                  Y.N, Y.T, Y.F, tmaj ? 1 : 0, (int)part_ready, op.stream()));
}

// --------------------------------------------------------------------------- greedy CTC decode
// logits [T, N, K] (fp32/bf16, time-major) -> labels int32 [N, T or more] (first counts[n] valid),
// counts [N] int32, optional score [N] fp32 (greedy path log-probability)
void ctc_greedy(at::Tensor logits, at::Tensor lens, at::Tensor labels, at::Tensor counts, int64_t blank,
                OptT score) {
  const Op op{"ctc_greedy"};
  op.dims(logits, "logits", 3, "T, N, K");
  const int T = (int)logits.size(0), N = (int)logits.size(1), K = (int)logits.size(2);
  const Act lg = op.act(logits, "logits", "T, N, K", whole(logits));
  op.launched(ds2_ctc_greedy(lg.p, lg.bf16, op.i32(lens, "lens", "N", exactly(N)), T, N, K, (int)blank,
                             op.i32(labels, "labels", "N, T", at_least((int64_t)N * T)),
                             op.i32(counts, "counts", "N", exactly(N)), op.f32(score, "score", "N", exactly(N)), op.stream()));
}

// --------------------------------------------------------------------------- copies and fills (csrc/fill.hip)
// out [C, R] = in [R, C]^T (bf16, unit-stride rows; rows may be pitched: the kernel takes both row strides)
void transpose_bf16(at::Tensor in, at::Tensor out) {
  const Op op{"transpose_bf16"};
  const Pitched i = op.pitched(in, "in", at::kBFloat16, 0, 1, false), o = op.pitched(out, "out", at::kBFloat16, 0, 1, false);
  TORCH_CHECK(out.size(0) == in.size(1) && out.size(1) == in.size(0), "transpose_bf16: out must be [C, R]");
  op.launched(ds2_transpose_bf16(i.p, o.p, (int)in.size(0), (int)in.size(1), (int)i.ld, (int)o.ld, op.stream()));
}

// dst_i[r, :] = src_i[r, :] then zeros to dst_i's row end, for 2-D (or 1-D: one row) tensors of
// one dtype with unit-stride rows and src cols <= dst cols; plus ns <= 4 fp32 scalars into
// sdst (fp32 [ns or more]). ONE launch (csrc/fill.hip multi_copy_kernel).
void multi_copy(std::vector<at::Tensor> dsts, std::vector<at::Tensor> srcs, c10::optional<at::Tensor> sdst,
                std::vector<double> svals) {
  const Op op{"multi_copy"};
  TORCH_CHECK(dsts.size() == srcs.size() && dsts.size() <= 8 && svals.size() <= 4, "multi_copy: <= 8 pairs, <= 4 scalars");
  void* dp[8];
  const void* sp[8];
  unsigned long long rows[8];
  unsigned srow[8], drow[8], spitch[8], dpitch[8];
  for (size_t i = 0; i < dsts.size(); ++i) {
    const at::Tensor &d = dsts[i], &s = srcs[i];
    const at::ScalarType dt = d.scalar_type();
    const int64_t es = d.element_size();
    TORCH_CHECK(d.dim() == s.dim(), "multi_copy: a pair is 1-D or 2-D alike");
    if (d.dim() == 1) {   // 1-D pairs are contiguous
      TORCH_CHECK(s.numel() <= d.numel(), "multi_copy: src longer than dst");
      dp[i] = op.raw(d, "dst", dt, "n", whole(d));
      sp[i] = op.raw(s, "src", dt, "<= n", whole(s));
      rows[i] = 1;
      srow[i] = (unsigned)(s.numel() * es); drow[i] = (unsigned)(d.numel() * es);
      spitch[i] = srow[i]; dpitch[i] = drow[i];
    } else {              // 2-D pairs may be pitched views
      const Pitched D = op.pitched(d, "dst", dt, 0, 1, false), S = op.pitched(s, "src", dt, 0, 1, false);
      TORCH_CHECK(d.size(0) == s.size(0) && s.size(1) <= d.size(1), "multi_copy: rows match, src cols <= dst cols");
      TORCH_CHECK((d.size(0) <= 1 || D.ld >= d.size(1)) && (s.size(0) <= 1 || S.ld >= s.size(1)),
                  "multi_copy: rows must not overlap");
      dp[i] = D.p; sp[i] = S.p;
      rows[i] = (unsigned long long)d.size(0);
      srow[i] = (unsigned)(s.size(1) * es); drow[i] = (unsigned)(d.size(1) * es);
      spitch[i] = (unsigned)(std::max<int64_t>(S.ld, s.size(1)) * es);
      dpitch[i] = (unsigned)(std::max<int64_t>(D.ld, d.size(1)) * es);
    }
  }
  float sv[4] = {0.f, 0.f, 0.f, 0.f};
  for (size_t i = 0; i < svals.size(); ++i) sv[i] = (float)svals[i];
  op.launched(ds2_multi_copy((int)dsts.size(), dp, sp, rows, srow, drow, spitch, dpitch,
                             op.f32(sdst, "sdst", "ns", at_least((int64_t)svals.size())), sv, (int)svals.size(), op.stream()));
}

// feats fp32 -> bf16 (same size) and rnn lengths floor((seq_lens - 34) / 4), int32
void prep_inputs(at::Tensor x, at::Tensor y, at::Tensor lens_in, at::Tensor lens_out) {
  const Op op{"prep_inputs"};
  op.launched(ds2_prep_inputs(op.f32(x, "feats", "n", whole(x)), op.bf16(y, "feats bf16", "n", exactly(x.numel())), x.numel(),
                              op.i32(lens_in, "seq_lens", "B", whole(lens_in)),
                              op.i32(lens_out, "rnn lens", "B", exactly(lens_in.numel())), (int)lens_in.numel(), op.stream()));
}

// a wave on the current stream that waits (bounded by `timeout` s_memrealtime ticks) until census
// word `word` (int32, one element) is no longer -1: the persistent launch owning it is resident
void wait_resident(at::Tensor word, int64_t timeout) {
  const Op op{"wait_resident"};
  op.launched(ds2_wait_resident(op.u32(word, "census word", "1", exactly(1)), (long long)timeout, op.stream()));
}

// fill each (contiguous tensor of any dtype, 32-bit pattern) region in ONE launch (<= 8 regions)
void multi_fill(std::vector<at::Tensor> ts, std::vector<int64_t> patterns) {
  const Op op{"multi_fill"};
  TORCH_CHECK(ts.size() == patterns.size() && ts.size() <= 8, "multi_fill: <= 8 (tensor, pattern) pairs");
  void* ptrs[8];
  unsigned long long bytes[8];
  unsigned pats[8];
  for (size_t i = 0; i < ts.size(); ++i) {
    ptrs[i] = op.raw(ts[i], "region", kAnyDtype, "n", whole(ts[i]));
    bytes[i] = (unsigned long long)ts[i].numel() * ts[i].element_size();
    pats[i] = (unsigned)(uint32_t)patterns[i];
  }
  op.launched(ds2_multi_fill((int)ts.size(), ptrs, bytes, pats, op.stream()));
}

// out_j (= or +=) sum over axis 1 of in_j [R, B, C] (fp32, contiguous) into out_j [R * C]
// (fp32, contiguous): up to 4 slabs in one launch (csrc/reduce.hip, recurrent bias gradients)
void col_sum(std::vector<at::Tensor> ins, std::vector<at::Tensor> outs, std::vector<bool> acc) {
  const Op op{"col_sum"};
  TORCH_CHECK(!ins.empty() && ins.size() <= 4 && ins.size() == outs.size() && ins.size() == acc.size(),
              "col_sum: 1..4 (in, out, accumulate) triples");
  const float* ip[4];
  float* out[4];
  int R[4], B[4], C[4], a[4];
  for (size_t j = 0; j < ins.size(); ++j) {
    op.dims(ins[j], "in", 3, "R, B, C");
    ip[j] = op.f32(ins[j], "in", "R, B, C", whole(ins[j]));
    out[j] = op.f32(outs[j], "out", "R * C", exactly(ins[j].size(0) * ins[j].size(2)));
    R[j] = (int)ins[j].size(0);
    B[j] = (int)ins[j].size(1);
    C[j] = (int)ins[j].size(2);
    a[j] = acc[j] ? 1 : 0;
  }
  op.launched(ds2_col_sum((int)ins.size(), ip, out, R, B, C, a, op.stream()));
}

// --------------------------------------------------------------------------- CTC prefix beam search (csrc/beam.hip)
// The device-resident beams of B streams: node / last / parent int32 and pb / pnb fp32 [B, W]
// (1 <= W <= 32), nbeam / nnodes int32 [B], nodes int32 [B, cap, 2]
struct BeamState {
  int B, W, cap;
  int *node, *last, *parent, *nbeam, *nodes, *nnodes;
  float *pb, *pnb;
};
BeamState beam_state(const Op& op, const at::Tensor& node, const at::Tensor& last, const at::Tensor& parent,
                     const at::Tensor& pb, const at::Tensor& pnb, const at::Tensor& nbeam, const at::Tensor& nodes,
                     const at::Tensor& nnodes) {
  op.dims(node, "node", 2, "B, W");
  op.dims(nodes, "nodes", 3, "B, cap, 2");
  const int64_t B = node.size(0), W = node.size(1);
  TORCH_CHECK(W >= 1 && W <= 32 && nodes.size(0) == B && nodes.size(2) == 2, op.op,
              ": [B, W] beams with 1 <= W <= 32, nodes [B, cap, 2]");
  const Count bw = exactly(B * W), b = exactly(B);
  return {(int)B, (int)W, (int)nodes.size(1), op.i32(node, "node", "B, W", bw), op.i32(last, "last", "B, W", bw),
          op.i32(parent, "parent", "B, W", bw), op.i32(nbeam, "nbeam", "B", b), op.i32(nodes, "nodes", "B, cap, 2", whole(nodes)),
          op.i32(nnodes, "nnodes", "B", b), op.f32(pb, "pb", "B, W", bw), op.f32(pnb, "pnb", "B, W", bw)};
}

// LM shallow fusion (deepspeech_amd/lm.py): lm [S, K, 2] int32 (w fp32 bits, next state) and
// lmstate [B, W] int32 beside the beam state
struct BeamLm {
  const int* lm = nullptr;
  int S = 0, K = 0;
  int* lmstate = nullptr;
};
BeamLm beam_lm(const Op& op, const at::Tensor& lm, const at::Tensor& lmstate, const BeamState& s) {
  op.dims(lm, "lm", 3, "S, K, 2");
  TORCH_CHECK(lm.size(2) == 2 && lm.size(0) >= 1 && lm.size(0) * lm.size(1) < (1ll << 31), op.op,
              ": lm must be int32 [S, K, 2], S * K < 2^31");
  return {op.i32(lm, "lm", "S, K, 2", whole(lm)), (int)lm.size(0), (int)lm.size(1),
          op.i32(lmstate, "lmstate", "B, W", exactly((int64_t)s.B * s.W))};
}

// advance the beams by the frames of lp [T, B, K] (fp32 log-probs; frames [B] int32 per-stream frame
// counts, or all T); key [B, W, 2] int64: the hypotheses' prefix fingerprints (zero at reset); with
// an LM pair, fused with its weights
void ctc_beam_any(const Op& op, const at::Tensor& lp, const OptT& frames, int64_t blank, double prune, const BeamState& s,
                  const at::Tensor& err, const at::Tensor& key, const at::Tensor* lm, const at::Tensor* lmstate) {
  op.dims(lp, "lp", 3, "T, B, K");
  const int T = (int)lp.size(0), K = (int)lp.size(2);
  TORCH_CHECK(lp.size(1) == s.B && K >= 2 && K <= 64 && blank >= 0 && blank < K, op.op,
              ": lp [T, B, K] over the beams' B streams, 2 <= K <= 64, 0 <= blank < K");
  const float* lpp = op.f32(lp, "lp", "T, B, K", whole(lp));
  const int* fr = op.lens(frames, "frames", s.B);
  unsigned* e = op.u32(err, "err", "1", at_least(1));
  auto* k = reinterpret_cast<unsigned long long*>(op.i64(key, "key", "B, W, 2", exactly((int64_t)s.B * s.W * 2)));
  if (!lm) {
    op.launched(ds2_ctc_beam(lpp, fr, T, s.B, K, s.W, (int)blank, (float)prune, s.node, s.last, s.parent, s.pb, s.pnb, s.nbeam,
                             s.nodes, s.nnodes, s.cap, e, k, op.stream()));
    return;
  }
  const BeamLm l = beam_lm(op, *lm, *lmstate, s);
  TORCH_CHECK(l.K == K, op.op, ": lm must be int32 [S, K, 2] over lp's K classes");
  op.launched(ds2_ctc_beam_lm(lpp, fr, T, s.B, K, s.W, (int)blank, (float)prune, s.node, s.last, s.parent, s.pb, s.pnb, s.nbeam,
                              s.nodes, s.nnodes, s.cap, e, l.lm, l.S, l.lmstate, k, op.stream()));
}
void ctc_beam(at::Tensor lp, OptT frames, int64_t blank, double prune, at::Tensor node, at::Tensor last,
              at::Tensor parent, at::Tensor pb, at::Tensor pnb, at::Tensor nbeam, at::Tensor nodes,
              at::Tensor nnodes, at::Tensor err, at::Tensor key) {
  const Op op{"ctc_beam"};
  ctc_beam_any(op, lp, frames, blank, prune, beam_state(op, node, last, parent, pb, pnb, nbeam, nodes, nnodes), err, key,
               nullptr, nullptr);
}
void ctc_beam_lm(at::Tensor lp, OptT frames, int64_t blank, double prune, at::Tensor node, at::Tensor last,
                 at::Tensor parent, at::Tensor pb, at::Tensor pnb, at::Tensor nbeam, at::Tensor nodes,
                 at::Tensor nnodes, at::Tensor err, at::Tensor lm, at::Tensor lmstate, at::Tensor key) {
  const Op op{"ctc_beam_lm"};
  ctc_beam_any(op, lp, frames, blank, prune, beam_state(op, node, last, parent, pb, pnb, nbeam, nodes, nnodes), err, key,
               &lm, &lmstate);
}

// labels [B, W, Lcap] (back-aligned prefix walk: the first out_len entries), out_len [B, W] (-1:
// no hypothesis), score [B, W] of the device beams; with an LM pair, the </s> weight of each
// hypothesis' LM state is added to its score
void ctc_backtrack_any(const Op& op, const BeamState& s, const at::Tensor& out, const at::Tensor& out_len,
                       const at::Tensor& score, const at::Tensor* lm, const at::Tensor* lmstate, int64_t blank) {
  op.dims(out, "out", 3, "B, W, L");
  TORCH_CHECK(out.size(0) == s.B && out.size(1) == s.W, op.op, ": out must be int32 [B, W, L], got ", out.sizes());
  const Count bw = exactly((int64_t)s.B * s.W);
  int* o = op.i32(out, "out", "B, W, L", whole(out));
  int* ol = op.i32(out_len, "out_len", "B, W", bw);
  float* sc = op.f32(score, "score", "B, W", bw);
  if (!lm) {
    op.launched(ds2_ctc_beam_backtrack(s.nodes, s.cap, s.node, s.nbeam, s.pb, s.pnb, s.B, s.W, o, ol, sc, (int)out.size(2),
                                       op.stream()));
    return;
  }
  const BeamLm l = beam_lm(op, *lm, *lmstate, s);
  TORCH_CHECK(blank >= 0 && blank < l.K, op.op, ": 0 <= blank < K");
  op.launched(ds2_ctc_beam_backtrack_lm(s.nodes, s.cap, s.node, s.nbeam, s.pb, s.pnb, s.B, s.W, o, ol, sc, (int)out.size(2),
                                        l.lm, l.S, l.K, (int)blank, l.lmstate, op.stream()));
}
void ctc_beam_backtrack(at::Tensor node, at::Tensor last, at::Tensor parent, at::Tensor pb, at::Tensor pnb,
                        at::Tensor nbeam, at::Tensor nodes, at::Tensor nnodes, at::Tensor out, at::Tensor out_len,
                        at::Tensor score) {
  const Op op{"ctc_beam_backtrack"};
  ctc_backtrack_any(op, beam_state(op, node, last, parent, pb, pnb, nbeam, nodes, nnodes), out, out_len, score, nullptr,
                    nullptr, 0);
}
void ctc_beam_backtrack_lm(at::Tensor node, at::Tensor last, at::Tensor parent, at::Tensor pb, at::Tensor pnb,
                           at::Tensor nbeam, at::Tensor nodes, at::Tensor nnodes, at::Tensor out, at::Tensor out_len,
                           at::Tensor score, at::Tensor lm, at::Tensor lmstate, int64_t blank) {
  const Op op{"ctc_beam_backtrack_lm"};
  ctc_backtrack_any(op, beam_state(op, node, last, parent, pb, pnb, nbeam, nodes, nnodes), out, out_len, score, &lm,
                    &lmstate, blank);
}

// out[k] (= or +=) scale[0] * alpha * sum_m G[m, k] for k < K (G bf16 [M, ldg], contiguous: a
// pitched view is refused; scale a device fp32 scalar): the FC head's bias gradient
// (csrc/reduce.hip). M = 0 is legal: out = 0, or out unchanged under acc
void fc_bias_grad(at::Tensor G, int64_t K, at::Tensor scale, double alpha, at::Tensor out, bool acc) {
  const Op op{"fc_bias_grad"};
  op.dims(G, "G", 2, "M, ldg");
  TORCH_CHECK(K >= 1 && K <= 32 && G.size(1) >= 32 && G.size(1) % 8 == 0,
              "fc_bias_grad: 1 <= K <= 32, G of >= 32 columns, ldg % 8 == 0");
  op.launched(ds2_fc_bias_grad(op.bf16(G, "G", "M, ldg", whole(G), 16), (int)G.size(0), (int)G.size(1), (int)K,
                               op.scalar(scale, "scale"), (float)alpha, op.f32(out, "out", "K", exactly(K)), acc ? 1 : 0,
                               op.stream()));
}

// --------------------------------------------------------------------------- fp8 quantisation
int64_t fp8_quant_blocks(int64_t na, int64_t nb) { return ds2_fp8_quant_blocks(na, nb); }

// per-tensor e4m3fn quantisation of two bf16 operands a [rows_a, K], b [rows_b, K] into
// a8 [rows_a, Kp], b8 [rows_b, Kp] (columns >= K zero); scales[0] = amax_a/448,
// scales[1] = amax_b/448 * alpha (device-side, for the fp8 GEMM's epilogue; fp32 [2 or more]).
// part: fp32 [2 * fp8_quant_blocks or more]. a2 / asum (given
// together, a's shape): operand a is a + a2 (a bidirectional layer's two direction outputs),
// its bf16 sum written to asum in the same pass (bitwise torch.add) and quantised from there.
void fp8_quant2(at::Tensor a, at::Tensor b, double alpha, at::Tensor a8, at::Tensor b8, at::Tensor part,
                at::Tensor scales, c10::optional<at::Tensor> a2, c10::optional<at::Tensor> asum) {
  const Op op{"fp8_quant2"};
  TORCH_CHECK(a2.has_value() == asum.has_value(), "fp8_quant2: a2 and asum go together");
  for (const at::Tensor* t : {&a, &b, &a8, &b8}) op.dims(*t, "a / b / a8 / b8", 2, "rows, K");
  const int64_t K = a.size(1), Kp = a8.size(1), ra = a.size(0), rb = b.size(0);
  TORCH_CHECK(b.size(1) == K && a8.size(0) == ra && b8.size(0) == rb && b8.size(1) == Kp && Kp >= K && K % 8 == 0 && Kp % 8 == 0,
              "fp8_quant2: a [rows_a, K], b [rows_b, K], a8 [rows_a, Kp], b8 [rows_b, Kp], Kp >= K, K % 8 == 0");
  TORCH_CHECK(!a2.has_value() || (a2->sizes() == a.sizes() && asum->sizes() == a.sizes()), "fp8_quant2: a2 / asum of a's shape");
  const void* ap = op.bf16(a, "a", "rows_a, K", whole(a), 16);
  const void* bp = op.bf16(b, "b", "rows_b, K", whole(b), 16);
  // the cast stores 8 bytes (uint2) per chunk
  void* a8p = op.raw(a8, "a8", at::kFloat8_e4m3fn, "rows_a, Kp", whole(a8), 8);
  void* b8p = op.raw(b8, "b8", at::kFloat8_e4m3fn, "rows_b, Kp", whole(b8), 8);
  const int nb = ds2_fp8_quant_blocks(ra * Kp, rb * Kp);
  op.launched(ds2_fp8_quant2(ap, ra, bp, rb, (int)K, (int)Kp, (float)alpha, a8p, b8p,
                             op.f32(part, "part", "2 * fp8_quant_blocks", at_least(2 * nb)),
                             op.f32(scales, "scales", "2", at_least(2)), op.bf16(a2, "a2", "rows_a, K", whole(a), 16),
                             op.bf16(asum, "asum", "rows_a, K", whole(a), 16), op.stream()));
}

// --------------------------------------------------------------------------- GEMM (csrc/gemm.hip, csrc/gemm8.hip)
// Operands are (possibly batched) matrices whose innermost dimension is unit-stride; the leading
// dimension is the row stride. a_col / b_col select the column-major reading of the kernels'
// headers. epi 0: bf16 C = alpha*acc + bias; 1: fp32 C = alpha*acc; 2: fp32 C += alpha*acc.
static int dev_cus() {
  static int cus_of[64] = {0};
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "hipGetDevice");
  if (!cus_of[dev])
    TORCH_CHECK(hipDeviceGetAttribute(&cus_of[dev], hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess,
                "CU count");
  return cus_of[dev];
}
int grid_cap(int64_t max_grid) { return max_grid > 0 ? (int)std::min<int64_t>(max_grid, dev_cus()) : dev_cus(); }

// fill: regions the GEMM launch initialises for the next kernel (multi_fill semantics)
DS2Fill make_fill(const Op& op, const std::vector<at::Tensor>& fill, const std::vector<int64_t>& fill_pat) {
  TORCH_CHECK(fill.size() == fill_pat.size() && fill.size() <= 8, "<= 8 (fill region, pattern) pairs");
  DS2Fill fd{};
  fd.n = (int)fill.size();
  for (size_t i = 0; i < fill.size(); ++i) {
    const int64_t bytes = fill[i].numel() * fill[i].element_size();
    TORCH_CHECK(bytes % 4 == 0, op.op, ": fill regions of whole 32-bit words");
    fd.ptr[i] = static_cast<unsigned*>(op.raw(fill[i], "fill region", kAnyDtype, "n", whole(fill[i]), 4));
    fd.words[i] = (unsigned long long)bytes / 4;
    fd.pattern[i] = (unsigned)(uint32_t)fill_pat[i];
  }
  return fd;
}

// The three operands of one GEMM: dtypes, 16-B alignment, unit-stride rows (ld_mult: and row strides
// that are multiples of that many elements), all 2-D or all batched 3-D of one batch
struct GemmAbc {
  Pitched a, b, c;
  int64_t batch;
};
GemmAbc gemm_abc(const Op& op, const at::Tensor& A, const at::Tensor& B, const at::Tensor& C, at::ScalarType ab,
                 at::ScalarType c, int ld_mult, bool batched) {
  const GemmAbc g{op.pitched(A, "A", ab, 16, ld_mult, batched), op.pitched(B, "B", ab, 16, ld_mult, batched),
                  op.pitched(C, "C", c, 16, ld_mult, batched), A.dim() == 3 ? A.size(0) : 1};
  TORCH_CHECK(B.dim() == A.dim() && C.dim() == A.dim(), op.op, ": operands must all be 2-D or all 3-D");
  if (g.batch > 1) TORCH_CHECK(B.size(0) == g.batch && C.size(0) == g.batch, op.op, ": batch mismatch");
  return g;
}
at::ScalarType epi_dtype(const Op& op, int64_t epi, int64_t lo = 0) {
  TORCH_CHECK(epi >= lo && epi <= 2, op.op, ": epi ", lo, "..2");
  return epi == 0 ? at::kBFloat16 : at::kFloat;
}
const void* gemm_bias(const Op& op, const OptT& bias, int64_t epi, int64_t N) {
  TORCH_CHECK(!has(bias) || epi == 0, op.op, ": bias must be bf16 [N] (epi 0)");
  return op.bf16(bias, "bias", "N", exactly(N), 8);
}
// split-K through consecutive ranges of one fp32 workspace (S * batch * M * N floats or more, 16-B
// aligned) and one zeroed int32 counter buffer (tiles or more; one buffer per stream)
void gemm_splitk(const Op& op, const OptT& ws, const OptT& cnt, int S, int64_t MN, int64_t tiles, int64_t& wofs, int64_t& cofs,
                 float*& wsp, unsigned*& cntp) {
  if (S <= 1) return;
  TORCH_CHECK(has(ws) && has(cnt), op.op, ": split-K needs an fp32 workspace and zeroed int32 tile counters");
  wsp = op.f32(ws, "ws", "S, batch, M, N", at_least(wofs + S * MN), 16) + wofs;
  TORCH_CHECK(wofs % 4 == 0, op.op, ": 16-B aligned workspace");
  cntp = op.u32(cnt, "cnt", "tiles", at_least(cofs + tiles)) + cofs;
  wofs += S * MN;
  cofs += tiles;
}

void gemm8(at::Tensor A, at::Tensor B, at::Tensor C, OptT bias, int64_t epi, double alpha, OptT alpha_dev,
           OptT alpha_dev2, bool a_col, bool b_col, int64_t splits, OptT ws, OptT cnt, int64_t max_grid,
           std::vector<at::Tensor> fill, std::vector<int64_t> fill_pat, bool ext_red) {
  const Op op{"gemm8"};
  const bool fp8 = A.scalar_type() == at::kFloat8_e4m3fn;
  const DS2Fill fd = make_fill(op, fill, fill_pat);
  const GemmAbc g = gemm_abc(op, A, B, C, fp8 ? at::kFloat8_e4m3fn : at::kBFloat16, epi_dtype(op, epi), 1, true);
  const int64_t M = a_col ? A.size(-1) : A.size(-2), K = a_col ? A.size(-2) : A.size(-1);
  const int64_t N = b_col ? B.size(-1) : B.size(-2), Kb = b_col ? B.size(-2) : B.size(-1);
  TORCH_CHECK(Kb == K && C.size(-2) == M && C.size(-1) == N, "gemm8: shapes");
  float* wsp = nullptr;
  unsigned* cntp = nullptr;
  int64_t wofs = 0, cofs = 0;
  const int S = ds2_gemm8_splits((int)K, fp8 ? 1 : 0, (int)std::max<int64_t>(1, splits));
  gemm_splitk(op, ws, cnt, S, g.batch * M * N, ((M + 255) / 256) * ((N + 255) / 256) * g.batch, wofs, cofs, wsp, cntp);
  op.launched(ds2_gemm8(g.a.p, g.b.p, g.c.p, gemm_bias(op, bias, epi, N), op.scalar(alpha_dev, "alpha_dev"),
                        op.scalar(alpha_dev2, "alpha_dev2"), (int)M, (int)N, (int)K, (int)g.a.ld, (int)g.b.ld, (int)g.c.ld,
                        fp8 ? 1 : 0, a_col ? 1 : 0, b_col ? 1 : 0, (int)epi, (float)alpha, (int)g.batch, g.a.bs, g.b.bs,
                        g.c.bs, S, wsp, cntp, grid_cap(max_grid), fd.n ? &fd : nullptr, ext_red ? 1 : 0, op.stream()));
}

// A group of independent bf16 GEMMs of the same operand modes in one launch (one grid over all
// their tiles): C[i] (fp32, epi[i] 1 store / 2 accumulate) = A[i] B[i]^T, split-K S[i] through
// consecutive ranges of one workspace ws (S[i] * M * N floats each) and one zeroed counter
// buffer cnt (tiles each).
void gemm8_group(std::vector<at::Tensor> A, std::vector<at::Tensor> B, std::vector<at::Tensor> C,
                 std::vector<int64_t> epi, std::vector<int64_t> splits, bool a_col, bool b_col, OptT ws, OptT cnt,
                 int64_t max_grid) {
  const Op op{"gemm8_group"};
  const size_t np = A.size();
  TORCH_CHECK(np >= 1 && np <= 24 && B.size() == np && C.size() == np && epi.size() == np && splits.size() == np,
              "gemm8_group: 1..24 members, one A, B, C, epi, splits each");
  std::vector<const void*> pa(np), pb(np);
  std::vector<void*> pc(np);
  std::vector<float*> pw(np, nullptr);
  std::vector<unsigned*> pn(np, nullptr);
  std::vector<int> dims(8 * np);
  int64_t wofs = 0, cofs = 0;
  for (size_t i = 0; i < np; ++i) {
    const at::Tensor &a = A[i], &b = B[i], &c = C[i];
    epi_dtype(op, epi[i], 1);
    const GemmAbc g = gemm_abc(op, a, b, c, at::kBFloat16, at::kFloat, 1, false);
    const int64_t M = a_col ? a.size(1) : a.size(0), K = a_col ? a.size(0) : a.size(1);
    const int64_t N = b_col ? b.size(1) : b.size(0), Kb = b_col ? b.size(0) : b.size(1);
    TORCH_CHECK(Kb == K && c.size(0) == M && c.size(1) == N, "gemm8_group: shapes of member ", i);
    const int S = ds2_gemm8_splits((int)K, 0, (int)std::max<int64_t>(1, splits[i]));
    gemm_splitk(op, ws, cnt, S, M * N, ((M + 255) / 256) * ((N + 255) / 256), wofs, cofs, pw[i], pn[i]);
    pa[i] = g.a.p; pb[i] = g.b.p; pc[i] = g.c.p;
    int* d = dims.data() + 8 * i;
    d[0] = (int)M; d[1] = (int)N; d[2] = (int)K;
    d[3] = (int)g.a.ld; d[4] = (int)g.b.ld; d[5] = (int)g.c.ld;
    d[6] = (int)epi[i]; d[7] = S;
  }
  op.launched(ds2_gemm8_group((int)np, pa.data(), pb.data(), pc.data(), pw.data(), pn.data(), dims.data(), a_col ? 1 : 0,
                              b_col ? 1 : 0, grid_cap(max_grid), op.stream()));
}

// csrc/gemm.hip: row strides are multiples of 8 elements. A col-mode operand may be padded to
// Ml / Nl columns and hold only Kl k-rows (the stored extents); alpha_dev is one fp32 device scalar.
void gemm(at::Tensor A, at::Tensor B, at::Tensor C, OptT bias, int64_t M, int64_t N, int64_t K, bool a_col,
          bool b_col, int64_t epi, double alpha, int64_t cfg, OptT alpha_dev, int64_t Ml, int64_t Nl, int64_t Kl,
          std::vector<at::Tensor> fill, std::vector<int64_t> fill_pat) {
  const Op op{"gemm"};
  const DS2Fill fd = make_fill(op, fill, fill_pat);
  const GemmAbc g = gemm_abc(op, A, B, C, at::kBFloat16, epi_dtype(op, epi), 8, true);
  const int64_t Mx = Ml ? Ml : M, Nx = Nl ? Nl : N, Kx = Kl ? Kl : K;
  const int64_t ar = a_col ? Kx : M, ac = a_col ? Mx : K, br = b_col ? Kx : N, bc = b_col ? Nx : K;
  TORCH_CHECK(A.size(-2) == ar && A.size(-1) == ac, "gemm: A shape");
  TORCH_CHECK(B.size(-2) == br && B.size(-1) == bc, "gemm: B shape");
  TORCH_CHECK(C.size(-2) == M && C.size(-1) == N, "gemm: C shape");
  op.launched(ds2_gemm(g.a.p, g.b.p, g.c.p, gemm_bias(op, bias, epi, N), op.scalar(alpha_dev, "alpha_dev", exactly(1)),
                       (int)M, (int)N, (int)K, (int)g.a.ld, (int)g.b.ld, (int)g.c.ld, (int)Ml, (int)Nl, (int)Kl,
                       a_col ? 1 : 0, b_col ? 1 : 0, (int)epi, (float)alpha, (int)g.batch, g.a.bs, g.b.bs, g.c.bs, (int)cfg,
                       fd.n ? &fd : nullptr, op.stream()));
}

// FC head + CTC (training): h [T, N, H] bf16, W [K, H] bf16, bias [K] bf16 -> loss [N] fp32,
// G [T*N, 32] bf16 (per-utterance dloss/dlogits, zero-padded classes); ws fp32 [ctc_ws_floats or more]
// mean (optional, [1] fp32): the batch-mean loss written by the same launch; counter / first_bad
// (optional, [1] int32 each): the per-step divergence watch of utils/stats.py NonfiniteWatch
void head_ctc(at::Tensor h, at::Tensor W, at::Tensor bias, at::Tensor lens, at::Tensor labels, at::Tensor label_lens,
              at::Tensor loss, at::Tensor G, at::Tensor ws, int64_t blank, bool zero_inf, OptT mean, OptT counter,
              OptT first_bad) {
  const Op op{"head_ctc"};
  op.dims(h, "h", 3, "T, N, H");
  op.dims(W, "W", 2, "K, H");
  const int64_t T = h.size(0), N = h.size(1), H = h.size(2), K = W.size(0);
  TORCH_CHECK(W.size(1) == H && K <= 32 && H % 32 == 0, "head_ctc: W [K, H], K <= 32 classes and H % 32 == 0");
  const CtcLabels l = ctc_labels(op, lens, labels, label_lens, N);
  float* mean_p = op.f32(mean, "mean", "1", exactly(1));
  TORCH_CHECK(has(counter) == has(first_bad) && (!has(counter) || mean_p), "head_ctc: the watch needs mean, counter and first_bad");
  op.launched(ds2_head_ctc(op.bf16(h, "h", "T, N, H", whole(h)), op.bf16(W, "W", "K, H", whole(W)),
                           op.bf16(bias, "bias", "K", exactly(K)), l.lens, l.labels, l.label_lens,
                           op.f32(loss, "loss", "N", exactly(N)), op.bf16(G, "G", "T*N, 32", exactly(T * N * 32)),
                           op.f32(ws, "ws", "ctc_ws_floats", at_least(ds2_ctc_ws_floats((int)T, (int)N, l.Lmax))), (int)T,
                           (int)N, (int)H, (int)K, l.Lmax, (int)blank, zero_inf ? 1 : 0, mean_p,
                           op.i32(counter, "counter", "1", exactly(1)), op.i32(first_bad, "first_bad", "1", exactly(1)),
                           op.stream()));
}

// FC head alone: logits [M, K] (fp32 or bf16) = h [M, H] W^T + b
void fc_logits(at::Tensor h, at::Tensor W, at::Tensor bias, at::Tensor logits) {
  const Op op{"fc_logits"};
  op.dims(W, "W", 2, "K, H");
  const int64_t K = W.size(0), H = W.size(1);
  TORCH_CHECK(h.dim() >= 1 && h.size(-1) == H && K <= 32 && H % 32 == 0, "fc_logits: h [..., H], W [K, H], K <= 32, H % 32 == 0");
  const int64_t M = h.numel() / H;
  const Act lg = op.act(logits, "logits", "M, K", exactly(M * K));
  op.launched(ds2_fc_logits(op.bf16(h, "h", "M, H", whole(h)), op.bf16(W, "W", "K, H", whole(W)),
                            op.bf16(bias, "bias", "K", exactly(K)), lg.p, lg.bf16, (int)M, (int)H, (int)K, op.stream()));
}

// --------------------------------------------------------------------------- lookahead convolution (csrc/lookahead.hip)
// Shapes every lookahead entry point shares: x bf16 [T, B, H], lens int32 [B]; tau from w bf16 [H, tau+1]
struct Lookahead {
  const void* x;
  int T, B, H;
};
Lookahead lookahead_x(const Op& op, const at::Tensor& x, const char* name) {
  op.dims(x, name, 3, "T, B, H");
  TORCH_CHECK(x.size(0) >= 1 && x.size(1) >= 1 && x.size(2) % 8 == 0, op.op, ": bf16 [T, B, H] activations, H % 8 == 0");
  return {op.bf16(x, name, "T, B, H", whole(x)), (int)x.size(0), (int)x.size(1), (int)x.size(2)};
}
const void* lookahead_w(const Op& op, const at::Tensor& w, int64_t H, int64_t& tau) {
  op.dims(w, "w", 2, "H, tau+1");
  tau = w.size(1) - 1;
  TORCH_CHECK(tau >= 1 && tau <= 31, op.op, ": w must be bf16 [H, tau+1], 1 <= tau <= 31");
  return op.bf16(w, "w", "H, tau+1", exactly(H * (tau + 1)));
}

// out = r (bwd false, x = h) or dh (bwd true, x = dr)
void lookahead(at::Tensor x, at::Tensor w, at::Tensor lens, at::Tensor out, bool bwd) {
  const Op op{"lookahead"};
  int64_t tau = 0;
  const Lookahead X = lookahead_x(op, x, "x");
  const void* wp = lookahead_w(op, w, X.H, tau);
  op.launched(ds2_lookahead(X.x, wp, op.i32(lens, "lens", "B", exactly(X.B)), op.bf16(out, "out", "T, B, H", whole(x)), X.T,
                            X.B, X.H, (int)tau, bwd ? 1 : 0, op.stream()));
}

int64_t lookahead_wgrad_parts(int64_t T, int64_t B, int64_t H) {
  return ds2_lookahead_wgrad_parts((int)T, (int)B, (int)H);
}

// part [P, H*(tau+1)] fp32, P = lookahead_wgrad_parts(T, B, H); tau is part's to tell
void lookahead_wgrad(at::Tensor dr, at::Tensor h, at::Tensor lens, at::Tensor part, int64_t tau) {
  const Op op{"lookahead_wgrad"};
  const Lookahead D = lookahead_x(op, dr, "dr");
  TORCH_CHECK(tau >= 1 && tau <= 31, "lookahead_wgrad: 1 <= tau <= 31");
  op.launched(ds2_lookahead_wgrad(D.x, op.bf16(h, "h", "T, B, H", whole(dr)), op.i32(lens, "lens", "B", exactly(D.B)),
                                  op.f32(part, "part", "lookahead_wgrad_parts, H*(tau+1)",
                                         exactly((int64_t)ds2_lookahead_wgrad_parts(D.T, D.B, D.H) * D.H * (tau + 1))),
                                  D.T, D.B, D.H, (int)tau, op.stream()));
}

// one streaming step: out [n, B, H] from hist [tau, B, H] and x [n, B, H]; hist is rewritten
void lookahead_stream(at::Tensor hist, at::Tensor x, at::Tensor w, at::Tensor out) {
  const Op op{"lookahead_stream"};
  int64_t tau = 0;
  const Lookahead X = lookahead_x(op, x, "x");
  const void* wp = lookahead_w(op, w, X.H, tau);
  op.launched(ds2_lookahead_stream(op.bf16(hist, "hist", "tau, B, H", exactly(tau * X.B * X.H)), X.x, wp,
                                   op.bf16(out, "out", "n, B, H", whole(x)), X.T, X.B, X.H, (int)tau, op.stream()));
}

// --------------------------------------------------------------------------- SpecAugment (csrc/specaug.hip)
// x, out fp32 [B, T, F]; lens int32 [B]; plan int32 [B, 2 + 2 nF + 2 nT]
struct Spec {
  const float* x;
  const int* lens;
  int B, T, F;
};
Spec specaug_x(const Op& op, const at::Tensor& x, const at::Tensor& lens) {
  op.dims(x, "x", 3, "B, T, F");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= 65535 && x.size(1) >= 1 && x.size(1) <= 32767 && x.size(2) >= 1 &&
                  x.size(2) <= 1024,
              "specaug: B <= 65535, T <= 32767, F <= 1024");
  return {op.f32(x, "x", "B, T, F", whole(x)), op.i32(lens, "lens", "B", exactly(x.size(0))), (int)x.size(0), (int)x.size(1),
          (int)x.size(2)};
}
int* specaug_plan_arg(const Op& op, const at::Tensor& plan, int64_t B, int64_t nF, int64_t nT) {
  TORCH_CHECK(nF >= 0 && nF <= 8 && nT >= 0 && nT <= 16, op.op, ": nF <= 8, nT <= 16");
  return op.i32(plan, "plan", "B, 2 + 2 nF + 2 nT", exactly(B * (2 + 2 * nF + 2 * nT)));
}

// seed, step and first_utt come as 32-bit words
void specaug_plan(at::Tensor lens, at::Tensor plan, int64_t T, int64_t F, int64_t nF, int64_t Fw, int64_t nT,
                  int64_t Tw, int64_t p_ppm, int64_t W, int64_t seed_lo, int64_t seed_hi, int64_t step_lo,
                  int64_t step_hi, int64_t first_utt) {
  const Op op{"specaug_plan"};
  const int64_t B = lens.numel();
  const auto in31 = [](int64_t v, int64_t lo) { return v >= lo && v < (1LL << 31); };
  TORCH_CHECK(in31(B, 1) && in31(T, 1) && in31(F, 1), "specaug_plan: B, T, F in [1, 2^31)");
  TORCH_CHECK(in31(Fw, 0) && in31(Tw, 0) && in31(W, 0) && in31(p_ppm, 0), "specaug_plan: policy value out of range");
  op.launched(ds2_specaug_plan(op.i32(lens, "lens", "B", whole(lens)), specaug_plan_arg(op, plan, B, nF, nT), (int)B, (int)T,
                               (int)F, (int)nF, (int)Fw, (int)nT, (int)Tw, (int)p_ppm, (int)W, op.word(seed_lo, "seed_lo"),
                               op.word(seed_hi, "seed_hi"), op.word(step_lo, "step_lo"), op.word(step_hi, "step_hi"),
                               op.word(first_utt, "first_utt"), op.stream()));
}

void specaug_mean(at::Tensor x, at::Tensor lens, at::Tensor mean) {
  const Op op{"specaug_mean"};
  const Spec s = specaug_x(op, x, lens);
  op.launched(ds2_specaug_mean(s.x, s.lens, op.f32(mean, "mean", "B, F", exactly((int64_t)s.B * s.F)), s.B, s.T, s.F, op.stream()));
}

// out = SpecAugment(x) by plan; fill [B, F] or None (zeros); inplace: out is x and only masked cells are written
void specaug_apply(at::Tensor x, at::Tensor lens, at::Tensor plan, OptT fill, at::Tensor out, int64_t nF, int64_t nT,
                   bool inplace) {
  const Op op{"specaug_apply"};
  const Spec s = specaug_x(op, x, lens);
  op.launched(ds2_specaug_apply(s.x, s.lens, specaug_plan_arg(op, plan, s.B, nF, nT),
                                op.f32(fill, "fill", "B, F", exactly((int64_t)s.B * s.F)),
                                op.f32(out, "out", "B, T, F", whole(x)), s.B, s.T, s.F, (int)nF, (int)nT, inplace ? 1 : 0,
                                op.stream()));
}

// --------------------------------------------------------------------------- dropout (csrc/dropout.hip)
// out = dropout(x) under the mask of (seed, ctr = (step, first_utt) on the device, site); out may be x
void seq_dropout(at::Tensor x, at::Tensor out, at::Tensor ctr, int64_t seed_lo, int64_t seed_hi, int64_t site,
                 int64_t thr, double scale, bool locked) {
  const Op op{"seq_dropout"};
  op.dims(x, "x", 3, "T, N, H");
  TORCH_CHECK(x.size(0) >= 1 && x.size(1) >= 1 && x.size(2) >= 8 && x.size(2) % 8 == 0 && x.size(2) <= 8 * 65536,
              "seq_dropout: bf16 x, out [T, N, H], H % 8 == 0");
  TORCH_CHECK(x.numel() / 8 < (1LL << 31), "seq_dropout: T * N * H / 8 < 2^31");
  TORCH_CHECK(site >= 0 && site < 16384 && thr >= 1 && thr <= 65535, "seq_dropout: site < 16384, 1 <= thr <= 65535");
  op.launched(ds2_seq_dropout(op.bf16(x, "x", "T, N, H", whole(x)), op.bf16(out, "out", "T, N, H", whole(x)),
                              op.i32(ctr, "ctr", "2", at_least(2)), (int)x.size(0), (int)x.size(1), (int)x.size(2),
                              op.word(seed_lo, "seed_lo"), op.word(seed_hi, "seed_hi"), (int)site, (int)thr, (float)scale,
                              locked ? 1 : 0, op.stream()));
}

// --------------------------------------------------------------------------- audio (csrc/featurize.hip, csrc/resample.hip)
// What the audio entry points share: pcm [B, S] fp32 or int16, optional lens int32 [B], and
// (featurize, audio_stats) the per-row fp32 [B] offset and gain
struct Pcm {
  const void* p;
  int i16;
  int64_t B, S;
  const int* lens;
};
Pcm pcm_arg(const Op& op, const at::Tensor& pcm, const OptT& lens) {
  op.dims(pcm, "pcm", 2, "B, S");
  TORCH_CHECK(pcm.scalar_type() == at::kShort || pcm.scalar_type() == at::kFloat, op.op, ": pcm must be float32 or int16");
  TORCH_CHECK(pcm.size(1) < (1LL << 31), op.op, ": pcm rows of S < 2^31 samples");
  return {op.raw(pcm, "pcm", pcm.scalar_type(), "B, S", whole(pcm)), pcm.scalar_type() == at::kShort ? 1 : 0, pcm.size(0),
          pcm.size(1), op.lens(lens, "lens", pcm.size(0))};
}
float* per_row(const Op& op, const at::Tensor& t, const char* name, int64_t B) { return op.f32(t, name, "B", exactly(B)); }

// per-row offset = mean(x) and gain = 1 / max|x - mean| (1 when the peak is 0), on the device
void audio_stats(at::Tensor pcm, OptT lens, at::Tensor offset, at::Tensor gain) {
  const Op op{"audio_stats"};
  const Pcm a = pcm_arg(op, pcm, lens);
  op.launched(ds2_audio_stats(a.p, a.i16, a.S, (int)a.S, (int)a.B, a.lens, per_row(op, offset, "offset", a.B),
                              per_row(op, gain, "gain", a.B), op.stream()));
}

// kind 0 = mfcc (tables: basis [400, 512], mel_idx [322, 2], mel_w [322, 8], dct [322, 192], lifter [161]),
// kind 1 = spectrogram (basis [320, 320] with the window folded in). lead = 1: pcm[:, 0] is the sample before
// the first one (a stream's later calls). mode: 0 whole signal, 1 stream in flight, 2 stream end.
void featurize(at::Tensor pcm, OptT lens, at::Tensor offset, at::Tensor gain, at::Tensor basis, OptT mel_idx,
               OptT mel_w, OptT dct, OptT lifter, int64_t kind, int64_t lead, int64_t mode, at::Tensor out,
               at::Tensor frames) {
  const Op op{"featurize"};
  const Pcm p = pcm_arg(op, pcm, lens);
  TORCH_CHECK(kind == 0 || kind == 1, "featurize: kind 0 (mfcc) or 1 (spectrogram)");
  TORCH_CHECK((lead == 0 || lead == 1) && mode >= 0 && mode <= 2 && p.S >= lead, "featurize: lead / mode / S");
  op.dims(out, "out", 3, "B, T_max, 161");
  TORCH_CHECK(out.size(0) == p.B && out.size(2) == 161, "featurize: out must be [B, T_max, 161]");
  const Act o = op.act(out, "out", "B, T_max, 161", whole(out));
  DS2Feat a{};
  a.pcm = p.p;
  a.row_stride = p.S;
  a.S = (int)p.S; a.lead = (int)lead; a.mode = (int)mode; a.B = (int)p.B; a.T_max = (int)out.size(1);
  a.lens = p.lens;
  a.offset = per_row(op, offset, "offset", p.B);
  a.gain = per_row(op, gain, "gain", p.B);
  a.basis = kind == 0 ? op.f32(basis, "basis", "400, 512", exactly(400 * 512))
                      : op.f32(basis, "basis", "320, 320", exactly(320 * 320));
  if (kind == 0) {
    TORCH_CHECK(has(mel_idx) && has(mel_w) && has(dct) && has(lifter), "featurize: mfcc needs the mel, DCT and lifter tables");
    a.mel_idx = op.i32(mel_idx, "mel_idx", "322, 2", exactly(322 * 2));
    a.mel_w = op.f32(mel_w, "mel_w", "322, 8", exactly(322 * 8));
    a.dct = op.f32(dct, "dct", "322, 192", exactly(322 * 192));
    a.lifter = op.f32(lifter, "lifter", "161", exactly(161));
  }
  a.out = o.p;
  a.frames = op.i32(frames, "frames", "B", exactly(p.B));
  op.launched(ds2_featurize(&a, (int)kind, p.i16, o.bf16, op.stream()));
}

// out [B, n_out] fp32 and out_lens [B] int32 of one whole call (in_off = -(K/2 - 1), ph0 = 0, to_end) or of one
// stream push (buffer-relative in_off and start phase); h fp32 [L, K]
void resample(at::Tensor pcm, OptT lens, at::Tensor h, int64_t L, int64_t M, int64_t in_off, int64_t ph0,
              bool to_end, at::Tensor out, at::Tensor out_lens) {
  const Op op{"resample"};
  const Pcm p = pcm_arg(op, pcm, lens);
  op.dims(h, "h", 2, "L, K");
  op.dims(out, "out", 2, "B, n_out");
  const int64_t K = h.size(1);
  TORCH_CHECK(h.size(0) == L && L >= 1 && M >= 1 && ds2_resample_supported((int)L, (int)M, (int)K),
              "resample: h [L, K] and (L, M, K) inside the kernel's contract");
  TORCH_CHECK(out.size(0) == p.B && out.size(1) < (1LL << 31), "resample: out must be fp32 [B, n_out]");
  TORCH_CHECK(in_off > -(1LL << 31) && in_off < (1LL << 31) && ph0 >= 0 && ph0 < L, "resample: in_off / ph0");
  op.launched(ds2_resample(p.p, p.i16, p.S, (int)p.S, (int)p.B, p.lens, op.f32(h, "h", "L, K", whole(h)), (int)L, (int)M,
                           (int)K, (int)in_off, (int)ph0, (int)out.size(1), to_end ? 1 : 0,
                           op.f32(out, "out", "B, n_out", whole(out)), op.i32(out_lens, "out_lens", "B", exactly(p.B)),
                           op.stream()));
}

// --------------------------------------------------------------------------- noise augmentation (csrc/waveaug.hip)
// x fp32 or int16 [B, S] (S % 8 == 0, 16-byte aligned), optional lens int32 [B], plan int32 [B, 4] =
// (on, clip, off, snr_cdb); the bank: data fp32 [Ntot], start and length int32 [C]
struct Wave {
  const void* x;
  int i16;
  int B, S;
  const int* lens;
};
Wave waveaug_x(const Op& op, const at::Tensor& x, const OptT& lens) {
  op.dims(x, "x", 2, "B, S");
  TORCH_CHECK(x.scalar_type() == at::kShort || x.scalar_type() == at::kFloat, op.op, ": x must be float32 or int16");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= 65535 && x.size(1) >= 8 && x.size(1) < (1LL << 30) && x.size(1) % 8 == 0,
              op.op, ": x [B, S] with B <= 65535, 8 <= S < 2^30, S % 8 == 0, got ", x.sizes());
  return {op.raw(x, "x", x.scalar_type(), "B, S", whole(x), 16), x.scalar_type() == at::kShort ? 1 : 0, (int)x.size(0),
          (int)x.size(1), op.lens(lens, "lens", x.size(0))};
}
int* waveaug_plan_arg(const Op& op, const at::Tensor& plan, int64_t B) {
  return op.i32(plan, "plan", "B, 4", exactly(4 * B), 16);
}
struct NoiseBank {
  const float* data;
  const int *start, *length;
  int C;
  long long Ntot;
};
NoiseBank waveaug_bank(const Op& op, const at::Tensor& data, const at::Tensor& start, const at::Tensor& length) {
  const int64_t C = length.numel(), Ntot = data.numel();
  TORCH_CHECK(C >= 1 && C < (1LL << 31) && Ntot >= 1 && Ntot < (1LL << 31), op.op,
              ": a bank of C >= 1 clips and 1 <= Ntot < 2^31 samples");
  return {op.f32(data, "data", "Ntot", whole(data)), op.i32(start, "start", "C", exactly(C)),
          op.i32(length, "length", "C", whole(length)), (int)C, (long long)Ntot};
}
int64_t waveaug_segments(int64_t S) { return (S + ds2_waveaug_segment() - 1) / ds2_waveaug_segment(); }

// seed, step and first_utt come as 32-bit words; p in parts per million, the SNR range in centi-dB
void waveaug_plan(OptT lens, at::Tensor length, at::Tensor plan, int64_t S, int64_t p_ppm, int64_t snr_lo_cdb,
                  int64_t snr_hi_cdb, int64_t seed_lo, int64_t seed_hi, int64_t step_lo, int64_t step_hi,
                  int64_t first_utt) {
  const Op op{"waveaug.plan"};
  op.dims(plan, "plan", 2, "B, 4");
  const int64_t B = plan.size(0), C = length.numel();
  TORCH_CHECK(B >= 1 && B < (1LL << 31) && S >= 1 && S < (1LL << 31) && C >= 1 && C < (1LL << 31), op.op,
              ": B, S, C in [1, 2^31)");
  TORCH_CHECK(p_ppm >= 0 && p_ppm <= 1000000 && snr_lo_cdb >= -(1 << 20) && snr_hi_cdb <= (1 << 20) &&
                  snr_lo_cdb <= snr_hi_cdb,
              op.op, ": policy value out of range");
  op.launched(ds2_waveaug_plan(op.lens(lens, "lens", B), op.i32(length, "length", "C", whole(length)),
                               waveaug_plan_arg(op, plan, B), (int)B, (int)S, (int)C, (int)p_ppm,
                               (int)snr_lo_cdb, (int)snr_hi_cdb, op.word(seed_lo, "seed_lo"), op.word(seed_hi, "seed_hi"),
                               op.word(step_lo, "step_lo"), op.word(step_hi, "step_hi"), op.word(first_utt, "first_utt"),
                               op.stream()));
}

// part fp32 [B, segments of S, 2] = (sum x^2, sum z^2) per segment; segments at or past a row's length are not written
void waveaug_energy(at::Tensor x, OptT lens, at::Tensor plan, at::Tensor data, at::Tensor start, at::Tensor length,
                    at::Tensor part) {
  const Op op{"waveaug.energy"};
  const Wave w = waveaug_x(op, x, lens);
  const NoiseBank k = waveaug_bank(op, data, start, length);
  op.launched(ds2_waveaug_energy(w.x, w.i16, w.lens, waveaug_plan_arg(op, plan, w.B), k.data, k.start, k.length, k.C,
                                 k.Ntot, op.f32(part, "part", "B, segments, 2", exactly(2 * w.B * waveaug_segments(w.S))),
                                 w.B, w.S, op.stream()));
}

// energy fp64 [B, 2] = (Ex, En), the partials added in fp64; coef fp32 [B] = k (0 where the plan is off)
void waveaug_coef(OptT lens, at::Tensor plan, at::Tensor part, at::Tensor energy, at::Tensor coef, int64_t S) {
  const Op op{"waveaug.coef"};
  op.dims(plan, "plan", 2, "B, 4");
  const int64_t B = plan.size(0);
  TORCH_CHECK(B >= 1 && B <= 65535 && S >= 8 && S < (1LL << 30) && S % 8 == 0, op.op,
              ": B <= 65535, 8 <= S < 2^30, S % 8 == 0");
  op.launched(ds2_waveaug_coef(op.lens(lens, "lens", B), waveaug_plan_arg(op, plan, B),
                               op.f32(part, "part", "B, segments, 2", exactly(2 * B * waveaug_segments(S))),
                               static_cast<double*>(op.raw(energy, "energy", at::kDouble, "B, 2", exactly(2 * B))),
                               op.f32(coef, "coef", "B", exactly(B)), (int)B, (int)S, op.stream()));
}

// out fp32 [B, S] = x + coef * noise under the plan; rows that are off are copied, the tail past lens is +0
void waveaug_apply(at::Tensor x, OptT lens, at::Tensor plan, at::Tensor coef, at::Tensor data, at::Tensor start,
                   at::Tensor length, at::Tensor out) {
  const Op op{"waveaug.apply"};
  const Wave w = waveaug_x(op, x, lens);
  const NoiseBank k = waveaug_bank(op, data, start, length);
  op.launched(ds2_waveaug_apply(w.x, w.i16, w.lens, waveaug_plan_arg(op, plan, w.B), op.f32(coef, "coef", "B", exactly(w.B)),
                                k.data, k.start, k.length, k.C, k.Ntot,
                                op.f32(out, "out", "B, S", exactly((int64_t)w.B * w.S), 16), w.B, w.S, op.stream()));
}

// --------------------------------------------------------------------------- speed perturbation (csrc/speed.hip)
// A policy crosses the boundary as 5 V integers, (pct, L, M, K, table offset) per variant; h fp32 holds the
// variants' tables back to back; plan int32 [B, 2] = (pct, n_out)
DS2SpeedTable speed_table(const Op& op, const std::vector<int64_t>& vtab, int64_t h_words) {
  TORCH_CHECK(!vtab.empty() && vtab.size() % 5 == 0 && vtab.size() <= 40, op.op,
              ": a policy is 5 V integers (pct, L, M, K, offset), 1 <= V <= 8, got ", vtab.size());
  DS2SpeedTable t{};
  t.V = (int)(vtab.size() / 5);
  for (int v = 0; v < t.V; ++v) {
    for (int i = 0; i < 5; ++i)
      TORCH_CHECK(vtab[5 * v + i] >= 0 && vtab[5 * v + i] < (1LL << 31), op.op, ": policy word out of range");
    t.pct[v] = (int)vtab[5 * v], t.L[v] = (int)vtab[5 * v + 1], t.M[v] = (int)vtab[5 * v + 2];
    t.K[v] = (int)vtab[5 * v + 3], t.off[v] = (int)vtab[5 * v + 4];
  }
  TORCH_CHECK(ds2_speed_supported(&t, h_words), op.op,
              ": policy outside the kernels' contract (distinct percents in 50..200, L pct == 100 M, K even and <= 320, "
              "tables inside h, 160 KB of LDS)");
  return t;
}
int* speed_plan_arg(const Op& op, const at::Tensor& plan, int64_t B) { return op.i32(plan, "plan", "B, 2", exactly(2 * B)); }

// seed, step and first_utt come as 32-bit words; min_out int32 [B] or None, max_out 0: none
void speed_plan(OptT lens, OptT min_out, at::Tensor plan, int64_t S, int64_t max_out, std::vector<int64_t> vtab,
                int64_t seed_lo, int64_t seed_hi, int64_t step_lo, int64_t step_hi, int64_t first_utt) {
  const Op op{"speed.plan"};
  op.dims(plan, "plan", 2, "B, 2");
  const int64_t B = plan.size(0);
  TORCH_CHECK(B >= 1 && B < (1LL << 31) && S >= 1 && S < (1LL << 30) && max_out >= 0 && max_out < (1LL << 31), op.op,
              ": B in [1, 2^31), S in [1, 2^30), max_out in [0, 2^31)");
  const DS2SpeedTable t = speed_table(op, vtab, 1LL << 40);
  op.launched(ds2_speed_plan(op.lens(lens, "lens", B), op.i32(min_out, "min_out", "B", exactly(B)), speed_plan_arg(op, plan, B),
                             (int)B, (int)S, (int)max_out, &t, op.word(seed_lo, "seed_lo"), op.word(seed_hi, "seed_hi"),
                             op.word(step_lo, "step_lo"), op.word(step_hi, "step_hi"), op.word(first_utt, "first_utt"),
                             op.stream()));
}

// out fp32 [B, n_out], out_lens int32 [B]. tight: the caller derived n_out from the plan of a host copy of the
// lengths; without it n_out must hold the worst case of the policy
void speed_apply(at::Tensor x, OptT lens, at::Tensor plan, at::Tensor h, std::vector<int64_t> vtab, at::Tensor out,
                 at::Tensor out_lens, bool tight) {
  const Op op{"speed.apply"};
  op.dims(x, "x", 2, "B, S");
  op.dims(out, "out", 2, "B, n_out");
  TORCH_CHECK(x.scalar_type() == at::kShort || x.scalar_type() == at::kFloat, op.op, ": x must be float32 or int16");
  const int64_t B = x.size(0), S = x.size(1), n_out = out.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && S >= 1 && S < (1LL << 30), op.op, ": x [B, S] with B <= 65535, 1 <= S < 2^30, got ",
              x.sizes());
  const DS2SpeedTable t = speed_table(op, vtab, h.numel());
  TORCH_CHECK(out.size(0) == B && n_out >= 1 && n_out < (1LL << 31) && (tight || n_out >= ds2_speed_out_width(&t, S)), op.op,
              ": out must be fp32 [B, n_out] with n_out >= ", ds2_speed_out_width(&t, S),
              " (the policy's worst case) unless the caller vouches for a tight width, got ", out.sizes());
  op.launched(ds2_speed_apply(op.raw(x, "x", x.scalar_type(), "B, S", whole(x)), x.scalar_type() == at::kShort ? 1 : 0, (int)B,
                              (int)S, op.lens(lens, "lens", B), speed_plan_arg(op, plan, B),
                              op.f32(h, "h", "table words", whole(h), 16), h.numel(), &t,
                              op.f32(out, "out", "B, n_out", whole(out)), (int)n_out, tight ? 1 : 0,
                              op.i32(out_lens, "out_lens", "B", exactly(B)), op.stream()));
}

// --------------------------------------------------------------------------- summaries (csrc/stats.hip)
// counts int32 [hist_nbucket]; part fp32 [hist_blocks(n), 6 or more]
void hist_stats(at::Tensor x, at::Tensor counts, at::Tensor part) {
  const Op op{"hist_stats"};
  const Act X = op.act(x, "x", "n", whole(x));
  const int blocks = ds2_hist_blocks(x.numel());
  op.launched(ds2_hist_stats(X.p, X.bf16, x.numel(), op.u32(counts, "counts", "hist_nbucket", exactly(ds2_hist_nbucket())),
                             op.f32(part, "part", "hist_blocks, 6", at_least(6 * blocks)), blocks, op.stream()));
}

void nonfinite_watch(at::Tensor loss, at::Tensor counter, at::Tensor first_bad) {
  const Op op{"nonfinite_watch"};
  op.launched(ds2_nonfinite_watch(op.f32(loss, "loss", "1", exactly(1)), op.i32(counter, "counter", "1", exactly(1)),
                                  op.i32(first_bad, "first_bad", "1", exactly(1)), op.stream()));
}

// a test aid: `blocks` workgroups spin for `ticks`, then bump done (int32 [1 or more])
void spin(int64_t ticks, int64_t blocks, int64_t threads, int64_t lds_bytes, at::Tensor done) {
  const Op op{"spin"};
  op.launched(ds2_spin(ticks, (int)blocks, (int)threads, (int)lds_bytes, op.i32(done, "done", "1", at_least(1)), op.stream()));
}

py::tuple gemm_tile(int64_t cfg) {
  int bm = 0, bn = 0;
  TORCH_CHECK(ds2_gemm_tile((int)cfg, &bm, &bn) == 0, "gemm_tile: bad cfg");
  return py::make_tuple(bm, bn);
}

// --------------------------------------------------------------------------- device info
py::dict device_info(int64_t dev) {
  hipDeviceProp_t prop;
  TORCH_CHECK(hipGetDeviceProperties(&prop, (int)dev) == hipSuccess, "hipGetDeviceProperties failed");
  py::dict d;
  d["name"] = std::string(prop.name);
  d["gcn_arch"] = std::string(prop.gcnArchName);
  d["cus"] = prop.multiProcessorCount;
  d["lds_per_block"] = (int64_t)prop.sharedMemPerBlock;
  d["clock_khz"] = prop.clockRate;
  d["total_mem"] = (int64_t)prop.totalGlobalMem;
  return d;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "deepspeech_amd gfx950 kernels";
  m.def("rnn_fwd", &rnn_fwd);
  m.def("rnn_bwd", &rnn_bwd);
  m.def("rnn_kpw", &rnn_kpw);
  m.def("rnnf8_fwd", &rnnf8_fwd);
  m.def("rnnf8_supported", [](int64_t H, int64_t N, int64_t ndir) { return ds2_rnnf8_supported((int)H, (int)N, (int)ndir); });
  m.def("fp8_quant_pow2", &fp8_quant_pow2);
  m.def("fp8_quant_pow2_t", &fp8_quant_pow2_t);
  m.def("fp8_quant_u", &fp8_quant_u);
  m.def("rnnf8_bwd", &rnnf8_bwd);
  m.def("rnnf8_bwd_supported", [](int64_t H, int64_t N, int64_t ndir) {
    return ds2_rnnf8_bwd_supported((int)H, (int)N, (int)ndir);
  });
  m.def("rnnf8_ring_words", [](int64_t H, int64_t BG, int64_t R) { return ds2_rnnf8_ring_words((int)H, (int)BG, (int)R); });
  m.def("rnnx_fwd", &rnnx_fwd);
  m.def("rnnx_bwd", &rnnx_bwd);
  m.def("rnnx_members", [](int64_t H, int64_t cell) { return ds2_rnnx_members((int)H, (int)cell); });
  m.def("rnnx_fwd_family", [](int64_t H, int64_t cell, int64_t knobs) {
    return ds2_rnnx_fwd_family((int)H, (int)cell, (int)knobs);
  });
  m.def("rnnx_bwd_family", [](int64_t H, int64_t cell, int64_t R) { return ds2_rnnx_bwd_family((int)H, (int)cell, (int)R); });
  m.def("rnnx_fwd_fuses_sum", [](int64_t H, int64_t cell, int64_t ndir, int64_t knobs) {
    return ds2_rnnx_fwd_fuses_sum((int)H, (int)cell, (int)ndir, (int)knobs) != 0;
  });
  m.def("rnnx_grid", [](int64_t H, int64_t cell, int64_t ngroups, int64_t xcd_map) {
    return ds2_rnnx_grid((int)H, (int)cell, (int)ngroups, (int)xcd_map);
  });
  m.def("rnnx_ring_floats", [](int64_t H, int64_t BG, int64_t R) { return ds2_rnnx_ring_floats((int)H, (int)BG, (int)R); });
  m.def("ctc_fused", &ctc_fused);
  m.def("ctc_ws_floats", &ctc_ws_floats);
  m.def("ctc_align", &ctc_align);
  m.def("ctc_align_ws_bytes", &ctc_align_ws_bytes);
  m.def("bn_chunks", &bn_chunks);
  m.def("bn_stats", &bn_stats);
  m.def("bn_apply", &bn_apply);
  m.def("bn_bwd", &bn_bwd);
  m.def("adam_ema", &adam_ema, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("ema"),
        py::arg("p16"), py::arg("lr_t"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("gscale"),
        py::arg("ema_keep"), py::arg("skip"), py::arg("max_grid"), py::arg("hyper") = py::none(),
        py::arg("lds_reserve") = 0, py::arg("clip") = py::none());
  m.def("adam_ema_ranges", &adam_ema_ranges, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
        py::arg("ema"), py::arg("p16"), py::arg("lohi"), py::arg("lr_t"), py::arg("b1"), py::arg("b2"),
        py::arg("eps"), py::arg("gscale"), py::arg("ema_keep"), py::arg("hyper") = py::none(),
        py::arg("clip") = py::none());
  m.def("grad_norm_blocks", &grad_norm_blocks);
  m.def("grad_norm", &grad_norm);
  m.def("grad_sumsq_segment", &grad_sumsq_segment);
  m.def("grad_sumsq", &grad_sumsq, py::arg("g"), py::arg("gscale"), py::arg("part"), py::arg("max_grid") = 0,
        py::arg("nontemporal") = true);
  m.def("clip_finalize", &clip_finalize, py::arg("part"), py::arg("max_norm"), py::arg("state"));
  m.def("cast_bf16", &cast_bf16);
  m.def("device_info", &device_info);
  m.def("fp8_quant_blocks", &fp8_quant_blocks);
  m.def("prep_inputs", &prep_inputs);
  m.def("multi_copy", &multi_copy, py::arg("dsts"), py::arg("srcs"), py::arg("sdst") = py::none(),
        py::arg("svals") = std::vector<double>{});
  m.def("fp8_quant2", &fp8_quant2, py::arg("a"), py::arg("b"), py::arg("alpha"), py::arg("a8"), py::arg("b8"),
        py::arg("part"), py::arg("scales"), py::arg("a2") = py::none(), py::arg("asum") = py::none());
  m.def("transpose_bf16", &transpose_bf16);
  m.def("gemm8", &gemm8, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias"), py::arg("epi"),
        py::arg("alpha") = 1.0, py::arg("alpha_dev") = py::none(), py::arg("alpha_dev2") = py::none(),
        py::arg("a_col") = false, py::arg("b_col") = false, py::arg("splits") = 1, py::arg("ws") = py::none(),
        py::arg("cnt") = py::none(), py::arg("max_grid") = 0, py::arg("fill") = std::vector<at::Tensor>{},
        py::arg("fill_pat") = std::vector<int64_t>{}, py::arg("ext_red") = false);
  m.def("gemm8_group", &gemm8_group, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("epi"), py::arg("splits"),
        py::arg("a_col"), py::arg("b_col"), py::arg("ws"), py::arg("cnt"), py::arg("max_grid"));
  m.def("gemm8_splits", [](int64_t K, bool fp8, int64_t S) { return ds2_gemm8_splits((int)K, fp8 ? 1 : 0, (int)S); });
  m.def("multi_fill", &multi_fill);
  m.def("col_sum", &col_sum);
  m.def("wait_resident", &wait_resident);
  m.def("fc_bias_grad", &fc_bias_grad);
  m.def("ctc_beam", &ctc_beam);
  m.def("ctc_beam_backtrack", &ctc_beam_backtrack);
  m.def("ctc_beam_lm", &ctc_beam_lm);
  m.def("ctc_beam_backtrack_lm", &ctc_beam_backtrack_lm);
  m.def("event_new", &event_new, py::arg("flags") = 0);
  m.def("arm_stop_event", &arm_stop_event);
  m.def("disarm_stop_event", &disarm_stop_event);
  m.def("event_free", &event_free);
  m.def("event_record", &event_record);
  m.def("event_wait", &event_wait);
  m.def("event_query", &event_query);
  m.def("stream_wait", &stream_wait);
  m.def("ctc_greedy", &ctc_greedy, py::arg("logits"), py::arg("lens"), py::arg("labels"), py::arg("counts"),
        py::arg("blank"), py::arg("score") = py::none());
  m.def("conv1_fwd", &conv1_fwd);
  m.def("conv1_fwd_grid", &conv1_fwd_grid);
  m.def("conv2_fwd", &conv2_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("part"),
        py::arg("grid"), py::arg("trace") = py::none());
  m.def("conv2_dgrad", &conv2_dgrad, py::arg("dy"), py::arg("w"), py::arg("dx"), py::arg("grid"),
        py::arg("y1") = py::none(), py::arg("mean") = py::none(), py::arg("invstd") = py::none(),
        py::arg("gamma") = py::none(), py::arg("beta") = py::none(), py::arg("part") = py::none(),
        py::arg("trace") = py::none());
  m.def("conv2_wgrad", &conv2_wgrad);
  m.def("conv1_wgrad", &conv1_wgrad, py::arg("dy"), py::arg("x"), py::arg("part"), py::arg("dw"), py::arg("grid"),
        py::arg("y1") = py::none(), py::arg("mean") = py::none(), py::arg("invstd") = py::none(),
        py::arg("gamma") = py::none(), py::arg("beta") = py::none(), py::arg("dbeta") = py::none(),
        py::arg("dgamma") = py::none());
  m.def("conv2_wgrad_part_floats", &conv2_wgrad_part_floats);
  m.def("conv1_wgrad_part_floats", &conv1_wgrad_part_floats);
  m.def("bn_cl_finalize", &bn_cl_finalize);
  m.def("bn_cl_apply", &bn_cl_apply);
  m.def("bn_cl_bwd", &bn_cl_bwd, py::arg("dz"), py::arg("y"), py::arg("mean"), py::arg("invstd"), py::arg("gamma"),
        py::arg("beta"), py::arg("part"), py::arg("nb"), py::arg("dgamma"), py::arg("dbeta"), py::arg("dy"),
        py::arg("tmaj"), py::arg("part_ready") = 0);
  m.def("gemm", &gemm, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("a_col"), py::arg("b_col"), py::arg("epi"), py::arg("alpha"), py::arg("cfg"),
        py::arg("alpha_dev") = py::none(), py::arg("Ml") = 0, py::arg("Nl") = 0, py::arg("Kl") = 0,
        py::arg("fill") = std::vector<at::Tensor>{}, py::arg("fill_pat") = std::vector<int64_t>{});
  m.def("gemm_tile", &gemm_tile);
  m.def("head_ctc", &head_ctc, py::arg("h"), py::arg("W"), py::arg("bias"), py::arg("lens"), py::arg("labels"),
        py::arg("label_lens"), py::arg("loss"), py::arg("G"), py::arg("ws"), py::arg("blank"), py::arg("zero_inf"),
        py::arg("mean") = py::none(), py::arg("counter") = py::none(), py::arg("first_bad") = py::none());
  m.def("fc_logits", &fc_logits);
  m.def("lookahead", &lookahead);
  m.def("lookahead_wgrad_parts", &lookahead_wgrad_parts);
  m.def("lookahead_wgrad", &lookahead_wgrad);
  m.def("lookahead_stream", &lookahead_stream);
  m.def("specaug_plan", &specaug_plan);
  m.def("specaug_mean", &specaug_mean);
  m.def("specaug_apply", &specaug_apply, py::arg("x"), py::arg("lens"), py::arg("plan"), py::arg("fill"),
        py::arg("out"), py::arg("nF"), py::arg("nT"), py::arg("inplace"));
  m.def("seq_dropout", &seq_dropout, py::arg("x"), py::arg("out"), py::arg("ctr"), py::arg("seed_lo"),
        py::arg("seed_hi"), py::arg("site"), py::arg("thr"), py::arg("scale"), py::arg("locked"));
  m.def("audio_stats", &audio_stats, py::arg("pcm"), py::arg("lens"), py::arg("offset"), py::arg("gain"));
  m.def("featurize", &featurize, py::arg("pcm"), py::arg("lens"), py::arg("offset"), py::arg("gain"),
        py::arg("basis"), py::arg("mel_idx"), py::arg("mel_w"), py::arg("dct"), py::arg("lifter"), py::arg("kind"),
        py::arg("lead"), py::arg("mode"), py::arg("out"), py::arg("frames"));
  m.def("resample", &resample, py::arg("pcm"), py::arg("lens"), py::arg("h"), py::arg("L"), py::arg("M"),
        py::arg("in_off"), py::arg("ph0"), py::arg("to_end"), py::arg("out"), py::arg("out_lens"));
  m.def("resample_tile", []() { return ds2_resample_tile(); });
  m.def("resample_supported", [](int64_t L, int64_t M, int64_t K) {
    return ds2_resample_supported((int)L, (int)M, (int)K) != 0;
  });
  m.def("hist_stats", &hist_stats);
  m.def("hist_nbucket", []() { return ds2_hist_nbucket(); });
  m.def("hist_blocks", [](int64_t n) { return ds2_hist_blocks(n); });
  m.def("nonfinite_watch", &nonfinite_watch);
  m.def("spin", &spin);
  // csrc/waveaug.hip; checked like the entries above by tests/test_waveaug_bindings.py
  auto wa = m.def_submodule("waveaug", "additive-noise augmentation of waveforms (csrc/waveaug.hip)");
  wa.def("plan", &waveaug_plan, py::arg("lens"), py::arg("length"), py::arg("plan"), py::arg("S"), py::arg("p_ppm"),
         py::arg("snr_lo_cdb"), py::arg("snr_hi_cdb"), py::arg("seed_lo"), py::arg("seed_hi"), py::arg("step_lo"),
         py::arg("step_hi"), py::arg("first_utt"));
  wa.def("energy", &waveaug_energy, py::arg("x"), py::arg("lens"), py::arg("plan"), py::arg("data"), py::arg("start"),
         py::arg("length"), py::arg("part"));
  wa.def("coef", &waveaug_coef, py::arg("lens"), py::arg("plan"), py::arg("part"), py::arg("energy"), py::arg("coef"),
         py::arg("S"));
  wa.def("apply", &waveaug_apply, py::arg("x"), py::arg("lens"), py::arg("plan"), py::arg("coef"), py::arg("data"),
         py::arg("start"), py::arg("length"), py::arg("out"));
  wa.def("segment", []() { return ds2_waveaug_segment(); });
  // csrc/speed.hip; checked like the entries above by tests/test_speed_bindings.py
  auto sp = m.def_submodule("speed", "speed perturbation of waveforms (csrc/speed.hip)");
  sp.def("plan", &speed_plan, py::arg("lens"), py::arg("min_out"), py::arg("plan"), py::arg("S"), py::arg("max_out"),
         py::arg("vtab"), py::arg("seed_lo"), py::arg("seed_hi"), py::arg("step_lo"), py::arg("step_hi"),
         py::arg("first_utt"));
  sp.def("apply", &speed_apply, py::arg("x"), py::arg("lens"), py::arg("plan"), py::arg("h"), py::arg("vtab"),
         py::arg("out"), py::arg("out_lens"), py::arg("tight"));
  sp.def("tile", []() { return ds2_speed_tile(); });
  sp.def("supported", [](std::vector<int64_t> vtab, int64_t h_words) {
    if (vtab.empty() || vtab.size() % 5 != 0 || vtab.size() > 40) return false;
    DS2SpeedTable t{};
    t.V = (int)(vtab.size() / 5);
    for (size_t i = 0; i < vtab.size(); ++i) {
      if (vtab[i] < 0 || vtab[i] >= (1LL << 31)) return false;
      (i % 5 == 0 ? t.pct : i % 5 == 1 ? t.L : i % 5 == 2 ? t.M : i % 5 == 3 ? t.K : t.off)[i / 5] = (int)vtab[i];
    }
    return ds2_speed_supported(&t, h_words) != 0;
  }, py::arg("vtab"), py::arg("h_words"));
}

