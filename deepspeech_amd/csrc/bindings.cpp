// Python bindings of the deepspeech_amd gfx950 kernels (module deepspeech_amd._C).
//
// The .hip translation units expose plain extern "C" launchers that take raw pointers
// and a hipStream_t; this file validates tensors (device, dtype, contiguity, shapes)
// and launches on PyTorch's current HIP stream, so every op composes with torch streams
// and can be captured into a hipGraph.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "api.h"

namespace {

using OptT = c10::optional<at::Tensor>;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "deepspeech_amd kernel launch failed in ", what, " (code ", rc, ")");
}
// the conv front-end's launchers: the message also says what was refused
void check_conv(int rc, const char* what) {
  const char* why = ds2_conv_status_str(rc);
  TORCH_CHECK(rc == 0, "deepspeech_amd kernel launch failed in ", what, " (code ", rc, ")", why ? ": " : "",
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

void need_gpu(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

template <typename T>
T* ptr_or_null(const OptT& t, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  need_gpu(*t, name);
  return reinterpret_cast<T*>(t->data_ptr());
}

int is_bf16(const at::Tensor& t) {
  if (t.scalar_type() == at::kBFloat16) return 1;
  TORCH_CHECK(t.scalar_type() == at::kFloat, "expected float32 or bfloat16 tensor");
  return 0;
}

void need_bf16(const at::Tensor& t, const char* name) {
  need_gpu(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
}
void need_f32(const at::Tensor& t, const char* name, int64_t numel) {
  need_gpu(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.numel() >= numel, name, " too small (", t.numel(), " < ", numel, ")");
}
int* need_i32(const at::Tensor& t, const char* name, int64_t numel) {
  need_gpu(t, name);
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(t.numel() >= numel, name, " too small (", t.numel(), " < ", numel, ")");
  return t.data_ptr<int>();
}

// --------------------------------------------------------------------------- RNN
// Every recurrence descriptor (csrc/api.h) is filled the same way: the geometry from the 12
// integers of ops/rnn.py _geom, the buffers Python allocates stacked [ndir, ...] through
// dir_ptrs, the bias partials through bias_parts. U and bh are separate arena parameters and
// come as per-direction pairs (pair_ptrs).
template <typename D>
D rnn_desc(const std::vector<int64_t>& g, const at::Tensor& lens, const at::Tensor& err, int64_t timeout) {
  TORCH_CHECK(g.size() == 12, "recurrence geometry: the 12 integers of ops/rnn.py _geom");
  D d{};
  static_cast<DS2RnnGeom&>(d) = DS2RnnGeom{(int)g[0], (int)g[1], (int)g[2], (int)g[3], (int)g[4],  (int)g[5],
                                           (int)g[6], (int)g[7], (int)g[8], (int)g[9], (int)g[10], (int)g[11]};
  TORCH_CHECK(d.T >= 0 && d.N >= 1 && d.NP >= d.N && d.BG >= 1 && d.H >= 32 && d.H % 32 == 0 && d.steps <= d.T &&
                  (d.ndir == 1 || d.ndir == 2) && (d.cell == 0 || d.cell == 1),
              "recurrence geometry out of range");
  d.lens = need_i32(lens, "lens", d.N);
  TORCH_CHECK(lens.numel() == d.N, "lens must be int32 [N]");
  d.err = reinterpret_cast<unsigned*>(need_i32(err, "err", 1));
  d.timeout = timeout;
  return d;
}

// The direction pointers of a stacked buffer [ndir, per_dir elements]: on the device, of the
// given dtype, contiguous, of exactly that size (at_least: or larger, for state a longer
// launch saved; the directions then lie numel / ndir apart). Directions past ndir stay null.
template <typename P>
void dir_ptrs(P* (&out)[2], const at::Tensor& t, const char* name, at::ScalarType dtype, int64_t ndir,
              int64_t per_dir, bool at_least = false) {
  need_gpu(t, name);
  const int64_t n = t.numel();
  TORCH_CHECK(t.scalar_type() == dtype && (at_least ? n >= ndir * per_dir && n % ndir == 0 : n == ndir * per_dir),
              name, " must be ", dtype, " [", ndir, ", ", per_dir, at_least ? " or more]" : "]", ", got ", n, " of ",
              t.scalar_type());
  char* base = static_cast<char*>(t.data_ptr());
  for (int i = 0; i < 2; ++i) out[i] = i < ndir ? reinterpret_cast<P*>(base + i * (n / ndir) * t.element_size()) : nullptr;
}
template <typename P>
void dir_ptrs(P* (&out)[2], const OptT& t, const char* name, at::ScalarType dtype, int64_t ndir, int64_t per_dir,
              bool at_least = false) {
  out[0] = out[1] = nullptr;
  if (t.has_value() && t->defined()) dir_ptrs(out, *t, name, dtype, ndir, per_dir, at_least);
}

// Bias-gradient partials fp32 [k, ndir, BG, G*H] (k = 0 the input bias, k = 1 the GRU's
// recurrent bias) or none: per_dir = BG * G * H
void bias_parts(float* (&bx)[2], float* (&bh)[2], const OptT& parts, int64_t k, int64_t ndir, int64_t per_dir) {
  float* by_k[2];
  dir_ptrs(by_k, parts, "bias partials", at::kFloat, k, ndir * per_dir);
  for (int i = 0; i < 2; ++i) {
    bx[i] = (by_k[0] && i < ndir) ? by_k[0] + i * per_dir : nullptr;
    bh[i] = (by_k[1] && i < ndir) ? by_k[1] + i * per_dir : nullptr;
  }
}

template <typename P>
void pair_ptrs(P* (&out)[2], const OptT& f, const OptT& b, const char* name, int ndir, bool required) {
  out[0] = ptr_or_null<P>(f, name);
  out[1] = ndir == 2 ? ptr_or_null<P>(b, name) : nullptr;
  TORCH_CHECK(!required || (out[0] && (ndir == 1 || out[1])), name, ": a direction's tensor is missing");
}

// bf16 [T, N, row] activations / gradients beside the recurrence: gx, dy, dgx
void* need_seq(const at::Tensor& t, const char* name, const DS2RnnGeom& d, int64_t row, bool exact = false) {
  need_bf16(t, name);
  const int64_t n = (int64_t)d.T * d.N * row;
  TORCH_CHECK(exact ? t.numel() == n : t.numel() >= n, name, " must be bf16 [T, N, ", row, "]");
  return t.data_ptr();
}

// ---- generation 1 (csrc/rnn_persistent.hip): 16*mt-row tiles, one flag word per workgroup
template <typename D>
D rnn1_desc(const std::vector<int64_t>& g, const at::Tensor& lens, const at::Tensor& err, int64_t timeout, int64_t nw,
            int64_t mt, bool persistent, const at::Tensor& flags, const OptT& stamps) {
  D d = rnn_desc<D>(g, lens, err, timeout);
  TORCH_CHECK(d.NP == d.BG * 16 * mt, "NP must equal BG*16*mt");
  d.S = d.H / 16; d.nw = (int)nw; d.mt = (int)mt; d.persistent = persistent ? 1 : 0;
  d.flags = reinterpret_cast<unsigned*>(need_i32(flags, "flags", (int64_t)d.ndir * d.BG * d.S));
  d.stamps = ptr_or_null<unsigned long long>(stamps, "stamps");
  return d;
}

void rnn_fwd(std::vector<int64_t> geom, int64_t nw, int64_t mt, bool persistent, at::Tensor gx, at::Tensor lens,
             OptT U_f, OptT U_b, OptT bh_f, OptT bh_b, at::Tensor y, at::Tensor hx, at::Tensor hs, OptT gates,
             at::Tensor flags, at::Tensor err, int64_t timeout, OptT stamps) {
  DS2RnnFwd d = rnn1_desc<DS2RnnFwd>(geom, lens, err, timeout, nw, mt, persistent, flags, stamps);
  const int64_t hsz = (int64_t)(d.steps + 1) * d.NP * d.H;
  d.gx = need_seq(gx, "gx", d, d.gstride);
  pair_ptrs(d.U, U_f, U_b, "U", d.ndir, true);
  pair_ptrs(d.bh, bh_f, bh_b, "bh", d.ndir, false);
  dir_ptrs(d.y, y, "y", at::kBFloat16, d.ndir, (int64_t)d.T * d.N * d.H);
  dir_ptrs(d.hx, hx, "hx", at::kBFloat16, d.ndir, hsz, true);
  dir_ptrs(d.hsave, hs, "hs", at::kFloat, d.ndir, hsz, true);
  dir_ptrs(d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4, true);
  TORCH_CHECK(d.cell == 0 || d.gates[0], "GRU needs gate buffers");
  check(d.stamps ? ds2_rnn_fwd_stamps(&d, cur_stream()) : ds2_rnn_fwd(&d, cur_stream()), "rnn_fwd");
}

void rnn_bwd(std::vector<int64_t> geom, int64_t nw, int64_t mt, bool persistent, at::Tensor dy, at::Tensor lens,
             OptT U_f, OptT U_b, at::Tensor hs, OptT gates, at::Tensor dgh, at::Tensor dgx, OptT carry, OptT parts,
             double dgx_scale, at::Tensor flags, at::Tensor err, int64_t timeout, OptT stamps) {
  DS2RnnBwd d = rnn1_desc<DS2RnnBwd>(geom, lens, err, timeout, nw, mt, persistent, flags, stamps);
  const int64_t G = d.cell == 1 ? 3 : 1;
  d.dy = need_seq(dy, "dy", d, d.H);
  d.dgx = need_seq(dgx, "dgx", d, d.gstride);
  d.dgx_scale = (float)dgx_scale;
  pair_ptrs(d.U, U_f, U_b, "U", d.ndir, true);
  dir_ptrs(d.hsave, hs, "hs", at::kFloat, d.ndir, (int64_t)(d.steps + 1) * d.NP * d.H, true);
  dir_ptrs(d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4, true);
  TORCH_CHECK(d.cell == 0 || d.gates[0], "GRU needs gate buffers");
  dir_ptrs(d.dgh, dgh, "dgh", at::kBFloat16, d.ndir, (int64_t)d.steps * d.NP * G * d.H);
  dir_ptrs(d.carry, carry, "carry", at::kFloat, d.ndir, (int64_t)d.NP * d.H);
  bias_parts(d.dbx_part, d.dbh_part, parts, d.cell == 1 ? 2 : 1, d.ndir, d.BG * G * d.H);
  check(d.stamps ? ds2_rnn_bwd_stamps(&d, cur_stream()) : ds2_rnn_bwd(&d, cur_stream()), "rnn_bwd");
}

// ---- XCD-local groups of R rows (csrc/rnn_xcd.hip: 32 units per census word, R <= 16;
// csrc/rnn_fp8.hip: 64 units, R <= 8)
template <typename D>
D rnnx_desc(const std::vector<int64_t>& g, const at::Tensor& lens, const at::Tensor& err, int64_t timeout,
            const at::Tensor& census, int units, int max_rows) {
  D d = rnn_desc<D>(g, lens, err, timeout);
  TORCH_CHECK(d.NP == d.BG * d.R && d.R >= 1 && d.R <= max_rows, "bad row tiling");
  d.census = reinterpret_cast<unsigned*>(need_i32(census, "census", (int64_t)d.ndir * d.BG * (d.H / units)));
  return d;
}

void rnnx_fwd(std::vector<int64_t> geom, at::Tensor gx, at::Tensor lens, OptT U_f, OptT U_b, OptT bh_f, OptT bh_b,
              OptT y, OptT ysum, at::Tensor hx, at::Tensor hs, OptT gates, at::Tensor census, at::Tensor err,
              int64_t timeout, OptT stamps) {
  DS2RnnX d = rnnx_desc<DS2RnnX>(geom, lens, err, timeout, census, 32, 16);
  const int64_t hsz = (int64_t)(d.steps + 1) * d.NP * d.H;
  d.gx = need_seq(gx, "gx", d, d.gstride);
  d.dgx_scale = 1.f;
  pair_ptrs(d.U, U_f, U_b, "U", d.ndir, true);
  pair_ptrs(d.bh, bh_f, bh_b, "bh", d.ndir, false);
  // the fused direction sum (generations 4 - 6) is both directions' output
  if (ysum.has_value()) d.y[0] = d.y[1] = d.ysum = need_seq(*ysum, "ysum", d, d.H);
  else dir_ptrs(d.y, y, "y", at::kBFloat16, d.ndir, (int64_t)d.T * d.N * d.H);
  TORCH_CHECK(d.y[0], "rnnx_fwd needs y or ysum");
  dir_ptrs(d.ex, hx, "hx", at::kBFloat16, d.ndir, hsz, true);
  dir_ptrs(d.hsave, hs, "hs", at::kFloat, d.ndir, hsz, true);
  dir_ptrs(d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4, true);
  TORCH_CHECK(d.cell == 0 || d.gates[0], "GRU needs gate buffers");
  d.stamps = ptr_or_null<unsigned long long>(stamps, "stamps");
  check(ds2_rnnx_fwd(&d, cur_stream()), "rnnx_fwd");
}

// reduce-scatter BPTT (generation 3): dgh is a plain output, the exchange is the fp32 ring
// [ndir, ds2_rnnx_ring_floats], sentinel-filled
void rnnx_bwd(std::vector<int64_t> geom, at::Tensor dy, at::Tensor lens, OptT U_f, OptT U_b, at::Tensor hs, OptT gates,
              at::Tensor dgh, at::Tensor dgx, OptT parts, double dgx_scale, at::Tensor census, at::Tensor err,
              at::Tensor ring, int64_t timeout, OptT stamps) {
  DS2RnnX d = rnnx_desc<DS2RnnX>(geom, lens, err, timeout, census, 32, 16);
  const int64_t G = d.cell == 1 ? 3 : 1;
  d.gx = need_seq(dy, "dy", d, d.H);
  d.dgx = need_seq(dgx, "dgx", d, d.gstride);
  d.dgx_scale = (float)dgx_scale;
  pair_ptrs(d.U, U_f, U_b, "U", d.ndir, true);
  dir_ptrs(d.hsave, hs, "hs", at::kFloat, d.ndir, (int64_t)(d.steps + 1) * d.NP * d.H, true);
  dir_ptrs(d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4, true);
  TORCH_CHECK(d.cell == 0 || d.gates[0], "GRU needs gate buffers");
  dir_ptrs(d.ex, dgh, "dgh", at::kBFloat16, d.ndir, (int64_t)d.steps * d.NP * G * d.H, true);
  dir_ptrs(d.ring, ring, "ring", at::kFloat, d.ndir, ds2_rnnx_ring_floats(d.H, d.BG, d.R), true);
  bias_parts(d.dbx_part, d.dbh_part, parts, d.cell == 1 ? 2 : 1, d.ndir, d.BG * G * d.H);
  d.stamps = ptr_or_null<unsigned long long>(stamps, "stamps");
  check(ds2_rnnx_bwd_rs(&d, cur_stream()), "rnnx_bwd_rs");
}

// csrc/rnn_fp8.hip: GRU forward with e4m3 U8 [ndir, 3H, H] (per-tensor power-of-two scale, uexp =
// E8M0 exponent per direction on the device) and an e4m3 hidden-state exchange hq [ndir][steps+1]
// [NP][H] (slot 0 = e4m3 h0, slots 1.. 0xFF); saves hs / gates / bf16 hx like rnnx_fwd.
void rnnf8_fwd(std::vector<int64_t> geom, at::Tensor gx, at::Tensor lens, at::Tensor U8, at::Tensor uexp, OptT bh_f,
               OptT bh_b, at::Tensor y, at::Tensor hq, at::Tensor hx, at::Tensor hs, at::Tensor gates,
               at::Tensor census, at::Tensor err, int64_t timeout) {
  DS2RnnF8 d = rnnx_desc<DS2RnnF8>(geom, lens, err, timeout, census, 64, 8);
  TORCH_CHECK(ds2_rnnf8_supported(d.H, d.N, d.ndir), "rnnf8: unsupported geometry");
  TORCH_CHECK(d.steps >= 1 && d.BG * d.ndir <= 8 && d.gstride >= d.ndir * 3 * d.H, "rnnf8: plan");
  const int64_t hsz = (int64_t)(d.steps + 1) * d.NP * d.H;
  d.gx = need_seq(gx, "gx", d, d.gstride);
  dir_ptrs(d.U8, U8, "U8", at::kByte, d.ndir, (int64_t)3 * d.H * d.H);
  d.uexp = need_i32(uexp, "uexp", d.ndir);
  pair_ptrs(d.bh, bh_f, bh_b, "bh", d.ndir, false);
  dir_ptrs(d.y, y, "y", at::kBFloat16, d.ndir, (int64_t)d.T * d.N * d.H);
  dir_ptrs(d.hq, hq, "hq", at::kByte, d.ndir, hsz);
  dir_ptrs(d.hx, hx, "hx", at::kBFloat16, d.ndir, hsz);
  dir_ptrs(d.hsave, hs, "hs", at::kFloat, d.ndir, hsz);
  dir_ptrs(d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4);
  check(ds2_rnnf8_fwd(&d, cur_stream()), "rnnf8_fwd");
}

// csrc/rnn_fp8.hip fp8 GRU BPTT: U8T [ndir, H, 3H] e4m3 U^T (uexp per direction), saved fp32
// h / gates of the forward, tagged-bf16 reduce-scatter ring [ndir, ring_words] filled 0xFF..
void rnnf8_bwd(std::vector<int64_t> geom, at::Tensor dy, at::Tensor lens, at::Tensor U8T, at::Tensor uexp,
               at::Tensor hs, at::Tensor gates, at::Tensor dgh, at::Tensor dgx, OptT parts, double dgx_scale,
               at::Tensor census, at::Tensor err, at::Tensor ring, int64_t timeout) {
  DS2RnnF8B d = rnnx_desc<DS2RnnF8B>(geom, lens, err, timeout, census, 64, 8);
  TORCH_CHECK(ds2_rnnf8_bwd_supported(d.H, d.N, d.ndir), "rnnf8_bwd: unsupported geometry");
  TORCH_CHECK(d.steps >= 1 && d.BG * d.ndir <= 8 && d.gstride >= d.ndir * 3 * d.H, "rnnf8_bwd: plan");
  d.dy = need_seq(dy, "dy", d, d.H, true);
  d.dgx = need_seq(dgx, "dgx", d, d.gstride, true);
  d.dgx_scale = (float)dgx_scale;
  dir_ptrs(d.U8T, U8T, "U8T", at::kByte, d.ndir, (int64_t)3 * d.H * d.H);
  d.uexp = need_i32(uexp, "uexp", d.ndir);
  dir_ptrs(d.hsave, hs, "hs", at::kFloat, d.ndir, (int64_t)(d.steps + 1) * d.NP * d.H, true);
  dir_ptrs(d.gates, gates, "gates", at::kFloat, d.ndir, (int64_t)d.steps * d.NP * d.H * 4, true);
  dir_ptrs(d.dgh, dgh, "dgh", at::kBFloat16, d.ndir, (int64_t)d.steps * d.NP * 3 * d.H);
  dir_ptrs(d.ring, ring, "ring", at::kInt, d.ndir, ds2_rnnf8_ring_words(d.H, d.BG, d.R), true);
  bias_parts(d.dbx_part, d.dbh_part, parts, 2, d.ndir, (int64_t)d.BG * 3 * d.H);
  check(ds2_rnnf8_bwd(&d, cur_stream()), "rnnf8_bwd");
}

int64_t rnn_kpw(int64_t H, int64_t G, int64_t nw, bool fwd) { return ds2_rnn_kpw((int)H, (int)G, (int)nw, fwd ? 1 : 0); }

// e4m3 copy of a bf16 tensor scaled by ONE power of two (amax / 2^e <= 448); uexp[0] = 127 + e
void fp8_quant_pow2(at::Tensor x, at::Tensor q, at::Tensor uexp, at::Tensor amax) {
  need_gpu(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous(), "x must be contiguous bf16");
  TORCH_CHECK(q.scalar_type() == at::kByte && q.is_contiguous() && q.numel() == x.numel(), "q must be uint8 like x");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(q.data_ptr()) & 7) == 0,
              "x 16-B / q 8-B aligned");
  TORCH_CHECK(uexp.scalar_type() == at::kInt && uexp.numel() >= 1 && amax.scalar_type() == at::kInt && amax.numel() >= 1,
              "uexp / amax int32 device words");
  check(ds2_fp8_quant_pow2(x.data_ptr(), x.numel(), q.data_ptr(), uexp.data_ptr<int>(),
                           reinterpret_cast<unsigned*>(amax.data_ptr<int>()), cur_stream()),
        "fp8_quant_pow2");
}

// csrc/rnn_fp8.hip: e4m3 copies of U_f (and U_b) [rows][cols] bf16 with one power-of-two scale per
// direction: q [ndir, rows, cols] and / or qt [ndir, cols, rows] uint8, uexp int32 [>= ndir],
// part fp32 [>= ndir * 256] scratch
void fp8_quant_u(at::Tensor U_f, OptT U_b, OptT q, OptT qt, at::Tensor uexp, at::Tensor part) {
  const int ndir = U_b.has_value() ? 2 : 1;
  for (const at::Tensor* u : {&U_f, U_b.has_value() ? &*U_b : &U_f}) {
    need_gpu(*u, "U");
    TORCH_CHECK(u->scalar_type() == at::kBFloat16 && u->is_contiguous() && u->dim() == 2 && u->sizes() == U_f.sizes(),
                "U must be contiguous bf16 2-D, both directions alike");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(u->data_ptr()) & 15) == 0, "U 16-B aligned");
  }
  const int64_t rows = U_f.size(0), cols = U_f.size(1);
  TORCH_CHECK(rows % 64 == 0 && cols % 64 == 0, "fp8_quant_u: rows and cols multiples of 64");
  TORCH_CHECK(q.has_value() || qt.has_value(), "fp8_quant_u: q or qt");
  void* pq[2] = {nullptr, nullptr};
  void* pqt[2] = {nullptr, nullptr};
  if (q) {
    TORCH_CHECK(q->scalar_type() == at::kByte && q->is_contiguous() && q->numel() == ndir * rows * cols, "q uint8 [ndir, rows, cols]");
    for (int d = 0; d < ndir; ++d) pq[d] = static_cast<unsigned char*>(q->data_ptr()) + d * rows * cols;
  }
  if (qt) {
    TORCH_CHECK(qt->scalar_type() == at::kByte && qt->is_contiguous() && qt->numel() == ndir * rows * cols &&
                    (reinterpret_cast<uintptr_t>(qt->data_ptr()) & 15) == 0, "qt uint8 [ndir, cols, rows], 16-B aligned");
    for (int d = 0; d < ndir; ++d) pqt[d] = static_cast<unsigned char*>(qt->data_ptr()) + d * rows * cols;
  }
  TORCH_CHECK(uexp.scalar_type() == at::kInt && uexp.numel() >= ndir, "uexp int32 [>= ndir]");
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.numel() >= ndir * 256, "part fp32 [>= ndir * 256]");
  const void* px[2] = {U_f.data_ptr(), U_b.has_value() ? U_b->data_ptr() : U_f.data_ptr()};
  check(ds2_fp8_quant_u(ndir, px, (int)rows, (int)cols, pq, pqt, uexp.data_ptr<int>(), part.data_ptr<float>(),
                        cur_stream()), "fp8_quant_u");
}

// csrc/rnn_fp8.hip: transposed e4m3 copy q [cols][rows] of a bf16 [rows][cols] tensor scaled by
// one power of two (the fp8 BPTT's U^T); uexp[0] = 127 + e
void fp8_quant_pow2_t(at::Tensor x, at::Tensor q, at::Tensor uexp, at::Tensor amax) {
  need_gpu(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous() && x.dim() == 2, "x must be contiguous bf16 2-D");
  TORCH_CHECK(q.scalar_type() == at::kByte && q.is_contiguous() && q.numel() == x.numel(), "q must be uint8 like x");
  TORCH_CHECK(uexp.scalar_type() == at::kInt && uexp.numel() >= 1 && amax.scalar_type() == at::kInt && amax.numel() >= 1,
              "uexp / amax int32 device words");
  check(ds2_fp8_quant_pow2_t(x.data_ptr(), (int)x.size(0), (int)x.size(1), q.data_ptr(), uexp.data_ptr<int>(),
                             reinterpret_cast<unsigned*>(amax.data_ptr<int>()), cur_stream()),
        "fp8_quant_pow2_t");
}

// --------------------------------------------------------------------------- CTC
int64_t ctc_ws_floats(int64_t T, int64_t N, int64_t Lmax) { return ds2_ctc_ws_floats((int)T, (int)N, (int)Lmax); }

void ctc_fused(at::Tensor logits, at::Tensor lens, at::Tensor labels, at::Tensor label_lens, at::Tensor loss,
               at::Tensor grad, at::Tensor ws, int64_t blank, bool zero_inf) {
  need_gpu(logits, "logits");
  need_gpu(labels, "labels");
  need_gpu(ws, "ws");
  TORCH_CHECK(logits.dim() == 3, "logits must be [T, N, K]");
  TORCH_CHECK(grad.scalar_type() == logits.scalar_type() && grad.sizes() == logits.sizes(), "grad mismatch");
  const int T = (int)logits.size(0), N = (int)logits.size(1), K = (int)logits.size(2);
  const int Lmax = (int)labels.size(1);
  TORCH_CHECK(labels.size(0) == N && lens.numel() == N && label_lens.numel() == N, "batch mismatch");
  TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.numel() >= ds2_ctc_ws_floats(T, N, Lmax), "CTC workspace too small");
  check(ds2_ctc_fused(logits.data_ptr(), is_bf16(logits), lens.data_ptr<int>(), labels.data_ptr<int>(),
                      label_lens.data_ptr<int>(), loss.data_ptr<float>(), grad.data_ptr(), ws.data_ptr<float>(), T,
                      N, K, Lmax, (int)blank, zero_inf ? 1 : 0, cur_stream()),
        "ctc_fused");
}

// --------------------------------------------------------------------------- CTC forced alignment
int64_t ctc_align_ws_bytes(int64_t T, int64_t N, int64_t Lmax) {
  return ds2_ctc_align_ws_bytes((int)T, (int)N, (int)Lmax);
}

// emissions [T, N, K] (fp32 / bf16) -> path [N, T] int32, tok_start / tok_end [N, Lmax] int32,
// tok_score [N, Lmax] fp32, score [N] fp32 (csrc/align.hip)
void ctc_align(at::Tensor em, at::Tensor lens, at::Tensor labels, at::Tensor label_lens, at::Tensor path,
               at::Tensor tok_start, at::Tensor tok_end, at::Tensor tok_score, at::Tensor score, at::Tensor ws,
               int64_t blank, bool log_probs) {
  need_gpu(em, "emissions");
  need_gpu(labels, "labels");
  need_gpu(ws, "ws");
  TORCH_CHECK(em.dim() == 3, "emissions must be [T, N, K]");
  const int T = (int)em.size(0), N = (int)em.size(1), K = (int)em.size(2);
  TORCH_CHECK(labels.dim() == 2 && labels.scalar_type() == at::kInt, "labels must be int32 [N, Lmax]");
  const int Lmax = (int)labels.size(1);
  TORCH_CHECK(K <= 32, "ctc_align: K <= 32 classes");
  TORCH_CHECK(Lmax >= 1 && 2 * (int64_t)Lmax + 1 <= 2048, "ctc_align: 1 <= Lmax and 2*Lmax+1 <= 2048 lattice states");
  TORCH_CHECK(blank >= 0 && blank < K, "ctc_align: 0 <= blank < K");
  TORCH_CHECK(labels.size(0) == N && lens.numel() == N && label_lens.numel() == N, "batch mismatch");
  for (const at::Tensor* t : {&lens, &label_lens}) {
    need_gpu(*t, "lens / label_lens");
    TORCH_CHECK(t->scalar_type() == at::kInt, "lens / label_lens must be int32");
  }
  for (const at::Tensor* t : {&path, &tok_start, &tok_end}) {
    need_gpu(*t, "path / tok_start / tok_end");
    TORCH_CHECK(t->scalar_type() == at::kInt, "path / tok_start / tok_end must be int32");
  }
  need_gpu(tok_score, "tok_score");
  need_gpu(score, "score");
  TORCH_CHECK(tok_score.scalar_type() == at::kFloat && score.scalar_type() == at::kFloat, "scores must be fp32");
  TORCH_CHECK(path.numel() == (int64_t)N * T, "path must be [N, T]");
  TORCH_CHECK(tok_start.numel() == (int64_t)N * Lmax && tok_end.numel() == (int64_t)N * Lmax &&
                  tok_score.numel() == (int64_t)N * Lmax, "tok_start / tok_end / tok_score must be [N, Lmax]");
  TORCH_CHECK(score.numel() == N, "score must be [N]");
  TORCH_CHECK(ws.scalar_type() == at::kByte && ws.numel() >= ds2_ctc_align_ws_bytes(T, N, Lmax) &&
                  (reinterpret_cast<uintptr_t>(ws.data_ptr()) & 15) == 0,
              "alignment workspace too small or not 16-B aligned");
  check(ds2_ctc_align(em.data_ptr(), is_bf16(em), log_probs ? 1 : 0, lens.data_ptr<int>(), labels.data_ptr<int>(),
                      label_lens.data_ptr<int>(), path.data_ptr<int>(), tok_start.data_ptr<int>(),
                      tok_end.data_ptr<int>(), tok_score.data_ptr<float>(), score.data_ptr<float>(), ws.data_ptr(), T,
                      N, K, Lmax, (int)blank, cur_stream()),
        "ctc_align");
}

// --------------------------------------------------------------------------- BN
int64_t bn_chunks(int64_t N, int64_t T, int64_t F) { return ds2_bn_chunks((int)N, (int)T, (int)F); }

void bn_stats(at::Tensor y, at::Tensor part, double eps, at::Tensor mean, at::Tensor invstd, OptT run_mean,
              OptT run_var, double momentum) {
  need_gpu(y, "y");
  TORCH_CHECK(y.dim() == 4, "y must be NCHW");
  const int N = (int)y.size(0), C = (int)y.size(1), T = (int)y.size(2), F = (int)y.size(3);
  const int nb = (int)(part.numel() / (2 * C));
  check(ds2_bn_stats(y.data_ptr(), is_bf16(y), N, C, T, F, part.data_ptr<float>(), nb, (float)eps,
                     mean.data_ptr<float>(), invstd.data_ptr<float>(), ptr_or_null<float>(run_mean, "run_mean"),
                     ptr_or_null<float>(run_var, "run_var"), (float)momentum, cur_stream()),
        "bn_stats");
}

void bn_apply(at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta, at::Tensor out,
              int64_t layout) {
  need_gpu(y, "y");
  need_gpu(out, "out");
  const int N = (int)y.size(0), C = (int)y.size(1), T = (int)y.size(2), F = (int)y.size(3);
  TORCH_CHECK(out.numel() == y.numel(), "out size mismatch");
  check(ds2_bn_apply(y.data_ptr(), is_bf16(y), mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(), out.data_ptr(), is_bf16(out), N, C, T, F,
                     (int)layout, cur_stream()),
        "bn_apply");
}

void bn_bwd(at::Tensor dout, at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta,
            at::Tensor part, at::Tensor dgamma, at::Tensor dbeta, at::Tensor dy, int64_t layout) {
  need_gpu(dout, "dout");
  need_gpu(y, "y");
  need_gpu(dy, "dy");
  const int N = (int)y.size(0), C = (int)y.size(1), T = (int)y.size(2), F = (int)y.size(3);
  const int nb = (int)(part.numel() / (2 * C));
  TORCH_CHECK(dout.numel() == y.numel() && dy.numel() == y.numel(), "size mismatch");
  check(ds2_bn_bwd(dout.data_ptr(), is_bf16(dout), y.data_ptr(), is_bf16(y), mean.data_ptr<float>(),
                   invstd.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(), part.data_ptr<float>(),
                   nb, dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), dy.data_ptr(), is_bf16(dy), N, C, T, F,
                   (int)layout, cur_stream()),
        "bn_bwd");
}

// --------------------------------------------------------------------------- optimizer
// What the Adam + EMA kernels assume of their arrays (csrc/optim.hip: f32x4 accesses of the fp32
// arrays, uint2 stores of the bf16 copy): n elements each, contiguous, fp32 16-B and bf16 8-B aligned
static void adam_arrays_check(const at::Tensor& p, const at::Tensor& g, const at::Tensor& m, const at::Tensor& v,
                              const OptT& ema, const OptT& p16, const OptT& hyper, const char* what) {
  const int64_t n = p.numel();
  const at::Tensor* f32s[4] = {&p, &g, &m, &v};
  const char* names[4] = {"p", "g", "m", "v"};
  for (int i = 0; i < 4; ++i) {
    need_gpu(*f32s[i], names[i]);
    TORCH_CHECK(f32s[i]->scalar_type() == at::kFloat, what, ": fp32 arena expected (", names[i], ")");
    TORCH_CHECK(f32s[i]->numel() == n, what, ": arena size mismatch (", names[i], ")");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(f32s[i]->data_ptr()) % 16 == 0, what, ": ", names[i],
                " must be 16-byte aligned");
  }
  if (ema.has_value() && ema->defined()) {
    need_gpu(*ema, "ema");
    TORCH_CHECK(ema->scalar_type() == at::kFloat && ema->numel() == n, what, ": ema must be fp32 of p's size");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(ema->data_ptr()) % 16 == 0, what, ": ema must be 16-byte aligned");
  }
  if (p16.has_value() && p16->defined()) {
    need_gpu(*p16, "p16");
    TORCH_CHECK(p16->scalar_type() == at::kBFloat16 && p16->numel() == n, what, ": p16 must be bf16 of p's size");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p16->data_ptr()) % 8 == 0, what, ": p16 must be 8-byte aligned");
  }
  if (hyper.has_value() && hyper->defined()) {
    need_gpu(*hyper, "hyper");
    TORCH_CHECK(hyper->scalar_type() == at::kFloat && hyper->numel() >= 2, what, ": hyper must be fp32 {lr_t, ema_keep}");
  }
}

// The clipping state the CLIP kernels read (csrc/optim.hip): ds2_clip_state_words() fp32 words on the GPU
static void clip_state_check(const OptT& clip, const char* what) {
  if (clip.has_value() && clip->defined()) {
    need_gpu(*clip, "clip");
    TORCH_CHECK(clip->scalar_type() == at::kFloat && clip->numel() >= ds2_clip_state_words() && clip->is_contiguous(),
                what, ": clip must be the contiguous fp32 clipping state");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(clip->data_ptr()) % 4 == 0, what, ": clip must be 4-byte aligned");
  }
}

void adam_ema(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, OptT ema, OptT p16, double lr_t, double b1,
              double b2, double eps, double gscale, double ema_keep, OptT skip, int64_t max_grid, OptT hyper,
              int64_t lds_reserve, OptT clip) {
  TORCH_CHECK(lds_reserve >= 0 && lds_reserve <= 65536, "adam_ema: lds_reserve in [0, 64 KB]");
  adam_arrays_check(p, g, m, v, ema, p16, hyper, "adam_ema");
  clip_state_check(clip, "adam_ema");
  if (skip.has_value() && skip->defined()) {
    need_gpu(*skip, "skip");
    TORCH_CHECK(skip->scalar_type() == at::kInt && skip->numel() >= 1, "adam_ema: skip must be an int32 flag");
  }
  const long long n = p.numel();
  check(ds2_adam_ema(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                     ptr_or_null<float>(ema, "ema"), ptr_or_null<void>(p16, "p16"), n, (float)lr_t, (float)b1,
                     (float)b2, (float)eps, (float)gscale, (float)ema_keep, ptr_or_null<const int>(skip, "skip"),
                     (int)max_grid, ptr_or_null<const float>(hyper, "hyper"), (int)lds_reserve,
                     ptr_or_null<const float>(clip, "clip"), cur_stream()),
        "adam_ema");
}

// Adam + EMA over several (lo, hi) element ranges of whole-arena buffers in one launch
void adam_ema_ranges(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, OptT ema, OptT p16,
                     std::vector<int64_t> lohi, double lr_t, double b1, double b2, double eps, double gscale,
                     double ema_keep, OptT hyper, OptT clip) {
  adam_arrays_check(p, g, m, v, ema, p16, hyper, "adam_ema_ranges");
  clip_state_check(clip, "adam_ema_ranges");
  const long long n = p.numel();
  TORCH_CHECK(lohi.size() % 2 == 0, "adam_ema_ranges: (lo, hi) pairs");
  for (size_t i = 0; i < lohi.size(); ++i) TORCH_CHECK(lohi[i] >= 0 && lohi[i] <= n, "adam_ema_ranges: range");
  // two ranges sharing an element would be updated by two threads at once
  std::vector<std::pair<int64_t, int64_t>> sorted;
  for (size_t i = 0; i + 1 < lohi.size(); i += 2)
    if (lohi[i + 1] > lohi[i]) sorted.emplace_back(lohi[i], lohi[i + 1]);
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 1; i < sorted.size(); ++i)
    TORCH_CHECK(sorted[i].first >= sorted[i - 1].second, "adam_ema_ranges: ranges overlap");
  std::vector<long long> r(lohi.begin(), lohi.end());
  check(ds2_adam_ema_ranges(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                            ptr_or_null<float>(ema, "ema"), ptr_or_null<void>(p16, "p16"), r.data(),
                            (int)(r.size() / 2), (float)lr_t, (float)b1, (float)b2, (float)eps, (float)gscale,
                            (float)ema_keep, ptr_or_null<const float>(hyper, "hyper"),
                            ptr_or_null<const float>(clip, "clip"), cur_stream()),
        "adam_ema_ranges");
}

int64_t grad_norm_blocks(int64_t n) { return ds2_grad_norm_blocks(n); }

void grad_norm(at::Tensor g, double gscale, at::Tensor part, at::Tensor bad) {
  need_gpu(g, "g");
  need_gpu(part, "part");
  need_gpu(bad, "bad");
  TORCH_CHECK(g.scalar_type() == at::kFloat, "grad_norm: fp32 gradients");
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.numel() >= 1, "grad_norm: part must be a non-empty fp32 tensor");
  TORCH_CHECK(bad.scalar_type() == at::kInt && bad.numel() == 1, "grad_norm: bad must be one int32");
  check(ds2_grad_norm(g.data_ptr<float>(), g.numel(), (float)gscale, part.data_ptr<float>(), (int)part.numel(),
                      bad.data_ptr<int>(), cur_stream()),
        "grad_norm");
}

int64_t grad_sumsq_segment() { return ds2_grad_sumsq_segment(); }

// part[ceil(n / segment)] = fixed-order partial sums of (fl32(g gscale))^2, one per segment of g.
// nontemporal (the default, as measured: profiles/clip.md) only changes the load instruction, never a partial.
void grad_sumsq(at::Tensor g, double gscale, at::Tensor part, int64_t max_grid, bool nontemporal) {
  need_gpu(g, "g");
  need_gpu(part, "part");
  const int64_t seg = ds2_grad_sumsq_segment();
  TORCH_CHECK(g.scalar_type() == at::kFloat, "grad_sumsq: fp32 gradients");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0, "grad_sumsq: g must be 16-byte aligned");
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.numel() == (g.numel() + seg - 1) / seg,
              "grad_sumsq: part must hold one fp32 per segment of g");
  TORCH_CHECK(max_grid >= 0 && max_grid <= 65535, "grad_sumsq: max_grid in [0, 65535]");
  check(ds2_grad_sumsq(g.data_ptr<float>(), g.numel(), (float)gscale, part.data_ptr<float>(), (int)max_grid,
                       nontemporal ? 1 : 0, cur_stream()),
        "grad_sumsq");
}

// state = {S, norm, coef | bad, steps, clipped_steps, skipped_steps, spare} from the partials and max_norm
void clip_finalize(at::Tensor part, double max_norm, at::Tensor state) {
  need_gpu(part, "part");
  TORCH_CHECK(part.scalar_type() == at::kFloat, "clip_finalize: fp32 partials");
  TORCH_CHECK(max_norm > 0, "clip_finalize: max_norm must be > 0 (inf: measure only)");
  OptT st = state;
  clip_state_check(st, "clip_finalize");
  check(ds2_clip_finalize(part.data_ptr<float>(), part.numel(), (float)max_norm, state.data_ptr<float>(), cur_stream()),
        "clip_finalize");
}

void cast_bf16(at::Tensor x, at::Tensor y) {
  need_gpu(x, "x");
  need_gpu(y, "y");
  TORCH_CHECK(x.numel() == y.numel(), "size mismatch");
  check(ds2_cast_bf16(x.data_ptr<float>(), y.data_ptr(), x.numel(), cur_stream()), "cast_bf16");
}

// --------------------------------------------------------------------------- conv front-end
// x [N,T,F0] bf16, w [32,1,20,5] bf16 -> y [N,T1,F1,32] bf16, part [grid, 64] f32
void conv1_fwd(at::Tensor x, at::Tensor w, OptT bias, at::Tensor y, at::Tensor part) {
  need_bf16(x, "x"); need_bf16(w, "w"); need_bf16(y, "y");
  TORCH_CHECK(x.dim() == 3 && y.dim() == 4 && y.size(3) == 32 && w.numel() == 32 * 100, "conv1_fwd shapes");
  const int N = (int)x.size(0), T = (int)x.size(1), F0 = (int)x.size(2), T1 = (int)y.size(1), F1 = (int)y.size(2);
  TORCH_CHECK(y.size(0) == N, "conv1_fwd batch");
  need_f32(part, "part", (int64_t)ds2_conv1_fwd_grid(N, T1) * 64);
  check_conv(ds2_conv1_fwd(x.data_ptr(), w.data_ptr(), ptr_or_null<float>(bias, "bias"), y.data_ptr(),
                           part.data_ptr<float>(), N, T, F0, T1, F1, cur_stream()), "conv1_fwd");
}
int64_t conv1_fwd_grid(int64_t N, int64_t T1) { return ds2_conv1_fwd_grid((int)N, (int)T1); }

// per-tile phase stamps of workgroups 0..7 (optional int64 [8 * 16 * 6], tools/conv_timeline.py)
long long* trace_ptr(const OptT& trace) {
  if (!trace) return nullptr;
  TORCH_CHECK(trace->is_cuda() && trace->scalar_type() == at::kLong && trace->numel() >= 8 * 16 * 6 &&
                  trace->is_contiguous(), "trace must be a contiguous cuda int64 tensor of >= 768 elements");
  return reinterpret_cast<long long*>(trace->data_ptr<int64_t>());
}

// x [N,T1,F1,32], w [32,32,10,5] -> y [N,T2,F2,32], part [grid, 64]
void conv2_fwd(at::Tensor x, at::Tensor w, OptT bias, at::Tensor y, at::Tensor part, int64_t grid, OptT trace) {
  need_bf16(x, "x"); need_bf16(w, "w"); need_bf16(y, "y");
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4 && x.size(3) == 32 && y.size(3) == 32 && w.numel() == 32 * 32 * 50,
              "conv2_fwd shapes");
  TORCH_CHECK(grid > 0, "grid");
  need_f32(part, "part", grid * 64);
  check_conv(ds2_conv2_fwd(x.data_ptr(), w.data_ptr(), ptr_or_null<float>(bias, "bias"), y.data_ptr(),
                           part.data_ptr<float>(), (int)grid, (int)x.size(0), (int)x.size(1), (int)x.size(2),
                           (int)y.size(1), (int)y.size(2), trace_ptr(trace), cur_stream()), "conv2_fwd");
}

// dy [N,T2,F2,32], w [32,32,10,5] -> dx [N,T1,F1,32]
// bn (optional, all or none): y1 = conv1's output (dx's shape), conv1's BN mean / invstd / gamma
// / beta, and part [grid * 64] fp32 that receives per-workgroup BN-backward sums over dx
void conv2_dgrad(at::Tensor dy, at::Tensor w, at::Tensor dx, int64_t grid, OptT y1, OptT mean, OptT invstd,
                 OptT gamma, OptT beta, OptT part, OptT trace) {
  need_bf16(dy, "dy"); need_bf16(w, "w"); need_bf16(dx, "dx");
  TORCH_CHECK(dy.dim() == 4 && dx.dim() == 4 && dy.size(3) == 32 && dx.size(3) == 32 && w.numel() == 32 * 32 * 50,
              "conv2_dgrad shapes");
  TORCH_CHECK(grid > 0, "grid");
  DS2Conv2DgradBn bn{};
  const bool with_bn = y1.has_value();
  if (with_bn) {
    TORCH_CHECK(mean && invstd && gamma && beta && part, "conv2_dgrad: the BN arguments come all or none");
    need_bf16(*y1, "y1");
    TORCH_CHECK(y1->sizes() == dx.sizes(), "y1 must have dx's shape");
    need_f32(*mean, "mean", 32); need_f32(*invstd, "invstd", 32); need_f32(*gamma, "gamma", 32);
    need_f32(*beta, "beta", 32); need_f32(*part, "part", grid * 64);
    bn = DS2Conv2DgradBn{y1->data_ptr(), mean->data_ptr<float>(), invstd->data_ptr<float>(),
                         gamma->data_ptr<float>(), beta->data_ptr<float>(), part->data_ptr<float>()};
  }
  check_conv(ds2_conv2_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), (int)grid, (int)dx.size(0), (int)dx.size(1),
                             (int)dx.size(2), (int)dy.size(1), (int)dy.size(2), with_bn ? &bn : nullptr,
                             trace_ptr(trace), cur_stream()),
             "conv2_dgrad");
}

// dy [N,T2,F2,32], x [N,T1,F1,32] -> dw (fp32, 32*32*10*5), part scratch
void conv2_wgrad(at::Tensor dy, at::Tensor x, at::Tensor part, at::Tensor dw, int64_t grid) {
  need_bf16(dy, "dy"); need_bf16(x, "x");
  TORCH_CHECK(grid > 0, "grid");
  need_f32(part, "part", ds2_conv2_wgrad_part_floats((int)grid));
  need_f32(dw, "dw", 32 * 32 * 50);
  check_conv(ds2_conv2_wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr<float>(), (int)grid, dw.data_ptr<float>(),
                             (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)dy.size(1), (int)dy.size(2),
                             cur_stream()), "conv2_wgrad");
}

// dy [N,T1,F1,32], x [N,T,F0] -> dw (fp32, 32*20*5)
// bn (optional, all or none): dy is then dz = dL/d(clip(BN(y1))) and the kernel applies conv1's
// BatchNorm backward (batch statistics mean / invstd, affine gamma / beta, dbeta / dgamma sums)
// while staging it, bitwise as bn_cl_bwd's apply pass
void conv1_wgrad(at::Tensor dy, at::Tensor x, at::Tensor part, at::Tensor dw, int64_t grid, OptT y1, OptT mean,
                 OptT invstd, OptT gamma, OptT beta, OptT dbeta, OptT dgamma) {
  need_bf16(dy, "dy"); need_bf16(x, "x");
  TORCH_CHECK(grid > 0, "grid");
  need_f32(part, "part", ds2_conv1_wgrad_part_floats((int)grid));
  need_f32(dw, "dw", 32 * 100);
  DS2Conv1WgradBn bn{};
  const bool with_bn = y1.has_value();
  if (with_bn) {
    TORCH_CHECK(mean && invstd && gamma && beta && dbeta && dgamma, "conv1_wgrad: the BN arguments come all or none");
    need_bf16(*y1, "y1");
    TORCH_CHECK(y1->sizes() == dy.sizes(), "y1 must have dz's shape");
    for (const OptT* t : {&mean, &invstd, &gamma, &beta, &dbeta, &dgamma}) need_f32(**t, "bn vector", 32);
    bn = DS2Conv1WgradBn{dy.data_ptr(), y1->data_ptr(), mean->data_ptr<float>(), invstd->data_ptr<float>(),
                         gamma->data_ptr<float>(), beta->data_ptr<float>(), dbeta->data_ptr<float>(),
                         dgamma->data_ptr<float>()};
  }
  check_conv(ds2_conv1_wgrad(with_bn ? nullptr : dy.data_ptr(), x.data_ptr(), part.data_ptr<float>(), (int)grid,
                             dw.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)dy.size(1),
                             (int)dy.size(2), with_bn ? &bn : nullptr, cur_stream()), "conv1_wgrad");
}
int64_t conv2_wgrad_part_floats(int64_t grid) { return ds2_conv2_wgrad_part_floats((int)grid); }
int64_t conv1_wgrad_part_floats(int64_t grid) { return ds2_conv1_wgrad_part_floats((int)grid); }

void bn_cl_finalize(at::Tensor part, int64_t nb, double M, double eps, at::Tensor mean, at::Tensor invstd,
                    OptT run_mean, OptT run_var, double momentum) {
  need_f32(part, "part", nb * 64);
  need_f32(mean, "mean", 32); need_f32(invstd, "invstd", 32);
  check_conv(ds2_bn_cl_finalize(part.data_ptr<float>(), (int)nb, M, (float)eps, mean.data_ptr<float>(),
                                invstd.data_ptr<float>(), ptr_or_null<float>(run_mean, "run_mean"),
                                ptr_or_null<float>(run_var, "run_var"), (float)momentum, cur_stream()),
             "bn_cl_finalize");
}

// y [N,T,F,32] -> out [N,T,F,32] (tmaj=0) or [T,N,32*F] (tmaj=1)
void bn_cl_apply(at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta, at::Tensor out,
                 bool tmaj) {
  need_bf16(y, "y"); need_bf16(out, "out");
  TORCH_CHECK(y.dim() == 4 && y.size(3) == 32 && out.numel() == y.numel(), "bn_cl_apply shapes");
  need_f32(mean, "mean", 32); need_f32(invstd, "invstd", 32); need_f32(gamma, "gamma", 32); need_f32(beta, "beta", 32);
  check_conv(ds2_bn_cl_apply(y.data_ptr(), mean.data_ptr<float>(), invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                             beta.data_ptr<float>(), out.data_ptr(), (int)y.size(0), (int)y.size(1), (int)y.size(2),
                             tmaj ? 1 : 0, cur_stream()), "bn_cl_apply");
}

// part_ready: part already holds nb partial sums (conv2_dgrad's bn epilogue), skip the reduce pass;
// 2: also skip the apply pass (dgamma / dbeta only: conv1_wgrad applies the backward itself)
void bn_cl_bwd(at::Tensor dz, at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor beta,
               at::Tensor part, int64_t nb, at::Tensor dgamma, at::Tensor dbeta, at::Tensor dy, bool tmaj,
               int64_t part_ready) {
  need_bf16(dz, "dz"); need_bf16(y, "y"); need_bf16(dy, "dy");
  TORCH_CHECK(y.dim() == 4 && y.size(3) == 32 && dz.numel() == y.numel() && dy.numel() == y.numel(),
              "bn_cl_bwd shapes");
  need_f32(part, "part", nb * 64);
  need_f32(mean, "mean", 32); need_f32(invstd, "invstd", 32); need_f32(gamma, "gamma", 32); need_f32(beta, "beta", 32);
  need_f32(dgamma, "dgamma", 32); need_f32(dbeta, "dbeta", 32);
  check_conv(ds2_bn_cl_bwd(dz.data_ptr(), y.data_ptr(), mean.data_ptr<float>(), invstd.data_ptr<float>(),
                           gamma.data_ptr<float>(), beta.data_ptr<float>(), part.data_ptr<float>(), (int)nb,
                           dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), dy.data_ptr(), (int)y.size(0),
                           (int)y.size(1), (int)y.size(2), tmaj ? 1 : 0, (int)part_ready, cur_stream()), "bn_cl_bwd");
}

// --------------------------------------------------------------------------- greedy CTC decode
// logits [T, N, K] (fp32/bf16, time-major) -> labels [N, T] int32 (first counts[n] valid),
// counts [N] int32, optional score [N] fp32 (greedy path log-probability)
void ctc_greedy(at::Tensor logits, at::Tensor lens, at::Tensor labels, at::Tensor counts, int64_t blank,
                OptT score) {
  need_gpu(logits, "logits"); need_gpu(lens, "lens"); need_gpu(labels, "labels"); need_gpu(counts, "counts");
  TORCH_CHECK(logits.dim() == 3, "logits must be [T, N, K]");
  const int T = (int)logits.size(0), N = (int)logits.size(1), K = (int)logits.size(2);
  TORCH_CHECK(lens.scalar_type() == at::kInt && lens.numel() == N, "lens must be int32 [N]");
  TORCH_CHECK(labels.scalar_type() == at::kInt && labels.numel() >= (int64_t)N * T, "labels must be int32 [N, T]");
  TORCH_CHECK(counts.scalar_type() == at::kInt && counts.numel() == N, "counts must be int32 [N]");
  check(ds2_ctc_greedy(logits.data_ptr(), is_bf16(logits), lens.data_ptr<int>(), T, N, K, (int)blank,
                       labels.data_ptr<int>(), counts.data_ptr<int>(), ptr_or_null<float>(score, "score"),
                       cur_stream()), "ctc_greedy");
}

// --------------------------------------------------------------------------- multi-fill
// fill each (contiguous tensor, 32-bit pattern) region in ONE launch (<= 8 regions)
// out [C, R] = in [R, C]^T (bf16, unit-stride rows)
void transpose_bf16(at::Tensor in, at::Tensor out) {
  // rows may be pitched (row stride > row length): the kernel takes both row strides
  TORCH_CHECK(in.is_cuda() && out.is_cuda(), "transpose_bf16: GPU tensors");
  TORCH_CHECK(in.scalar_type() == at::kBFloat16 && out.scalar_type() == at::kBFloat16, "transpose_bf16: bf16");
  TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && in.stride(1) == 1 && out.stride(1) == 1, "transpose_bf16: 2-D rows");
  TORCH_CHECK(out.size(0) == in.size(1) && out.size(1) == in.size(0), "transpose_bf16: out must be [C, R]");
  check(ds2_transpose_bf16(in.data_ptr(), out.data_ptr(), (int)in.size(0), (int)in.size(1), (int)in.stride(0),
                           (int)out.stride(0), cur_stream()),
        "transpose_bf16");
}

// dst_i[r, :] = src_i[r, :] then zeros to dst_i's row end, for 2-D (or 1-D: one row) tensors of
// one dtype with unit-stride rows and src cols <= dst cols; plus ns <= 4 fp32 scalars into
// sdst. ONE launch (csrc/fill.hip multi_copy_kernel).
void multi_copy(std::vector<at::Tensor> dsts, std::vector<at::Tensor> srcs, c10::optional<at::Tensor> sdst,
                std::vector<double> svals) {
  TORCH_CHECK(dsts.size() == srcs.size() && dsts.size() <= 8 && svals.size() <= 4, "multi_copy: <= 8 pairs, <= 4 scalars");
  void* dp[8];
  const void* sp[8];
  unsigned long long rows[8];
  unsigned srow[8], drow[8], spitch[8], dpitch[8];
  for (size_t i = 0; i < dsts.size(); ++i) {
    at::Tensor d = dsts[i], s = srcs[i];
    // 2-D pairs may be pitched views (unit-stride rows, checked below); 1-D ones are contiguous
    TORCH_CHECK(d.is_cuda() && s.is_cuda(), "multi_copy: GPU tensors");
    TORCH_CHECK(d.scalar_type() == s.scalar_type() && d.dim() == s.dim() && (d.dim() == 1 || d.dim() == 2),
                "multi_copy: same dtype, 1-D or 2-D");
    const int64_t es = d.element_size();
    if (d.dim() == 1) {
      TORCH_CHECK(d.is_contiguous() && s.is_contiguous() && s.numel() <= d.numel(), "multi_copy: 1-D contiguous");
      rows[i] = 1;
      srow[i] = (unsigned)(s.numel() * es); drow[i] = (unsigned)(d.numel() * es);
      spitch[i] = srow[i]; dpitch[i] = drow[i];
    } else {
      TORCH_CHECK(d.size(0) == s.size(0) && s.size(1) <= d.size(1) && d.stride(1) == 1 && s.stride(1) == 1,
                  "multi_copy: rows match, unit-stride rows, src cols <= dst cols");
      TORCH_CHECK((d.size(0) <= 1 || d.stride(0) >= d.size(1)) && (s.size(0) <= 1 || s.stride(0) >= s.size(1)),
                  "multi_copy: rows must not overlap");
      rows[i] = (unsigned long long)d.size(0);
      srow[i] = (unsigned)(s.size(1) * es); drow[i] = (unsigned)(d.size(1) * es);
      spitch[i] = (unsigned)(std::max<int64_t>(s.stride(0), s.size(1)) * es);
      dpitch[i] = (unsigned)(std::max<int64_t>(d.stride(0), d.size(1)) * es);
    }
    dp[i] = d.data_ptr();
    sp[i] = s.data_ptr();
  }
  float sv[4] = {0.f, 0.f, 0.f, 0.f};
  for (size_t i = 0; i < svals.size(); ++i) sv[i] = (float)svals[i];
  float* sd = nullptr;
  if (sdst.has_value()) {
    need_gpu(*sdst, "multi_copy scalars");
    TORCH_CHECK(sdst->scalar_type() == at::kFloat && sdst->is_contiguous() && sdst->numel() >= (int64_t)svals.size(),
                "multi_copy: fp32 scalar slot");
    sd = sdst->data_ptr<float>();
  }
  check(ds2_multi_copy((int)dsts.size(), dp, sp, rows, srow, drow, spitch, dpitch, sd, sv, (int)svals.size(),
                       cur_stream()),
        "multi_copy");
}

// feats fp32 -> bf16 (same shape, contiguous) and rnn lengths floor((seq_lens - 34) / 4), int32
void prep_inputs(at::Tensor x, at::Tensor y, at::Tensor lens_in, at::Tensor lens_out) {
  need_gpu(x, "feats");
  need_gpu(y, "feats bf16");
  need_gpu(lens_in, "seq_lens");
  need_gpu(lens_out, "rnn lens");
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kBFloat16 && x.is_contiguous() &&
                  y.is_contiguous() && x.numel() == y.numel(), "prep_inputs: fp32 feats -> bf16 of the same size");
  TORCH_CHECK(lens_in.scalar_type() == at::kInt && lens_out.scalar_type() == at::kInt && lens_in.is_contiguous() &&
                  lens_out.is_contiguous() && lens_in.numel() == lens_out.numel(), "prep_inputs: int32 lengths");
  check(ds2_prep_inputs(x.data_ptr<float>(), y.data_ptr(), x.numel(), lens_in.data_ptr<int>(),
                        lens_out.data_ptr<int>(), (int)lens_in.numel(), cur_stream()),
        "prep_inputs");
}

// a wave on the current stream that waits (bounded by `timeout` s_memrealtime ticks) until census
// word `word` (int32, one element) is no longer -1: the persistent launch owning it is resident
// (csrc/fill.hip)
void wait_resident(at::Tensor word, int64_t timeout) {
  need_gpu(word, "census word");
  TORCH_CHECK(word.scalar_type() == at::kInt && word.numel() == 1, "wait_resident: one int32 census word");
  check(ds2_wait_resident(reinterpret_cast<const unsigned*>(word.data_ptr<int>()), (long long)timeout, cur_stream()),
        "wait_resident");
}

void multi_fill(std::vector<at::Tensor> ts, std::vector<int64_t> patterns) {
  TORCH_CHECK(ts.size() == patterns.size() && ts.size() <= 8, "multi_fill: <= 8 (tensor, pattern) pairs");
  void* ptrs[8];
  unsigned long long bytes[8];
  unsigned pats[8];
  for (size_t i = 0; i < ts.size(); ++i) {
    need_gpu(ts[i], "multi_fill region");
    ptrs[i] = ts[i].data_ptr();
    bytes[i] = (unsigned long long)ts[i].numel() * ts[i].element_size();
    pats[i] = (unsigned)(uint32_t)patterns[i];
  }
  check(ds2_multi_fill((int)ts.size(), ptrs, bytes, pats, cur_stream()), "multi_fill");
}

// out_j (= or +=) sum over axis 1 of in_j [R, B, C] (fp32, contiguous) into out_j [R * C]
// (fp32, contiguous): up to 4 slabs in one launch (csrc/reduce.hip, recurrent bias gradients)
void col_sum(std::vector<at::Tensor> ins, std::vector<at::Tensor> outs, std::vector<bool> acc) {
  TORCH_CHECK(!ins.empty() && ins.size() <= 4 && ins.size() == outs.size() && ins.size() == acc.size(),
              "col_sum: 1..4 (in, out, accumulate) triples");
  const float* ip[4];
  float* op[4];
  int R[4], B[4], C[4], a[4];
  for (size_t j = 0; j < ins.size(); ++j) {
    need_gpu(ins[j], "col_sum in");
    need_gpu(outs[j], "col_sum out");
    TORCH_CHECK(ins[j].dim() == 3 && ins[j].scalar_type() == at::kFloat && ins[j].is_contiguous(),
                "col_sum: in must be a contiguous fp32 [R, B, C]");
    TORCH_CHECK(outs[j].scalar_type() == at::kFloat && outs[j].is_contiguous() &&
                    outs[j].numel() == ins[j].size(0) * ins[j].size(2),
                "col_sum: out must be a contiguous fp32 tensor of R * C elements");
    ip[j] = ins[j].data_ptr<float>();
    op[j] = outs[j].data_ptr<float>();
    R[j] = (int)ins[j].size(0);
    B[j] = (int)ins[j].size(1);
    C[j] = (int)ins[j].size(2);
    a[j] = acc[j] ? 1 : 0;
  }
  check(ds2_col_sum((int)ins.size(), ip, op, R, B, C, a, cur_stream()), "col_sum");
}

// CTC prefix beam search (csrc/beam.hip): advance the device-resident beams of B streams by the
// frames of lp [T, B, K] (fp32 log-probs; frames [B] int32 per-stream frame counts, or all T)
static void beam_state_check(const at::Tensor& node, const at::Tensor& last, const at::Tensor& parent,
                             const at::Tensor& pb, const at::Tensor& pnb, const at::Tensor& nbeam,
                             const at::Tensor& nodes, const at::Tensor& nnodes, int64_t B) {
  for (const at::Tensor* t : {&node, &last, &parent, &pb, &pnb, &nbeam, &nodes, &nnodes}) {
    need_gpu(*t, "beam state");
    TORCH_CHECK(t->is_contiguous() && t->size(0) == B, "beam state: contiguous, leading dim B");
  }
  const int64_t W = node.size(1);
  for (const at::Tensor* t : {&node, &last, &parent, &nbeam, &nodes, &nnodes})
    TORCH_CHECK(t->scalar_type() == at::kInt, "beam state: int32 node / label / count tensors");
  TORCH_CHECK(pb.scalar_type() == at::kFloat && pnb.scalar_type() == at::kFloat, "beam state: fp32 scores");
  TORCH_CHECK(node.dim() == 2 && last.sizes() == node.sizes() && parent.sizes() == node.sizes() &&
                  pb.sizes() == node.sizes() && pnb.sizes() == node.sizes() && W >= 1 && W <= 32,
              "beam state: [B, W] tensors, 1 <= W <= 32");
  TORCH_CHECK(nodes.dim() == 3 && nodes.size(2) == 2, "beam state: nodes [B, cap, 2]");
  TORCH_CHECK(nbeam.numel() == B && nnodes.numel() == B, "beam state: nbeam / nnodes [B]");
}

void ctc_beam(at::Tensor lp, OptT frames, int64_t blank, double prune, at::Tensor node, at::Tensor last,
              at::Tensor parent, at::Tensor pb, at::Tensor pnb, at::Tensor nbeam, at::Tensor nodes,
              at::Tensor nnodes, at::Tensor err) {
  need_gpu(lp, "lp");
  TORCH_CHECK(lp.dim() == 3 && lp.scalar_type() == at::kFloat && lp.is_contiguous(),
              "ctc_beam: lp must be contiguous fp32 [T, B, K]");
  const int64_t T = lp.size(0), B = lp.size(1), K = lp.size(2);
  TORCH_CHECK(K >= 2 && K <= 64 && blank >= 0 && blank < K, "ctc_beam: 2 <= K <= 64, 0 <= blank < K");
  beam_state_check(node, last, parent, pb, pnb, nbeam, nodes, nnodes, B);
  need_gpu(err, "err");
  TORCH_CHECK(err.scalar_type() == at::kInt && err.numel() >= 1, "ctc_beam: err int32 [1]");
  const int* fr = nullptr;
  if (frames) {
    need_gpu(*frames, "frames");
    TORCH_CHECK(frames->scalar_type() == at::kInt && frames->is_contiguous() && frames->numel() == B,
                "ctc_beam: frames int32 [B]");
    fr = frames->data_ptr<int>();
  }
  check(ds2_ctc_beam(lp.data_ptr<float>(), fr, (int)T, (int)B, (int)K, (int)node.size(1), (int)blank, (float)prune,
                     node.data_ptr<int>(), last.data_ptr<int>(), parent.data_ptr<int>(), pb.data_ptr<float>(),
                     pnb.data_ptr<float>(), nbeam.data_ptr<int>(), nodes.data_ptr(), nnodes.data_ptr<int>(),
                     (int)nodes.size(1), reinterpret_cast<unsigned*>(err.data_ptr<int>()), cur_stream()),
        "ctc_beam");
}

// labels [B, W, Lcap] (back-aligned prefix walk: the first out_len entries), out_len [B, W] (-1:
// no hypothesis), score [B, W] of the device beams
void ctc_beam_backtrack(at::Tensor node, at::Tensor last, at::Tensor parent, at::Tensor pb, at::Tensor pnb,
                        at::Tensor nbeam, at::Tensor nodes, at::Tensor nnodes, at::Tensor out, at::Tensor out_len,
                        at::Tensor score) {
  const int64_t B = node.size(0), W = node.size(1);
  beam_state_check(node, last, parent, pb, pnb, nbeam, nodes, nnodes, B);
  need_gpu(out, "out");
  need_gpu(out_len, "out_len");
  need_gpu(score, "score");
  TORCH_CHECK(out.dim() == 3 && out.size(0) == B && out.size(1) == W && out.scalar_type() == at::kInt &&
                  out.is_contiguous(), "ctc_beam_backtrack: out int32 [B, W, L]");
  TORCH_CHECK(out_len.numel() == B * W && out_len.scalar_type() == at::kInt && out_len.is_contiguous() &&
                  score.numel() == B * W && score.scalar_type() == at::kFloat && score.is_contiguous(),
              "ctc_beam_backtrack: out_len int32 / score fp32 [B, W]");
  check(ds2_ctc_beam_backtrack(nodes.data_ptr(), (int)nodes.size(1), node.data_ptr<int>(), nbeam.data_ptr<int>(),
                               pb.data_ptr<float>(), pnb.data_ptr<float>(), (int)B, (int)W, out.data_ptr<int>(),
                               out_len.data_ptr<int>(), score.data_ptr<float>(), (int)out.size(2), cur_stream()),
        "ctc_beam_backtrack");
}

// LM shallow fusion (deepspeech_amd/lm.py): lm [S, K, 2] int32 (w fp32 bits, next state),
// lmstate [B, W] int32 and lmkey [B, W, 2] int64 (prefix fingerprints) beside the beam state
static void beam_lm_check(const at::Tensor& lm, const at::Tensor& lmstate, const at::Tensor& node, int64_t K) {
  need_gpu(lm, "lm");
  need_gpu(lmstate, "lmstate");
  TORCH_CHECK(lm.dim() == 3 && lm.size(2) == 2 && lm.size(1) == K && lm.size(0) >= 1 &&
                  lm.scalar_type() == at::kInt && lm.is_contiguous() && lm.size(0) * K < (1ll << 31),
              "beam lm: contiguous int32 [S, K, 2], S * K < 2^31");
  TORCH_CHECK(lmstate.scalar_type() == at::kInt && lmstate.is_contiguous() && lmstate.sizes() == node.sizes(),
              "beam lm: lmstate int32 [B, W]");
}

void ctc_beam_lm(at::Tensor lp, OptT frames, int64_t blank, double prune, at::Tensor node, at::Tensor last,
                 at::Tensor parent, at::Tensor pb, at::Tensor pnb, at::Tensor nbeam, at::Tensor nodes,
                 at::Tensor nnodes, at::Tensor err, at::Tensor lm, at::Tensor lmstate, at::Tensor lmkey) {
  need_gpu(lp, "lp");
  TORCH_CHECK(lp.dim() == 3 && lp.scalar_type() == at::kFloat && lp.is_contiguous(),
              "ctc_beam_lm: lp must be contiguous fp32 [T, B, K]");
  const int64_t T = lp.size(0), B = lp.size(1), K = lp.size(2);
  TORCH_CHECK(K >= 2 && K <= 64 && blank >= 0 && blank < K, "ctc_beam_lm: 2 <= K <= 64, 0 <= blank < K");
  beam_state_check(node, last, parent, pb, pnb, nbeam, nodes, nnodes, B);
  beam_lm_check(lm, lmstate, node, K);
  need_gpu(lmkey, "lmkey");
  TORCH_CHECK(lmkey.scalar_type() == at::kLong && lmkey.is_contiguous() && lmkey.dim() == 3 &&
                  lmkey.size(0) == B && lmkey.size(1) == node.size(1) && lmkey.size(2) == 2,
              "ctc_beam_lm: lmkey int64 [B, W, 2]");
  need_gpu(err, "err");
  TORCH_CHECK(err.scalar_type() == at::kInt && err.numel() >= 1, "ctc_beam_lm: err int32 [1]");
  const int* fr = nullptr;
  if (frames) {
    need_gpu(*frames, "frames");
    TORCH_CHECK(frames->scalar_type() == at::kInt && frames->is_contiguous() && frames->numel() == B,
                "ctc_beam_lm: frames int32 [B]");
    fr = frames->data_ptr<int>();
  }
  check(ds2_ctc_beam_lm(lp.data_ptr<float>(), fr, (int)T, (int)B, (int)K, (int)node.size(1), (int)blank,
                        (float)prune, node.data_ptr<int>(), last.data_ptr<int>(), parent.data_ptr<int>(),
                        pb.data_ptr<float>(), pnb.data_ptr<float>(), nbeam.data_ptr<int>(), nodes.data_ptr(),
                        nnodes.data_ptr<int>(), (int)nodes.size(1), reinterpret_cast<unsigned*>(err.data_ptr<int>()),
                        lm.data_ptr(), (int)lm.size(0), lmstate.data_ptr<int>(),
                        reinterpret_cast<unsigned long long*>(lmkey.data_ptr<int64_t>()), cur_stream()),
        "ctc_beam_lm");
}

// ctc_beam_backtrack with the </s> weight of each hypothesis' LM state added to its score
void ctc_beam_backtrack_lm(at::Tensor node, at::Tensor last, at::Tensor parent, at::Tensor pb, at::Tensor pnb,
                           at::Tensor nbeam, at::Tensor nodes, at::Tensor nnodes, at::Tensor out, at::Tensor out_len,
                           at::Tensor score, at::Tensor lm, at::Tensor lmstate, int64_t blank) {
  const int64_t B = node.size(0), W = node.size(1);
  beam_state_check(node, last, parent, pb, pnb, nbeam, nodes, nnodes, B);
  TORCH_CHECK(lm.dim() == 3, "beam lm: contiguous int32 [S, K, 2]");
  const int64_t K = lm.size(1);
  beam_lm_check(lm, lmstate, node, K);
  TORCH_CHECK(blank >= 0 && blank < K, "ctc_beam_backtrack_lm: 0 <= blank < K");
  need_gpu(out, "out");
  need_gpu(out_len, "out_len");
  need_gpu(score, "score");
  TORCH_CHECK(out.dim() == 3 && out.size(0) == B && out.size(1) == W && out.scalar_type() == at::kInt &&
                  out.is_contiguous(), "ctc_beam_backtrack_lm: out int32 [B, W, L]");
  TORCH_CHECK(out_len.numel() == B * W && out_len.scalar_type() == at::kInt && out_len.is_contiguous() &&
                  score.numel() == B * W && score.scalar_type() == at::kFloat && score.is_contiguous(),
              "ctc_beam_backtrack_lm: out_len int32 / score fp32 [B, W]");
  check(ds2_ctc_beam_backtrack_lm(nodes.data_ptr(), (int)nodes.size(1), node.data_ptr<int>(), nbeam.data_ptr<int>(),
                                  pb.data_ptr<float>(), pnb.data_ptr<float>(), (int)B, (int)W, out.data_ptr<int>(),
                                  out_len.data_ptr<int>(), score.data_ptr<float>(), (int)out.size(2), lm.data_ptr(),
                                  (int)lm.size(0), (int)K, (int)blank, lmstate.data_ptr<int>(), cur_stream()),
        "ctc_beam_backtrack_lm");
}

// out[k] (= or +=) scale[0] * alpha * sum_m G[m, k] for k < K (G bf16 [M, ldg] with unit column
// stride, scale a device fp32 scalar): the FC head's bias gradient (csrc/reduce.hip)
void fc_bias_grad(at::Tensor G, int64_t K, at::Tensor scale, double alpha, at::Tensor out, bool acc) {
  need_gpu(G, "G");
  need_gpu(scale, "scale");
  need_gpu(out, "out");
  TORCH_CHECK(G.dim() == 2 && G.scalar_type() == at::kBFloat16 && G.stride(1) == 1, "fc_bias_grad: G bf16 [M, ldg]");
  // M = 0 (an empty tensor has no data pointer) is legal: out = 0, or out unchanged under acc
  TORCH_CHECK(K >= 1 && K <= 32 && G.size(1) >= 32 && G.stride(0) % 8 == 0 &&
                  (G.size(0) == 0 || G.data_ptr<at::BFloat16>() != nullptr) &&
                  reinterpret_cast<uintptr_t>(G.data_ptr()) % 16 == 0,
              "fc_bias_grad: 1 <= K <= 32, G of >= 32 columns, row stride % 8 == 0, 16-B aligned");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() >= 1, "fc_bias_grad: fp32 device scale");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() == K, "fc_bias_grad: fp32 out [K]");
  check(ds2_fc_bias_grad(G.data_ptr(), (int)G.size(0), (int)G.stride(0), (int)K, scale.data_ptr<float>(),
                         (float)alpha, out.data_ptr<float>(), acc ? 1 : 0, cur_stream()),
        "fc_bias_grad");
}

// --------------------------------------------------------------------------- fp8 quantisation
int64_t fp8_quant_blocks(int64_t na, int64_t nb) { return ds2_fp8_quant_blocks(na, nb); }

// per-tensor e4m3fn quantisation of two bf16 operands a [rows_a, K], b [rows_b, K] into
// a8 [rows_a, Kp], b8 [rows_b, Kp] (columns >= K zero); scales[0] = amax_a/448,
// scales[1] = amax_b/448 * alpha (device-side, for the fp8 GEMM's epilogue). a2 / asum (given
// together, a's shape): operand a is a + a2 (a bidirectional layer's two direction outputs),
// its bf16 sum written to asum in the same pass (bitwise torch.add) and quantised from there.
void fp8_quant2(at::Tensor a, at::Tensor b, double alpha, at::Tensor a8, at::Tensor b8, at::Tensor part,
                at::Tensor scales, c10::optional<at::Tensor> a2, c10::optional<at::Tensor> asum) {
  TORCH_CHECK(a2.has_value() == asum.has_value(), "fp8_quant2: a2 and asum go together");
  if (a2.has_value()) {
    need_gpu(*a2, "a2");
    need_gpu(*asum, "asum");
    TORCH_CHECK(a2->scalar_type() == at::kBFloat16 && asum->scalar_type() == at::kBFloat16 && a2->is_contiguous() &&
                    asum->is_contiguous() && a2->sizes() == a.sizes() && asum->sizes() == a.sizes() &&
                    (reinterpret_cast<uintptr_t>(a2->data_ptr()) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(asum->data_ptr()) & 15) == 0,
                "a2 / asum: contiguous 16-B aligned bf16 of a's shape");
  }
  need_gpu(a, "a");
  need_gpu(b, "b");
  need_gpu(a8, "a8");
  need_gpu(b8, "b8");
  need_gpu(part, "part");
  need_gpu(scales, "scales");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16, "bf16 operands expected");
  TORCH_CHECK(a8.scalar_type() == at::kFloat8_e4m3fn && b8.scalar_type() == at::kFloat8_e4m3fn, "e4m3fn outputs");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.is_contiguous() && b.is_contiguous() && a.size(1) == b.size(1),
              "a [rows_a, K], b [rows_b, K] contiguous");
  const int64_t K = a.size(1), Kp = a8.size(-1);
  TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.is_contiguous() && b8.is_contiguous() && a8.size(0) == a.size(0) &&
                  b8.size(0) == b.size(0) && b8.size(1) == Kp && Kp >= K && K % 8 == 0 && Kp % 8 == 0,
              "a8 [rows_a, Kp], b8 [rows_b, Kp], Kp >= K, K % 8 == 0");
  TORCH_CHECK(scales.scalar_type() == at::kFloat && scales.numel() >= 2, "scales: 2 floats");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(b.data_ptr()) & 15) == 0,
              "16-B aligned operands expected");
  // the cast stores 8 bytes (uint2) per chunk
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a8.data_ptr()) & 7) == 0 && (reinterpret_cast<uintptr_t>(b8.data_ptr()) & 7) == 0,
              "fp8_quant2: a8 / b8 must be 8-byte aligned");
  const int nb = ds2_fp8_quant_blocks(a.size(0) * Kp, b.size(0) * Kp);
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.numel() >= 2 * nb, "part: 2*blocks floats");
  check(ds2_fp8_quant2(a.data_ptr(), a.size(0), b.data_ptr(), b.size(0), (int)K, (int)Kp, (float)alpha, a8.data_ptr(),
                       b8.data_ptr(), part.data_ptr<float>(), scales.data_ptr<float>(),
                       a2.has_value() ? a2->data_ptr() : nullptr, asum.has_value() ? asum->data_ptr() : nullptr,
                       cur_stream()),
        "fp8_quant2");
}

// --------------------------------------------------------------------------- GEMM (csrc/gemm8.hip)
// C = epi(alpha * alpha_dev * alpha_dev2 * A B^T) on the STORED operands: A [(batch,) M, K] or,
// a_col, [(batch,) K, M]; B [(batch,) N, K] or, b_col, [(batch,) K, N]; unit-stride rows.
// bf16 (row-mode K % 32 == 0) or fp8 e4m3fn (row mode, K % 128 == 0). C bf16 (epi 0, + bias)
// or fp32 (epi 1 store, 2 accumulate). splits > 1: split-K through ws (fp32).
static const float* dev_scalar(const OptT& t, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->numel() >= 1, name, " must be an fp32 device scalar");
  return t->data_ptr<float>();
}

static int dev_cus() {
  static int cus_of[64] = {0};
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "hipGetDevice");
  if (!cus_of[dev])
    TORCH_CHECK(hipDeviceGetAttribute(&cus_of[dev], hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess,
                "CU count");
  return cus_of[dev];
}

// fill: regions the GEMM launch initialises for the next kernel (multi_fill semantics)
DS2Fill make_fill(const std::vector<at::Tensor>& fill, const std::vector<int64_t>& fill_pat) {
  TORCH_CHECK(fill.size() == fill_pat.size() && fill.size() <= 8, "<= 8 (fill region, pattern) pairs");
  DS2Fill fd{};
  fd.n = (int)fill.size();
  for (size_t i = 0; i < fill.size(); ++i) {
    need_gpu(fill[i], "fill region");
    TORCH_CHECK((fill[i].numel() * fill[i].element_size()) % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(fill[i].data_ptr()) & 3) == 0,
                "fill regions of whole, aligned 32-bit words");
    fd.ptr[i] = (unsigned*)fill[i].data_ptr();
    fd.words[i] = (unsigned long long)fill[i].numel() * fill[i].element_size() / 4;
    fd.pattern[i] = (unsigned)(uint32_t)fill_pat[i];
  }
  return fd;
}

void gemm8(at::Tensor A, at::Tensor B, at::Tensor C, OptT bias, int64_t epi, double alpha, OptT alpha_dev,
           OptT alpha_dev2, bool a_col, bool b_col, int64_t splits, OptT ws, OptT cnt, int64_t max_grid,
           std::vector<at::Tensor> fill, std::vector<int64_t> fill_pat, bool ext_red) {
  const bool fp8 = A.scalar_type() == at::kFloat8_e4m3fn;
  const DS2Fill fd = make_fill(fill, fill_pat);
  TORCH_CHECK(fp8 ? B.scalar_type() == at::kFloat8_e4m3fn
                  : (A.scalar_type() == at::kBFloat16 && B.scalar_type() == at::kBFloat16),
              "gemm8: bf16 or fp8 e4m3fn operands (both the same)");
  TORCH_CHECK(epi >= 0 && epi <= 2, "gemm8: epi 0..2");
  TORCH_CHECK(C.scalar_type() == (epi == 0 ? at::kBFloat16 : at::kFloat), "gemm8: C dtype does not match epi");
  TORCH_CHECK(B.dim() == A.dim() && C.dim() == A.dim() && (A.dim() == 2 || A.dim() == 3), "gemm8: 2-D or batched 3-D");
  for (const at::Tensor* t : {&A, &B, &C}) {
    TORCH_CHECK(t->is_cuda() && t->stride(-1) == 1, "gemm8: unit-stride rows");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(t->data_ptr()) & 15) == 0, "gemm8: 16-B aligned operands");
  }
  const int64_t batch = A.dim() == 3 ? A.size(0) : 1;
  if (batch > 1) TORCH_CHECK(B.size(0) == batch && C.size(0) == batch, "gemm8: batch mismatch");
  const int64_t M = a_col ? A.size(-1) : A.size(-2), K = a_col ? A.size(-2) : A.size(-1);
  const int64_t N = b_col ? B.size(-1) : B.size(-2), Kb = b_col ? B.size(-2) : B.size(-1);
  TORCH_CHECK(Kb == K && C.size(-2) == M && C.size(-1) == N, "gemm8: shapes");
  const int64_t lda = A.stride(-2), ldb = B.stride(-2), ldc = C.stride(-2);
  const void* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(epi == 0 && bias->scalar_type() == at::kBFloat16 && bias->is_contiguous() && bias->numel() == N,
                "gemm8: bias must be bf16 [N] (epi 0)");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(bias->data_ptr()) & 7) == 0, "gemm8: bias 8-B aligned");
    bp = bias->data_ptr();
  }
  float* wsp = nullptr;
  unsigned* cntp = nullptr;
  const int S = ds2_gemm8_splits((int)K, fp8 ? 1 : 0, (int)std::max<int64_t>(1, splits));
  if (S > 1) {
    TORCH_CHECK(ws.has_value() && ws->defined() && ws->is_cuda() && ws->scalar_type() == at::kFloat &&
                    ws->numel() >= (int64_t)S * batch * M * N,
                "gemm8: split-K needs an fp32 workspace of ", S * batch * M * N, " floats");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(ws->data_ptr()) & 15) == 0, "gemm8: 16-B aligned workspace");
    wsp = ws->data_ptr<float>();
    const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256) * batch;
    TORCH_CHECK(cnt.has_value() && cnt->defined() && cnt->is_cuda() && cnt->scalar_type() == at::kInt &&
                    cnt->numel() >= tiles,
                "gemm8: split-K needs ", tiles, " zeroed int32 tile counters (one buffer per stream)");
    cntp = reinterpret_cast<unsigned*>(cnt->data_ptr<int>());
  }
  const int64_t sA = batch > 1 ? A.stride(0) : 0, sB = batch > 1 ? B.stride(0) : 0, sC = batch > 1 ? C.stride(0) : 0;
  check(ds2_gemm8(A.data_ptr(), B.data_ptr(), C.data_ptr(), bp, dev_scalar(alpha_dev, "alpha_dev"),
                  dev_scalar(alpha_dev2, "alpha_dev2"), (int)M, (int)N, (int)K, (int)lda, (int)ldb, (int)ldc,
                  fp8 ? 1 : 0, a_col ? 1 : 0, b_col ? 1 : 0, (int)epi, (float)alpha, (int)batch, sA, sB, sC, S, wsp,
                  cntp, max_grid > 0 ? (int)std::min<int64_t>(max_grid, dev_cus()) : dev_cus(), fd.n ? &fd : nullptr,
                  ext_red ? 1 : 0, cur_stream()),
        "gemm8");
}

// A group of independent bf16 GEMMs of the same operand modes in one launch (one grid over all
// their tiles): C[i] (fp32, epi[i] 1 store / 2 accumulate) = A[i] B[i]^T, split-K S[i] through
// consecutive ranges of one workspace ws (S[i] * M * N floats each) and one zeroed counter
// buffer cnt (tiles each).
void gemm8_group(std::vector<at::Tensor> A, std::vector<at::Tensor> B, std::vector<at::Tensor> C,
                 std::vector<int64_t> epi, std::vector<int64_t> splits, bool a_col, bool b_col, OptT ws, OptT cnt,
                 int64_t max_grid) {
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
    TORCH_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16 && c.scalar_type() == at::kFloat,
                "gemm8_group: bf16 operands, fp32 C");
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "gemm8_group: 2-D members");
    for (const at::Tensor* t : {&a, &b, &c}) {
      TORCH_CHECK(t->is_cuda() && t->stride(-1) == 1, "gemm8_group: unit-stride rows");
      TORCH_CHECK((reinterpret_cast<uintptr_t>(t->data_ptr()) & 15) == 0, "gemm8_group: 16-B aligned operands");
    }
    const int64_t M = a_col ? a.size(1) : a.size(0), K = a_col ? a.size(0) : a.size(1);
    const int64_t N = b_col ? b.size(1) : b.size(0), Kb = b_col ? b.size(0) : b.size(1);
    TORCH_CHECK(Kb == K && c.size(0) == M && c.size(1) == N, "gemm8_group: shapes of member ", i);
    TORCH_CHECK(epi[i] == 1 || epi[i] == 2, "gemm8_group: epi 1 or 2");
    const int S = ds2_gemm8_splits((int)K, 0, (int)std::max<int64_t>(1, splits[i]));
    if (S > 1) {
      const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
      TORCH_CHECK(ws.has_value() && ws->defined() && ws->is_cuda() && ws->scalar_type() == at::kFloat &&
                      ws->numel() >= wofs + (int64_t)S * M * N,
                  "gemm8_group: split-K workspace too small");
      TORCH_CHECK(cnt.has_value() && cnt->defined() && cnt->is_cuda() && cnt->scalar_type() == at::kInt &&
                      cnt->numel() >= cofs + tiles,
                  "gemm8_group: split-K counters too small");
      pw[i] = ws->data_ptr<float>() + wofs;
      TORCH_CHECK((reinterpret_cast<uintptr_t>(pw[i]) & 15) == 0, "gemm8_group: 16-B aligned workspace");
      pn[i] = reinterpret_cast<unsigned*>(cnt->data_ptr<int>()) + cofs;
      wofs += (int64_t)S * M * N;
      cofs += tiles;
    }
    pa[i] = a.data_ptr();
    pb[i] = b.data_ptr();
    pc[i] = c.data_ptr();
    int* d = dims.data() + 8 * i;
    d[0] = (int)M; d[1] = (int)N; d[2] = (int)K;
    d[3] = (int)a.stride(0); d[4] = (int)b.stride(0); d[5] = (int)c.stride(0);
    d[6] = (int)epi[i]; d[7] = S;
  }
  check(ds2_gemm8_group((int)np, pa.data(), pb.data(), pc.data(), pw.data(), pn.data(), dims.data(), a_col ? 1 : 0,
                        b_col ? 1 : 0, max_grid > 0 ? (int)std::min<int64_t>(max_grid, dev_cus()) : dev_cus(),
                        cur_stream()),
        "gemm8_group");
}

// --------------------------------------------------------------------------- GEMM (csrc/gemm.hip)
// Operands are given as (possibly batched) matrices whose innermost dimension is unit-stride;
// the leading dimension is the row stride. a_col / b_col select the column-major reading of
// the csrc/gemm.hip header. epi 0: bf16 C = alpha*acc + bias; 1: fp32 C = alpha*acc;
// 2: fp32 C += alpha*acc.
int64_t ld_of(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.dim() == 2 || t.dim() == 3, name, " must be 2-D or batched 3-D");
  TORCH_CHECK(t.stride(-1) == 1, name, " must have a unit-stride last dimension");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, name, " must be 16-B aligned");
  const int64_t ld = t.dim() == 2 ? t.stride(0) : t.stride(1);
  TORCH_CHECK(ld % 8 == 0, name, " row stride must be a multiple of 8 elements");
  return ld;
}

void gemm(at::Tensor A, at::Tensor B, at::Tensor C, OptT bias, int64_t M, int64_t N, int64_t K, bool a_col,
          bool b_col, int64_t epi, double alpha, int64_t cfg, OptT alpha_dev, int64_t Ml, int64_t Nl, int64_t Kl,
          std::vector<at::Tensor> fill, std::vector<int64_t> fill_pat) {
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 && B.scalar_type() == at::kBFloat16, "gemm: bf16 operands");
  const DS2Fill fd = make_fill(fill, fill_pat);
  TORCH_CHECK(epi >= 0 && epi <= 2, "gemm: epi 0..2");
  TORCH_CHECK(C.scalar_type() == (epi == 0 ? at::kBFloat16 : at::kFloat), "gemm: C dtype does not match epi");
  const int64_t lda = ld_of(A, "A"), ldb = ld_of(B, "B"), ldc = ld_of(C, "C");
  const int64_t batch = A.dim() == 3 ? A.size(0) : 1;
  TORCH_CHECK(B.dim() == A.dim() && C.dim() == A.dim(), "gemm: operands must all be 2-D or all 3-D");
  if (batch > 1) TORCH_CHECK(B.size(0) == batch && C.size(0) == batch, "gemm: batch mismatch");
  // stored extents: a col-mode operand may be padded to Ml/Nl columns and hold only Kl k-rows
  const int64_t Mx = Ml ? Ml : M, Nx = Nl ? Nl : N, Kx = Kl ? Kl : K;
  const int64_t ar = a_col ? Kx : M, ac = a_col ? Mx : K, br = b_col ? Kx : N, bc = b_col ? Nx : K;
  TORCH_CHECK(A.size(-2) == ar && A.size(-1) == ac, "gemm: A shape");
  TORCH_CHECK(B.size(-2) == br && B.size(-1) == bc, "gemm: B shape");
  const float* ad = nullptr;
  if (alpha_dev.has_value() && alpha_dev->defined()) {
    TORCH_CHECK(alpha_dev->is_cuda() && alpha_dev->scalar_type() == at::kFloat && alpha_dev->numel() == 1,
                "gemm: alpha_dev must be one fp32 device scalar");
    ad = alpha_dev->data_ptr<float>();
  }
  TORCH_CHECK(C.size(-2) == M && C.size(-1) == N, "gemm: C shape");
  const void* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(epi == 0 && bias->scalar_type() == at::kBFloat16 && bias->is_contiguous() && bias->numel() == N,
                "gemm: bias must be bf16 [N] (epi 0)");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(bias->data_ptr()) & 7) == 0, "gemm: bias 8-B aligned");
    bp = bias->data_ptr();
  }
  const int64_t sA = batch > 1 ? A.stride(0) : 0, sB = batch > 1 ? B.stride(0) : 0, sC = batch > 1 ? C.stride(0) : 0;
  check(ds2_gemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), bp, ad, (int)M, (int)N, (int)K, (int)lda, (int)ldb,
                 (int)ldc, (int)Ml, (int)Nl, (int)Kl, a_col ? 1 : 0, b_col ? 1 : 0, (int)epi, (float)alpha, (int)batch,
                 sA, sB, sC, (int)cfg, fd.n ? &fd : nullptr, cur_stream()),
        "gemm");
}

// FC head + CTC (training): h [T, N, H] bf16, W [K, H] bf16, bias [K] bf16 -> loss [N] fp32,
// G [T*N, 32] bf16 (per-utterance dloss/dlogits, zero-padded classes)
// mean (optional, [1] fp32): the batch-mean loss written by the same launch; counter / first_bad
// (optional, [1] int32 each): the per-step divergence watch of utils/stats.py NonfiniteWatch
void head_ctc(at::Tensor h, at::Tensor W, at::Tensor bias, at::Tensor lens, at::Tensor labels, at::Tensor label_lens,
              at::Tensor loss, at::Tensor G, at::Tensor ws, int64_t blank, bool zero_inf, OptT mean, OptT counter,
              OptT first_bad) {
  for (auto* t : {&h, &W, &bias, &lens, &labels, &label_lens, &loss, &G, &ws}) need_gpu(*t, "head_ctc operand");
  TORCH_CHECK(h.dim() == 3 && h.scalar_type() == at::kBFloat16, "h: [T, N, H] bf16");
  const int64_t T = h.size(0), N = h.size(1), H = h.size(2), K = W.size(0);
  TORCH_CHECK(W.scalar_type() == at::kBFloat16 && W.dim() == 2 && W.size(1) == H, "W: [K, H] bf16");
  TORCH_CHECK(bias.scalar_type() == at::kBFloat16 && bias.numel() == K, "bias: [K] bf16");
  TORCH_CHECK(K <= 32 && H % 32 == 0, "head_ctc: K <= 32 classes and H % 32 == 0");
  TORCH_CHECK(lens.scalar_type() == at::kInt && lens.numel() == N, "lens: [N] int32");
  TORCH_CHECK(labels.scalar_type() == at::kInt && labels.dim() == 2 && labels.size(0) == N, "labels: [N, Lmax] int32");
  TORCH_CHECK(label_lens.scalar_type() == at::kInt && label_lens.numel() == N, "label_lens: [N] int32");
  TORCH_CHECK(loss.scalar_type() == at::kFloat && loss.numel() == N, "loss: [N] fp32");
  TORCH_CHECK(G.scalar_type() == at::kBFloat16 && G.numel() == T * N * 32, "G: [T*N, 32] bf16");
  const int64_t Lmax = labels.size(1);
  TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.numel() >= ds2_ctc_ws_floats((int)T, (int)N, (int)Lmax),
              "head_ctc: workspace too small");
  float* mean_p = nullptr;
  int *counter_p = nullptr, *first_p = nullptr;
  if (mean.has_value()) {
    need_gpu(*mean, "head_ctc mean");
    TORCH_CHECK(mean->scalar_type() == at::kFloat && mean->numel() == 1, "mean: [1] fp32");
    mean_p = mean->data_ptr<float>();
  }
  if (counter.has_value() || first_bad.has_value()) {
    TORCH_CHECK(mean_p != nullptr && counter.has_value() && first_bad.has_value(),
                "head_ctc: the watch needs mean, counter and first_bad");
    need_gpu(*counter, "head_ctc counter");
    need_gpu(*first_bad, "head_ctc first_bad");
    TORCH_CHECK(counter->scalar_type() == at::kInt && counter->numel() == 1 && first_bad->scalar_type() == at::kInt &&
                    first_bad->numel() == 1, "counter / first_bad: [1] int32");
    counter_p = counter->data_ptr<int>();
    first_p = first_bad->data_ptr<int>();
  }
  check(ds2_head_ctc(h.data_ptr(), W.data_ptr(), bias.data_ptr(), lens.data_ptr<int>(), labels.data_ptr<int>(),
                     label_lens.data_ptr<int>(), loss.data_ptr<float>(), G.data_ptr(), ws.data_ptr<float>(), (int)T,
                     (int)N, (int)H, (int)K, (int)Lmax, (int)blank, zero_inf ? 1 : 0, mean_p, counter_p, first_p,
                     cur_stream()),
        "head_ctc");
}

// FC head alone: logits [M, K] (fp32 or bf16) = h [M, H] W^T + b
void fc_logits(at::Tensor h, at::Tensor W, at::Tensor bias, at::Tensor logits) {
  for (auto* t : {&h, &W, &bias, &logits}) need_gpu(*t, "fc_logits operand");
  const int64_t H = h.size(-1), M = h.numel() / H, K = W.size(0);
  TORCH_CHECK(h.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16 && bias.scalar_type() == at::kBFloat16,
              "fc_logits: bf16 h / W / bias");
  TORCH_CHECK(W.size(1) == H && bias.numel() == K && logits.numel() == M * K && K <= 32 && H % 32 == 0,
              "fc_logits: shapes");
  check(ds2_fc_logits(h.data_ptr(), W.data_ptr(), bias.data_ptr(), logits.data_ptr(), is_bf16(logits), (int)M, (int)H,
                      (int)K, cur_stream()),
        "fc_logits");
}

// --------------------------------------------------------------------------- lookahead convolution (csrc/lookahead.hip)
// Shapes every lookahead entry point shares: x bf16 [T, B, H], w bf16 [H, tau+1]; returns tau.
int lookahead_dims(const at::Tensor& x, const at::Tensor& w, const char* what) {
  need_gpu(x, what);
  need_gpu(w, "lookahead w");
  TORCH_CHECK(x.dim() == 3 && w.dim() == 2 && x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16,
              "lookahead: bf16 [T, B, H] activations and bf16 [H, tau+1] weights");
  const int64_t H = x.size(2), tau = w.size(1) - 1;
  TORCH_CHECK(x.size(0) >= 1 && x.size(1) >= 1 && w.size(0) == H && H % 8 == 0 && tau >= 1 && tau <= 31,
              "lookahead: H % 8 == 0, 1 <= tau <= 31, w [H, tau+1]");
  return (int)tau;
}

const int* lookahead_lens(const at::Tensor& lens, const at::Tensor& x) {
  need_gpu(lens, "lookahead lens");
  TORCH_CHECK(lens.scalar_type() == at::kInt && lens.numel() == x.size(1), "lookahead: lens int32 [B]");
  return lens.data_ptr<int>();
}

// out = r (bwd false, x = h) or dh (bwd true, x = dr)
void lookahead(at::Tensor x, at::Tensor w, at::Tensor lens, at::Tensor out, bool bwd) {
  const int tau = lookahead_dims(x, w, "lookahead x");
  need_gpu(out, "lookahead out");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.sizes() == x.sizes(), "lookahead: out like x");
  check(ds2_lookahead(x.data_ptr(), w.data_ptr(), lookahead_lens(lens, x), out.data_ptr(), (int)x.size(0),
                      (int)x.size(1), (int)x.size(2), tau, bwd ? 1 : 0, cur_stream()),
        "lookahead");
}

int64_t lookahead_wgrad_parts(int64_t T, int64_t B, int64_t H) {
  return ds2_lookahead_wgrad_parts((int)T, (int)B, (int)H);
}

// part [P, H*(tau+1)] fp32, P = lookahead_wgrad_parts(T, B, H); tau is part's to tell
void lookahead_wgrad(at::Tensor dr, at::Tensor h, at::Tensor lens, at::Tensor part, int64_t tau) {
  need_gpu(dr, "lookahead dr");
  need_gpu(h, "lookahead h");
  need_gpu(part, "lookahead part");
  TORCH_CHECK(dr.dim() == 3 && dr.scalar_type() == at::kBFloat16 && h.scalar_type() == at::kBFloat16 &&
                  h.sizes() == dr.sizes() && dr.size(2) % 8 == 0 && tau >= 1 && tau <= 31 && dr.size(0) >= 1 &&
                  dr.size(1) >= 1,
              "lookahead_wgrad: bf16 dr, h [T, B, H], H % 8 == 0, 1 <= tau <= 31");
  const int T = (int)dr.size(0), B = (int)dr.size(1), H = (int)dr.size(2);
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.dim() == 2 &&
                  part.size(0) == ds2_lookahead_wgrad_parts(T, B, H) && part.size(1) == (int64_t)H * (tau + 1),
              "lookahead_wgrad: part fp32 [lookahead_wgrad_parts, H*(tau+1)]");
  check(ds2_lookahead_wgrad(dr.data_ptr(), h.data_ptr(), lookahead_lens(lens, dr), part.data_ptr<float>(), T, B, H,
                            (int)tau, cur_stream()),
        "lookahead_wgrad");
}

// one streaming step: out [n, B, H] from hist [tau, B, H] and x [n, B, H]; hist is rewritten
void lookahead_stream(at::Tensor hist, at::Tensor x, at::Tensor w, at::Tensor out) {
  const int tau = lookahead_dims(x, w, "lookahead x");
  need_gpu(hist, "lookahead hist");
  need_gpu(out, "lookahead out");
  TORCH_CHECK(hist.scalar_type() == at::kBFloat16 && hist.dim() == 3 && hist.size(0) == tau &&
                  hist.size(1) == x.size(1) && hist.size(2) == x.size(2) && out.scalar_type() == at::kBFloat16 &&
                  out.sizes() == x.sizes(),
              "lookahead_stream: hist bf16 [tau, B, H], out like x");
  check(ds2_lookahead_stream(hist.data_ptr(), x.data_ptr(), w.data_ptr(), out.data_ptr(), (int)x.size(0),
                             (int)x.size(1), (int)x.size(2), tau, cur_stream()),
        "lookahead_stream");
}

// --------------------------------------------------------------------------- SpecAugment (csrc/specaug.hip)
// plan int32 [B, 2 + 2 nF + 2 nT] from lens int32 [B]; seed, step and first_utt come as 32-bit words
void specaug_plan(at::Tensor lens, at::Tensor plan, int64_t T, int64_t F, int64_t nF, int64_t Fw, int64_t nT,
                  int64_t Tw, int64_t p_ppm, int64_t W, int64_t seed_lo, int64_t seed_hi, int64_t step_lo,
                  int64_t step_hi, int64_t first_utt) {
  const int64_t B = lens.numel();
  const int* l = need_i32(lens, "specaug lens", B);
  TORCH_CHECK(B >= 1 && B < (1LL << 31) && T >= 1 && T < (1LL << 31) && F >= 1 && F < (1LL << 31),
              "specaug_plan: B, T, F in [1, 2^31)");
  TORCH_CHECK(nF >= 0 && nF <= 8 && nT >= 0 && nT <= 16, "specaug_plan: nF <= 8, nT <= 16");
  TORCH_CHECK(plan.dim() == 2 && plan.size(0) == B && plan.size(1) == 2 + 2 * nF + 2 * nT,
              "specaug_plan: plan int32 [B, 2 + 2 nF + 2 nT]");
  int* p = need_i32(plan, "specaug plan", 0);
  const auto in32 = [](int64_t v) { return v >= 0 && v < (1LL << 31); };
  TORCH_CHECK(in32(Fw) && in32(Tw) && in32(W) && in32(p_ppm), "specaug_plan: policy value out of range");
  const auto word = [](int64_t v) {
    TORCH_CHECK(v >= 0 && v <= 0xffffffffLL, "specaug_plan: seed / step / first_utt as 32-bit words");
    return (unsigned)v;
  };
  check(ds2_specaug_plan(l, p, (int)B, (int)T, (int)F, (int)nF, (int)Fw, (int)nT, (int)Tw, (int)p_ppm, (int)W,
                         word(seed_lo), word(seed_hi), word(step_lo), word(step_hi), word(first_utt), cur_stream()),
        "specaug_plan");
}

void specaug_dims(const at::Tensor& x, const at::Tensor& lens, const char* what) {
  need_gpu(x, what);
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 3, what, " must be float32 [B, T, F]");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= 65535 && x.size(1) >= 1 && x.size(1) <= 32767 && x.size(2) >= 1 &&
                  x.size(2) <= 1024,
              "specaug: B <= 65535, T <= 32767, F <= 1024");
  need_i32(lens, "specaug lens", x.size(0));
  TORCH_CHECK(lens.numel() == x.size(0), "specaug: lens int32 [B]");
}

void specaug_mean(at::Tensor x, at::Tensor lens, at::Tensor mean) {
  specaug_dims(x, lens, "specaug x");
  need_f32(mean, "specaug mean", x.size(0) * x.size(2));
  TORCH_CHECK(mean.numel() == x.size(0) * x.size(2), "specaug_mean: mean float32 [B, F]");
  check(ds2_specaug_mean(x.data_ptr<float>(), lens.data_ptr<int>(), mean.data_ptr<float>(), (int)x.size(0),
                         (int)x.size(1), (int)x.size(2), cur_stream()),
        "specaug_mean");
}

// out = SpecAugment(x) by plan; fill [B, F] or None (zeros); inplace: out is x and only masked cells are written
void specaug_apply(at::Tensor x, at::Tensor lens, at::Tensor plan, OptT fill, at::Tensor out, int64_t nF, int64_t nT,
                   bool inplace) {
  specaug_dims(x, lens, "specaug x");
  need_gpu(out, "specaug out");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.sizes() == x.sizes(), "specaug_apply: out like x");
  TORCH_CHECK(nF >= 0 && nF <= 8 && nT >= 0 && nT <= 16, "specaug_apply: nF <= 8, nT <= 16");
  need_i32(plan, "specaug plan", x.size(0) * (2 + 2 * nF + 2 * nT));
  TORCH_CHECK(plan.numel() == x.size(0) * (2 + 2 * nF + 2 * nT), "specaug_apply: plan int32 [B, 2 + 2 nF + 2 nT]");
  const float* f = ptr_or_null<const float>(fill, "specaug fill");
  if (f) TORCH_CHECK(fill->scalar_type() == at::kFloat && fill->numel() == x.size(0) * x.size(2),
                     "specaug_apply: fill float32 [B, F]");
  check(ds2_specaug_apply(x.data_ptr<float>(), lens.data_ptr<int>(), plan.data_ptr<int>(), f, out.data_ptr<float>(),
                          (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)nF, (int)nT, inplace ? 1 : 0,
                          cur_stream()),
        "specaug_apply");
}

// --------------------------------------------------------------------------- dropout (csrc/dropout.hip)
// out = dropout(x) under the mask of (seed, ctr = (step, first_utt) on the device, site); out may be x
void seq_dropout(at::Tensor x, at::Tensor out, at::Tensor ctr, int64_t seed_lo, int64_t seed_hi, int64_t site,
                 int64_t thr, double scale, bool locked) {
  need_bf16(x, "seq_dropout x");
  need_bf16(out, "seq_dropout out");
  const int* c = need_i32(ctr, "seq_dropout ctr", 2);
  TORCH_CHECK(x.dim() == 3 && out.sizes() == x.sizes() && x.size(0) >= 1 && x.size(1) >= 1 && x.size(2) >= 8 &&
                  x.size(2) % 8 == 0 && x.size(2) <= 8 * 65536,
              "seq_dropout: bf16 x, out [T, N, H], H % 8 == 0");
  TORCH_CHECK(x.numel() / 8 < (1LL << 31), "seq_dropout: T * N * H / 8 < 2^31");
  TORCH_CHECK(x.get_device() == out.get_device() && x.get_device() == ctr.get_device(), "seq_dropout: one device");
  TORCH_CHECK(site >= 0 && site < 16384 && thr >= 1 && thr <= 65535, "seq_dropout: site < 16384, 1 <= thr <= 65535");
  const auto word = [](int64_t v) {
    TORCH_CHECK(v >= 0 && v <= 0xffffffffLL, "seq_dropout: the seed as 32-bit words");
    return (unsigned)v;
  };
  check(ds2_seq_dropout(x.data_ptr(), out.data_ptr(), c, (int)x.size(0), (int)x.size(1), (int)x.size(2),
                        word(seed_lo), word(seed_hi), (int)site, (int)thr, (float)scale, locked ? 1 : 0, cur_stream()),
        "seq_dropout");
}

// --------------------------------------------------------------------------- audio features (csrc/featurize.hip)
int pcm_is_i16(const at::Tensor& pcm) {
  need_gpu(pcm, "pcm");
  TORCH_CHECK(pcm.dim() == 2, "pcm must be [B, S]");
  if (pcm.scalar_type() == at::kShort) return 1;
  TORCH_CHECK(pcm.scalar_type() == at::kFloat, "pcm must be float32 or int16");
  return 0;
}

const int* feat_lens(const OptT& lens, int64_t B) {
  const int* p = ptr_or_null<const int>(lens, "lens");
  if (p) TORCH_CHECK(lens->scalar_type() == at::kInt && lens->numel() == B, "lens must be int32 [B]");
  return p;
}

// per-row offset = mean(x) and gain = 1 / max|x - mean| (1 when the peak is 0), on the device
void audio_stats(at::Tensor pcm, OptT lens, at::Tensor offset, at::Tensor gain) {
  const int i16 = pcm_is_i16(pcm);
  const int64_t B = pcm.size(0), S = pcm.size(1);
  TORCH_CHECK(S < (1LL << 31), "audio_stats: row too long");
  need_gpu(offset, "offset");
  need_gpu(gain, "gain");
  TORCH_CHECK(offset.scalar_type() == at::kFloat && offset.numel() == B && gain.scalar_type() == at::kFloat &&
                  gain.numel() == B, "offset / gain must be fp32 [B]");
  check(ds2_audio_stats(pcm.data_ptr(), i16, S, (int)S, (int)B, feat_lens(lens, B), offset.data_ptr<float>(),
                        gain.data_ptr<float>(), cur_stream()),
        "audio_stats");
}

// kind 0 = mfcc (tables: basis [400, 512], mel_idx [322, 2], mel_w [322, 8], dct [322, 192], lifter [161]),
// kind 1 = spectrogram (basis [320, 320] with the window folded in). lead = 1: pcm[:, 0] is the sample before
// the first one (a stream's later calls). mode: 0 whole signal, 1 stream in flight, 2 stream end.
void featurize(at::Tensor pcm, OptT lens, at::Tensor offset, at::Tensor gain, at::Tensor basis, OptT mel_idx,
               OptT mel_w, OptT dct, OptT lifter, int64_t kind, int64_t lead, int64_t mode, at::Tensor out,
               at::Tensor frames) {
  const int i16 = pcm_is_i16(pcm);
  const int64_t B = pcm.size(0), S = pcm.size(1);
  TORCH_CHECK(kind == 0 || kind == 1, "featurize: kind 0 (mfcc) or 1 (spectrogram)");
  TORCH_CHECK((lead == 0 || lead == 1) && mode >= 0 && mode <= 2 && S >= lead && S < (1LL << 31), "featurize: lead / mode / S");
  for (const at::Tensor* t : {&offset, &gain, &basis, &out, &frames}) need_gpu(*t, "featurize operand");
  TORCH_CHECK(offset.scalar_type() == at::kFloat && offset.numel() == B && gain.scalar_type() == at::kFloat &&
                  gain.numel() == B, "offset / gain must be fp32 [B]");
  const int64_t L = kind == 0 ? 400 : 320, NCOL = kind == 0 ? 512 : 320;
  TORCH_CHECK(basis.scalar_type() == at::kFloat && basis.numel() == L * NCOL, "featurize: basis must be fp32 [", L, ", ", NCOL, "]");
  TORCH_CHECK(out.dim() == 3 && out.size(0) == B && out.size(2) == 161, "featurize: out must be [B, T_max, 161]");
  TORCH_CHECK(frames.scalar_type() == at::kInt && frames.numel() == B, "frames must be int32 [B]");
  DS2Feat a{};
  a.pcm = pcm.data_ptr();
  a.row_stride = S;
  a.S = (int)S; a.lead = (int)lead; a.mode = (int)mode; a.B = (int)B; a.T_max = (int)out.size(1);
  a.lens = feat_lens(lens, B);
  a.offset = offset.data_ptr<float>();
  a.gain = gain.data_ptr<float>();
  a.basis = basis.data_ptr<float>();
  if (kind == 0) {
    a.mel_idx = ptr_or_null<const int>(mel_idx, "mel_idx");
    a.mel_w = ptr_or_null<const float>(mel_w, "mel_w");
    a.dct = ptr_or_null<const float>(dct, "dct");
    a.lifter = ptr_or_null<const float>(lifter, "lifter");
    TORCH_CHECK(a.mel_idx && a.mel_w && a.dct && a.lifter, "featurize: mfcc needs the mel, DCT and lifter tables");
    TORCH_CHECK(mel_idx->scalar_type() == at::kInt && mel_idx->numel() == 322 * 2 && mel_w->scalar_type() == at::kFloat &&
                    mel_w->numel() == 322 * 8 && dct->scalar_type() == at::kFloat && dct->numel() == 322 * 192 &&
                    lifter->scalar_type() == at::kFloat && lifter->numel() == 161, "featurize: mfcc table shapes");
  }
  a.out = out.data_ptr();
  a.frames = frames.data_ptr<int>();
  check(ds2_featurize(&a, (int)kind, i16, is_bf16(out), cur_stream()), "featurize");
}

// --------------------------------------------------------------------------- resampling (csrc/resample.hip)
// out [B, n_out] fp32 and out_lens [B] int32 of one whole call (in_off = -(K/2 - 1), ph0 = 0, to_end) or of one
// stream push (buffer-relative in_off and start phase)
void resample(at::Tensor pcm, OptT lens, at::Tensor h, int64_t L, int64_t M, int64_t in_off, int64_t ph0,
              bool to_end, at::Tensor out, at::Tensor out_lens) {
  const int i16 = pcm_is_i16(pcm);
  const int64_t B = pcm.size(0), S = pcm.size(1);
  TORCH_CHECK(pcm.is_contiguous() && S < (1LL << 31), "resample: pcm must be contiguous [B, S], S < 2^31");
  for (const at::Tensor* t : {&h, &out, &out_lens}) need_gpu(*t, "resample operand");
  TORCH_CHECK(h.scalar_type() == at::kFloat && h.dim() == 2 && h.is_contiguous() && h.size(0) == L,
              "resample: h must be contiguous fp32 [L, K]");
  const int64_t K = h.size(1);
  TORCH_CHECK(L >= 1 && M >= 1 && ds2_resample_supported((int)L, (int)M, (int)K),
              "resample: (L, M, K) outside the kernel's contract");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && out.size(0) == B && out.is_contiguous() &&
                  out.size(1) < (1LL << 31), "resample: out must be contiguous fp32 [B, n_out]");
  TORCH_CHECK(out_lens.scalar_type() == at::kInt && out_lens.numel() == B, "resample: out_lens must be int32 [B]");
  TORCH_CHECK(in_off > -(1LL << 31) && in_off < (1LL << 31) && ph0 >= 0 && ph0 < L, "resample: in_off / ph0");
  check(ds2_resample(pcm.data_ptr(), i16, S, (int)S, (int)B, feat_lens(lens, B), h.data_ptr<float>(), (int)L, (int)M,
                     (int)K, (int)in_off, (int)ph0, (int)out.size(1), to_end ? 1 : 0, out.data_ptr<float>(),
                     out_lens.data_ptr<int>(), cur_stream()),
        "resample");
}

// --------------------------------------------------------------------------- summaries (csrc/stats.hip)
void hist_stats(at::Tensor x, at::Tensor counts, at::Tensor part) {
  need_gpu(x, "x");
  need_gpu(counts, "counts");
  need_gpu(part, "part");
  TORCH_CHECK(counts.scalar_type() == at::kInt && counts.numel() == ds2_hist_nbucket(), "counts: [nbucket] int32");
  const int blocks = ds2_hist_blocks(x.numel());
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.numel() >= 6 * blocks, "part: [blocks, 6] fp32");
  check(ds2_hist_stats(x.data_ptr(), is_bf16(x), x.numel(), reinterpret_cast<unsigned*>(counts.data_ptr<int>()),
                       part.data_ptr<float>(), blocks, cur_stream()),
        "hist_stats");
}

void nonfinite_watch(at::Tensor loss, at::Tensor counter, at::Tensor first_bad) {
  need_gpu(loss, "loss");
  need_gpu(counter, "counter");
  need_gpu(first_bad, "first_bad");
  TORCH_CHECK(loss.scalar_type() == at::kFloat && loss.numel() == 1, "loss: fp32 scalar");
  TORCH_CHECK(counter.scalar_type() == at::kInt && first_bad.scalar_type() == at::kInt, "int32 words");
  check(ds2_nonfinite_watch(loss.data_ptr<float>(), counter.data_ptr<int>(), first_bad.data_ptr<int>(), cur_stream()),
        "nonfinite_watch");
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
  m.def("spin", [](int64_t ticks, int64_t blocks, int64_t threads, int64_t lds_bytes, at::Tensor done) {
    need_gpu(done, "done");
    TORCH_CHECK(done.scalar_type() == at::kInt, "done: int32");
    check(ds2_spin(ticks, (int)blocks, (int)threads, (int)lds_bytes, done.data_ptr<int>(), cur_stream()), "spin");
  });
}

