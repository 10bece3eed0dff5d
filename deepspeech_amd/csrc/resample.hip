// Polyphase windowed-sinc resampling of PCM rows (ops/resample.py; oracle: ops/reference.py
// resample_ref). Rates in -> out reduce to L = out / gcd, M = in / gcd; output j of a launch has
// t = ph0 + j * M (64 bits, formed once), q = t / L, ph = t % L and
//   y[j] = sum_{k = 0 .. K-1} h[ph, k] * x[in_off + q + k]
// as one chain of fp32 fma in ascending k from +0, with x outside [0, len) read as +0 by
// selection while the tile is staged, so nothing past a row's length (garbage, NaN) reaches an
// output. in_off is the buffer index of tap 0 of output 0 (negative: the left zero padding) and
// ph0 the phase of output 0: a whole call passes (-(K/2 - 1), 0), a stream push its buffer-
// relative values, so every output is the same chain over the same values however the signal
// was chunked.
//
// One workgroup per (row, grid.x-strided tiles of TILE_OUT outputs). The coefficient table sits in
// LDS for the workgroup's whole life; with L = 1 every lane multiplies by the same word, which
// the UNI instantiation reads through the scalar cache instead (no table in LDS, half the LDS
// reads). The LDS layout, the staging of the table and of each tile's input span (at most
// (TILE_OUT - 1) * M / L + K + 1 samples, staged once) and the chain live in resample_tile.h,
// which csrc/speed.hip shares. Columns at or past a row's count are written as zeros and
// out_lens[b] by the same launch. No atomics, no MFMA (the ascending-k chain is the definition),
// nothing read back: the launch can be captured in a graph.
#include "resample_tile.h"

using namespace ds2;

namespace {

struct RsArgs {
  const void* x;
  long long row_stride;     // samples between rows
  int S, B;                 // row width of the buffer, rows
  const int* lens;          // [B] valid samples of the buffer, or null (= S)
  const float* h;           // [L, K]
  int L, M, K;
  int in_off, ph0;
  int n_out, to_end;        // out is [B, n_out]; to_end: a row's count stops where its samples do
  int span;                 // floats of LDS for a tile's input span
  float* out;
  int* out_lens;            // [B]
};

template <typename IN, bool UNI>
__global__ __launch_bounds__(rs::THREADS) void resample_kernel(RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int L = a.L, M = a.M, K = a.K;
  float* hs = rs_lds;                                  // [L][K + 1]
  float* xs = rs_lds + rs::table_words(L, K);          // [span], 16-byte aligned

  int len = a.lens ? a.lens[b] : a.S;
  len = max(0, min(len, a.S));
  // outputs of this row: j counts while the centre sample in_off + K/2 - 1 + q_j is a valid one
  int cnt = a.n_out;
  if (a.to_end) {
    const long long num = ((long long)len - ((long long)a.in_off + K / 2 - 1)) * L - a.ph0;
    const long long c = num <= 0 ? 0 : (num + M - 1) / M;
    cnt = (int)min((long long)a.n_out, c);
  }
  if (blockIdx.x == 0 && tid == 0) a.out_lens[b] = cnt;

  const IN* xrow = reinterpret_cast<const IN*>(a.x) + (long long)b * a.row_stride;
  const rs::Filter f{a.h, L, M, K, a.in_off, a.ph0, a.span};
  const rs::Row<IN> w{xrow, (reinterpret_cast<uintptr_t>(xrow) & 15) == 0, a.S, len,
                      a.out + (long long)b * a.n_out, a.n_out, cnt};
  const int ntiles = (a.n_out + rs::TILE - 1) / rs::TILE;
  bool table = false;

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int j0 = t * rs::TILE;
    if (j0 >= cnt) {                                   // padding only
      rs::zero_tile(w.out, j0, a.n_out);
      continue;
    }
    if (!UNI && !table) {
      rs::stage_table(hs, a.h, L, K);
      table = true;
    }
    rs::tile<IN, UNI>(f, w, hs, xs, j0);
  }
}

}  // namespace

extern "C" int ds2_resample_tile() { return rs::TILE; }

// 1 when (L, M, K) lies inside the kernel's contract
extern "C" int ds2_resample_supported(int L, int M, int K) { return rs::supported(L, M, K); }

// x [B, S] fp32 / int16 rows row_stride samples apart, h fp32 [L, K], out fp32 [B, n_out],
// out_lens int32 [B]. -90: shape outside the contract, -91: in_off / ph0 outside their ranges.
extern "C" int ds2_resample(const void* x, int in_i16, long long row_stride, int S, int B, const int* lens,
                            const float* h, int L, int M, int K, int in_off, int ph0, int n_out, int to_end,
                            float* out, int* out_lens, hipStream_t st) {
  if (B <= 0) return 0;
  if (!ds2_resample_supported(L, M, K) || B > 65535 || S < 0 || n_out < 0 || row_stride < S) return -90;
  if (ph0 < 0 || ph0 >= L || in_off < -(K / 2 - 1) || (long long)n_out * M / L + (long long)in_off > (1LL << 31))
    return -91;
  RsArgs a{};
  a.x = x; a.row_stride = row_stride; a.S = S; a.B = B; a.lens = lens; a.h = h;
  a.L = L; a.M = M; a.K = K; a.in_off = in_off; a.ph0 = ph0; a.n_out = n_out; a.to_end = to_end;
  a.span = rs::span_words(L, M, K);
  a.out = out; a.out_lens = out_lens;
  const int lds = (rs::table_words(L, K) + a.span) * 4;
  static bool attr = false;
  if (!attr) {
    for (const void* kern : {(const void*)resample_kernel<float, false>, (const void*)resample_kernel<short, false>,
                             (const void*)resample_kernel<float, true>, (const void*)resample_kernel<short, true>})
      DS2_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, rs::MAX_LDS));
    attr = true;
  }
  // a workgroup keeps its table across the tiles it walks: about 2048 workgroups per launch
  const int ntiles = (n_out + rs::TILE - 1) / rs::TILE;
  const int gx = max(1, min(ntiles, (2048 + B - 1) / B));
  const bool uni = L == 1;
  if (uni && in_i16) hipLaunchKernelGGL((resample_kernel<short, true>), dim3(gx, B), dim3(rs::THREADS), lds, st, a);
  else if (uni) hipLaunchKernelGGL((resample_kernel<float, true>), dim3(gx, B), dim3(rs::THREADS), lds, st, a);
  else if (in_i16) hipLaunchKernelGGL((resample_kernel<short, false>), dim3(gx, B), dim3(rs::THREADS), lds, st, a);
  else hipLaunchKernelGGL((resample_kernel<float, false>), dim3(gx, B), dim3(rs::THREADS), lds, st, a);
  return (int)hipGetLastError();
}
