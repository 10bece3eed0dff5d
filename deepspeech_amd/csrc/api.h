// The launch ABI of the deepspeech_amd gfx950 kernels: every descriptor and every extern "C"
// launcher that bindings.cpp calls, declared once. common.h includes this file, so each .hip
// file sees the prototype before its own definition and a definition whose parameter list
// differs does not compile ("conflicting types" for a C-linkage name); bindings.cpp includes it
// instead of keeping a copy. Host-safe: no device code, only the runtime API's handle types.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

extern "C" {

// ---- fill.hip ---------------------------------------------------------------------------
// Buffers the NEXT kernel of a stream needs initialised (a recurrence's h0 slots, sentinel-
// filled exchange slots, census words, bias partials): written by a persistent GEMM launch's
// lighter workgroups (one work unit fewer than the busiest) after their last unit, while the
// others finish theirs, instead of by a separate multi_fill launch on the critical path
// (csrc/fill.hip semantics: region r = words[r] 32-bit words of pattern[r]).
struct DS2Fill {
  int n;
  unsigned* ptr[8];
  unsigned long long words[8];
  unsigned pattern[8];
};

// Completion event armed for the next launch made through ds2_launch (common.h)
hipEvent_t ds2_take_stop_event();
void ds2_arm_stop_event(hipEvent_t e);

int ds2_multi_fill(int n, void* const* ptrs, const unsigned long long* bytes, const unsigned* patterns,
                   hipStream_t st);
int ds2_multi_copy(int n, void* const* dst, const void* const* src, const unsigned long long* rows,
                   const unsigned* src_row, const unsigned* dst_row, const unsigned* src_pitch,
                   const unsigned* dst_pitch, float* sdst, const float* svals, int ns, hipStream_t st);
int ds2_wait_resident(const unsigned* word, long long timeout, hipStream_t st);
int ds2_prep_inputs(const float* x, void* y, long long n, const int* lens_in, int* lens_out, int nl,
                    hipStream_t st);
int ds2_transpose_bf16(const void* in, void* out, int R, int C, int ldi, int ldo, hipStream_t st);

// ---- the recurrences ---------------------------------------------------------------------
// Geometry every recurrence descriptor starts with, in the order ops/rnn.py _geom builds it
// (generation 1 leaves R, xcd_map and knobs 0; the fp8 kernels are GRU only and take no knobs).
struct DS2RnnGeom {
  int T, N, NP, H, BG, R, steps, gstride, ndir, xcd_map, cell, knobs;
};

// ---- rnn_persistent.hip (and its timestamped build, rnn_persistent_stamps.hip) ------------
// Python-visible descriptors (flat, fixed-layout structs filled by the bindings).
struct DS2RnnFwd : DS2RnnGeom {
  int S, nw, mt, persistent;
  const int* lens;
  const void* gx;
  const void* U[2];
  const float* bh[2];
  void* y[2];
  void* hx[2];
  float* hsave[2];
  float* gates[2];
  unsigned* flags;
  unsigned* err;
  long long timeout;
  unsigned long long* stamps;
};

struct DS2RnnBwd : DS2RnnGeom {
  int S, nw, mt, persistent;
  const int* lens;
  const void* dy;
  const void* U[2];
  const float* hsave[2];
  const float* gates[2];
  void* dgh[2];
  void* dgx;
  float* carry[2];
  float* dbx_part[2];
  float* dbh_part[2];
  float dgx_scale;
  unsigned* flags;
  unsigned* err;
  long long timeout;
  unsigned long long* stamps;
};

int ds2_rnn_kpw(int H, int G, int nw, int fwd);
int ds2_rnn_fwd(const DS2RnnFwd* d, hipStream_t st);
int ds2_rnn_bwd(const DS2RnnBwd* d, hipStream_t st);
int ds2_rnn_kpw_stamps(int H, int G, int nw, int fwd);
int ds2_rnn_fwd_stamps(const DS2RnnFwd* d, hipStream_t st);
int ds2_rnn_bwd_stamps(const DS2RnnBwd* d, hipStream_t st);

// ---- rnn_xcd.hip ------------------------------------------------------------------------
struct DS2RnnX : DS2RnnGeom {
  const int* lens;
  const void* gx;        // fwd: gx;  bwd: dy
  const void* U[2];
  const float* bh[2];
  void* y[2];            // fwd: y
  void* ex[2];           // fwd: hx exchange;  bwd: dgh exchange
  float* hsave[2];
  float* gates[2];
  void* dgx;
  float* dbx_part[2];
  float* dbh_part[2];
  float dgx_scale;
  unsigned* census;
  unsigned* err;
  long long timeout;
  unsigned long long* stamps;
  void* ring[2];         // bwd reduce-scatter exchange ring (fp32, sentinel-filled)
  void* ysum;            // fwd gen 4: fused direction sum (sentinel-filled) or null
};

int ds2_rnnx_fwd(const DS2RnnX* d, hipStream_t st);
int ds2_rnnx_bwd_rs(const DS2RnnX* d, hipStream_t st);
int ds2_rnnx_members(int H, int cell);
int ds2_rnnx_fwd_fuses_sum(int H, int cell, int ndir, int knobs);
int ds2_rnnx_fwd_family(int H, int cell, int knobs);
int ds2_rnnx_bwd_family(int H, int cell, int R);
long long ds2_rnnx_ring_floats(int H, int BG, int R);
int ds2_rnnx_grid(int H, int cell, int ngroups, int xcd_map);

// ---- rnn_fp8.hip ------------------------------------------------------------------------
struct DS2RnnF8 : DS2RnnGeom {
  const int* lens;
  const void* gx;
  const void* U8[2];
  const int* uexp;
  const float* bh[2];
  void* y[2];
  void* hq[2];
  void* hx[2];
  float* hsave[2];
  float* gates[2];
  unsigned* census;
  unsigned* err;
  long long timeout;
};

struct DS2RnnF8B : DS2RnnGeom {
  const int* lens;
  const void* dy;
  const void* U8T[2];
  const int* uexp;
  const float* hsave[2];
  const float* gates[2];
  void* dgh[2];
  void* dgx;
  void* ring[2];
  float* dbx_part[2];
  float* dbh_part[2];
  float dgx_scale;
  unsigned* census;
  unsigned* err;
  long long timeout;
};

int ds2_rnnf8_supported(int H, int N, int ndir);
size_t ds2_rnnf8_smem(int H);
int ds2_rnnf8_fwd(const DS2RnnF8* d, hipStream_t st);
int ds2_rnnf8_bwd_supported(int H, int N, int ndir);
long long ds2_rnnf8_ring_words(int H, int BG, int R);
int ds2_rnnf8_bwd(const DS2RnnF8B* d, hipStream_t st);
int ds2_fp8_quant_u(int ndir, const void* const* x, int rows, int cols, void* const* q, void* const* qt, int* uexp,
                    float* part, hipStream_t st);
int ds2_fp8_quant_pow2_t(const void* x, int rows, int cols, void* q, int* uexp, unsigned* amax, hipStream_t st);
int ds2_fp8_quant_pow2(const void* x, long long n, void* q, int* uexp, unsigned* amax, hipStream_t st);

// ---- gemm.hip, gemm8.hip, quant.hip -----------------------------------------------------
int ds2_gemm(const void* A, const void* B, void* C, const void* bias, const float* alpha_dev, int M, int N, int K,
             int lda, int ldb, int ldc, int Ml, int Nl, int Kl, int a_col, int b_col, int epi, float alpha, int batch,
             long long sA, long long sB, long long sC, int cfg, const DS2Fill* fill, hipStream_t st);
int ds2_gemm_tile(int cfg, int* bm, int* bn);
int ds2_gemm8(const void* A, const void* B, void* C, const void* bias, const float* alpha_dev,
              const float* alpha_dev2, int M, int N, int K, int lda, int ldb, int ldc, int fp8, int a_col, int b_col,
              int epi, float alpha, int batch, long long sA, long long sB, long long sC, int S, float* ws,
              unsigned* cnt, int cus, const DS2Fill* fill, int ext_red, hipStream_t st);
int ds2_gemm8_group(int np, const void* const* A, const void* const* B, void* const* C, float* const* ws,
                    unsigned* const* cnt, const int* dims, int a_col, int b_col, int cus, hipStream_t st);
int ds2_gemm8_splits(int K, int fp8, int S);
int ds2_fp8_quant_blocks(long long na, long long nb_el);
int ds2_fp8_quant2(const void* a, long long rows_a, const void* b, long long rows_b, int K, int Kp, float alpha,
                   void* a8, void* b8, float* part, float* scales, const void* a2, void* asum, hipStream_t st);

// ---- ctc.hip, decode.hip, beam.hip ------------------------------------------------------
int ds2_ctc_fused(const void* logits, int logits_bf16, const int* lens, const int* labels, const int* label_lens,
                  float* loss, void* grad, float* ws, int T, int N, int K, int Lmax, int blank, int zero_inf,
                  hipStream_t st);
long long ds2_ctc_ws_floats(int T, int N, int Lmax);
int ds2_head_ctc(const void* h, const void* W, const void* bias, const int* lens, const int* labels,
                 const int* label_lens, float* loss, void* G, float* ws, int T, int N, int H, int K, int Lmax,
                 int blank, int zero_inf, float* mean, int* counter, int* first_bad, hipStream_t st);
int ds2_nonfinite_watch(const float* loss, int* counter, int* first_bad, hipStream_t st);
int ds2_fc_logits(const void* h, const void* W, const void* bias, void* logits, int out_bf16, int M, int H, int K,
                  hipStream_t st);
int ds2_ctc_greedy(const void* logits, int bf16, const int* lens, int T, int N, int K, int blank,
                   int* labels, int* counts, float* score, hipStream_t st);
// key [B][W][2]: 64-bit fingerprints of each hypothesis' prefix and of its parent's, the beams'
// prefix identity (zero at reset; csrc/beam.hip). -51: no key buffer.
int ds2_ctc_beam(const float* lp, const int* frames, int T, int B, int K, int W, int blank, float prune, int* node,
                 int* last, int* parent, float* pb, float* pnb, int* nbeam, void* nodes, int* nnodes, int cap,
                 unsigned* err, unsigned long long* key, hipStream_t st);
int ds2_ctc_beam_backtrack(const void* nodes, int cap, const int* node, const int* nbeam, const float* pb,
                           const float* pnb, int B, int W, int* out, int* out_len, float* score, int Lcap,
                           hipStream_t st);
// LM shallow fusion: lm [S][K] int2 rows (w fp32 bits, next state), lmstate [B][W] int32, key as
// above; the backtrack adds the </s> weight (column blank) to every score (final mode). -51: bad
// LM arguments.
int ds2_ctc_beam_lm(const float* lp, const int* frames, int T, int B, int K, int W, int blank, float prune, int* node,
                    int* last, int* parent, float* pb, float* pnb, int* nbeam, void* nodes, int* nnodes, int cap,
                    unsigned* err, const void* lm, int S, int* lmstate, unsigned long long* key, hipStream_t st);
int ds2_ctc_beam_backtrack_lm(const void* nodes, int cap, const int* node, const int* nbeam, const float* pb,
                              const float* pnb, int B, int W, int* out, int* out_len, float* score, int Lcap,
                              const void* lm, int S, int K, int blank, const int* lmstate, hipStream_t st);

// ---- align.hip --------------------------------------------------------------------------
// CTC forced alignment (Viterbi path + backtrack). em [T, N, K] fp32 / bf16 (log_probs != 0: used
// as they are, else log-softmaxed), labels [N, Lmax] (Lmax >= 1); outputs path [N, T],
// tok_start / tok_end / tok_score [N, Lmax], score [N]; ws of ds2_ctc_align_ws_bytes bytes.
// Returns -20 for K > 32, -21 for 2*Lmax+1 > 2048 (ws_bytes: -1), -22 for a blank outside [0, K).
long long ds2_ctc_align_ws_bytes(int T, int N, int Lmax);
int ds2_ctc_align(const void* em, int em_bf16, int log_probs, const int* lens, const int* labels,
                  const int* label_lens, int* path, int* tok_start, int* tok_end, float* tok_score, float* score,
                  void* ws, int T, int N, int K, int Lmax, int blank, hipStream_t st);

// ---- bn_act.hip -------------------------------------------------------------------------
int ds2_bn_stats(const void* y, int y_bf16, int N, int C, int T, int F, float* part, int nb, float eps, float* mean,
                 float* invstd, float* run_mean, float* run_var, float momentum, hipStream_t st);
int ds2_bn_chunks(int N, int T, int F);
int ds2_bn_apply(const void* y, int y_bf16, const float* mean, const float* invstd, const float* gamma,
                 const float* beta, void* out, int out_bf16, int N, int C, int T, int F, int layout, hipStream_t st);
int ds2_bn_bwd(const void* dout, int dout_bf16, const void* y, int y_bf16, const float* mean, const float* invstd,
               const float* gamma, const float* beta, float* part, int nb, float* dgamma, float* dbeta, void* dy,
               int dy_bf16, int N, int C, int T, int F, int layout, hipStream_t st);

// ---- optim.hip, reduce.hip, stats.hip ---------------------------------------------------
int ds2_adam_ema(float* p, const float* g, float* m, float* v, float* ema, void* p16, long long n, float lr_t,
                 float b1, float b2, float eps, float gscale, float ema_keep, const int* skip, int max_grid,
                 const float* hyper, int lds_reserve, const float* clip, hipStream_t st);
int ds2_adam_ema_ranges(float* p, const float* g, float* m, float* v, float* ema, void* p16, const long long* lohi,
                        int nr, float lr_t, float b1, float b2, float eps, float gscale, float ema_keep,
                        const float* hyper, const float* clip, hipStream_t st);
int ds2_grad_norm_blocks(long long n);
int ds2_grad_norm(const float* g, long long n, float gscale, float* part, int nblocks, int* bad, hipStream_t st);
// gradient-norm clipping: per-segment partial sums of squares, then {S, norm, coef, bad, steps,
// clipped_steps, skipped_steps, spare} (ds2_clip_state_words() 4-byte words) read by the updates
// that are given the state as `clip`
int ds2_grad_sumsq_segment(void);
int ds2_clip_state_words(void);
int ds2_grad_sumsq(const float* g, long long n, float gscale, float* part, int max_grid, int nontemporal,
                   hipStream_t st);
int ds2_clip_finalize(const float* part, long long nseg, float max_norm, float* state, hipStream_t st);
int ds2_cast_bf16(const float* x, void* y, long long n, hipStream_t st);
int ds2_col_sum(int n, const float* const* in, float* const* out, const int* R, const int* B, const int* C,
                const int* acc, hipStream_t st);
int ds2_fc_bias_grad(const void* G, int M, int ldg, int K, const float* scale, float alpha, float* out, int acc,
                     hipStream_t st);
int ds2_hist_nbucket();
int ds2_hist_npos();
int ds2_hist_blocks(long long n);
int ds2_hist_stats(const void* x, int bf16, long long n, unsigned* counts, float* part, int blocks, hipStream_t st);
int ds2_spin(long long ticks, int blocks, int threads, int lds_bytes, int* done, hipStream_t st);

// ---- lookahead.hip ----------------------------------------------------------------------
// Lookahead (row) convolution: x, out bf16 [T, B, H] (H % 8 == 0, 16-B aligned), w bf16
// [H, tau+1], 1 <= tau <= 31, lens [B]. bwd = 0: out = r from x = h; bwd = 1: out = dh from
// x = dr. The weight gradient writes ds2_lookahead_wgrad_parts fp32 partials [P, H*(tau+1)] for
// ds2_col_sum. The streaming step reads hist [tau, B, H] and x [n, B, H], writes out [n, B, H]
// and rewrites hist. -60: shape outside the contract, -61: misaligned base, -62: weights
// beyond the LDS.
int ds2_lookahead(const void* x, const void* w, const int* lens, void* out, int T, int B, int H, int tau, int bwd,
                  hipStream_t st);
int ds2_lookahead_stream(void* hist, const void* x, const void* w, void* out, int n, int B, int H, int tau,
                         hipStream_t st);
int ds2_lookahead_wgrad_tpw(int T, int B, int H);
int ds2_lookahead_wgrad_parts(int T, int B, int H);
int ds2_lookahead_wgrad(const void* dr, const void* h, const int* lens, float* part, int T, int B, int H, int tau,
                        hipStream_t st);

// ---- specaug.hip ------------------------------------------------------------------------
// SpecAugment on stored frames: x, out fp32 [B, T, F] (1 <= F <= 1024, 1 <= T <= 32767, B <= 65535),
// lens int32 [B], plan int32 [B, 2 + 2 nF + 2 nT] = (w0, w, f0, fw, ..., t0, tw, ...), mean fp32
// [B, F] or null (fill = zero). The plan kernel draws from Philox4x32-10 with key seed, counter
// (block, first_utt + b, step) and takes any T, F >= 1. In place (x == out, plans without a warp
// only) nothing is read and only masked cells of frames < lens are written. -70: shape outside
// the contract, -71: policy outside its range (nF <= 8, nT <= 16, p_ppm <= 1000000), -72: inplace
// set without x == out, or x == out without it.
int ds2_specaug_plan(const int* lens, int* plan, int B, int T, int F, int nF, int Fw, int nT, int Tw, int p_ppm,
                     int W, unsigned seed_lo, unsigned seed_hi, unsigned step_lo, unsigned step_hi,
                     unsigned first_utt, hipStream_t st);
int ds2_specaug_mean(const float* x, const int* lens, float* mean, int B, int T, int F, hipStream_t st);
int ds2_specaug_apply(const float* x, const int* lens, const int* plan, const float* mean, float* out, int B, int T,
                      int F, int nF, int nT, int inplace, hipStream_t st);

// ---- dropout.hip ------------------------------------------------------------------------
// Dropout between recurrent layers: x, out bf16 [T, N, H] (H % 8 == 0, H <= 2^19, 16-B aligned,
// T * N * H / 8 < 2^31); out == x runs in place. ctr int32 [2] on the device = (step, first_utt)
// mod 2^32, read by the kernel. Element (t, b, i) is kept iff 16 bits of the Philox4x32-10 block
// with key seed and counter (locked ? 0 : t, first_utt + b, step, 0x80000000 | locked << 30 |
// site << 16 | i >> 3) are >= thr; kept: bf16(x * scale), dropped: +0. -80: shape outside the
// contract, -81: misaligned, -82: site >= 16384, thr outside [1, 65535] or scale < 1.
int ds2_seq_dropout(const void* x, void* out, const int* ctr, int T, int N, int H, unsigned seed_lo,
                    unsigned seed_hi, int site, int thr, float scale, int locked, hipStream_t st);

// ---- conv1.hip, conv2.hip, bn_cl.hip (shared layer: conv_common.h, bn_math.h) -----------
// optional BatchNorm-backward apply fused into conv1's weight-gradient staging
struct DS2Conv1WgradBn {
  const void *dz, *y1;                             // bf16 [N][T1][F1][32]
  const float *mean, *invstd, *gamma, *beta, *dbeta, *dgamma;
};

// optional BatchNorm-backward sums fused into the conv2 data-gradient epilogue
struct DS2Conv2DgradBn {
  const void* y1;                                  // conv1 output [N][T1][F1][32] bf16
  const float *mean, *invstd, *gamma, *beta;       // conv1 BN batch statistics and affine
  float* part;                                     // [grid][32][2]
};

// what a negative return code of the launchers below refused (ConvStatus in conv_common.h); null
// for any other code
const char* ds2_conv_status_str(int rc);
size_t ds2_conv2_fwd_smem(int F1);
size_t ds2_conv2_dgrad_smem(int F2);
size_t ds2_conv2_wgrad_smem(int F1);
long long ds2_conv2_wgrad_part_floats(int grid);
long long ds2_conv1_wgrad_part_floats(int grid);
int ds2_conv1_fwd_grid(int N, int T1);
int ds2_conv1_fwd(const void* x, const void* w, const float* bias, void* y, float* part, int N, int T, int F0,
                  int T1, int F1, hipStream_t st);
int ds2_conv2_fwd(const void* x, const void* w, const float* bias, void* y, float* part, int grid, int N, int T1,
                  int F1, int T2, int F2, long long* trace, hipStream_t st);
int ds2_conv2_dgrad(const void* dy, const void* w, void* dx, int grid, int N, int T1, int F1, int T2, int F2,
                    const DS2Conv2DgradBn* bn, long long* trace, hipStream_t st);
int ds2_conv2_wgrad(const void* dy, const void* x, float* part, int grid, float* dw, int N, int T1, int F1, int T2,
                    int F2, hipStream_t st);
int ds2_conv1_wgrad(const void* dy, const void* x, float* part, int grid, float* dw, int N, int T, int F0, int T1,
                    int F1, const DS2Conv1WgradBn* bn, hipStream_t st);
int ds2_bn_cl_finalize(const float* part, int nb, double M, float eps, float* mean, float* invstd, float* run_mean,
                       float* run_var, float momentum, hipStream_t st);
int ds2_bn_cl_apply(const void* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                    void* out, int N, int T, int F, int tmaj, hipStream_t st);
int ds2_bn_cl_bwd(const void* dz, const void* y, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, float* part, int nb, float* dgamma, float* dbeta, void* dy, int N, int T, int F,
                  int tmaj, int part_ready, hipStream_t st);

// ---- featurize.hip ----------------------------------------------------------------------
struct DS2Feat {
  const void* pcm;        // [B, row_stride] samples; logical sample n of row b is pcm[b][lead + n]
  long long row_stride;
  int S, lead, mode, B, T_max;
  const int* lens;        // [B] valid logical samples, or null (= S - lead)
  const float* offset;    // [B]
  const float* gain;      // [B]
  const float* basis;     // [L, 2 * NH]
  const int* mel_idx;     // [322, 2] (first bin, taps)           (mfcc)
  const float* mel_w;     // [322, 8]                             (mfcc)
  const float* dct;       // [322, 192], columns >= 161 zero      (mfcc)
  const float* lifter;    // [161]                                (mfcc)
  void* out;              // [B, T_max, 161]
  int* frames;            // [B]
};

int ds2_audio_stats(const void* pcm, int in_i16, long long row_stride, int S, int B, const int* lens, float* offset,
                    float* gain, hipStream_t st);
int ds2_featurize(const DS2Feat* a, int kind, int in_i16, int out_bf16, hipStream_t st);

// ---- resample.hip ------------------------------------------------------------------------
// Polyphase resampling of PCM rows: x fp32 / int16 [B, S] (rows row_stride samples apart), lens
// [B] valid samples or null, h fp32 [L, K] (K even, K <= 320, L * K <= 24576), out fp32
// [B, n_out], out_lens int32 [B]. Output j reads x[in_off + (ph0 + j M) / L + k], k < K, with
// phase (ph0 + j M) % L; to_end: a row's outputs stop with its samples (else every row has
// n_out). -90: shape outside the contract, -91: in_off / ph0 outside their ranges.
int ds2_resample_tile();
int ds2_resample_supported(int L, int M, int K);
int ds2_resample(const void* x, int in_i16, long long row_stride, int S, int B, const int* lens, const float* h,
                 int L, int M, int K, int in_off, int ph0, int n_out, int to_end, float* out, int* out_lens,
                 hipStream_t st);

// ---- waveaug.hip -------------------------------------------------------------------------
// Additive noise at a random SNR on the waveform: x fp32 / int16 [B, S] contiguous and 16-byte
// aligned (S % 8 == 0, 8 <= S < 2^30, B <= 65535), lens int32 [B] or null, bank = data fp32
// [Ntot < 2^31] with start, length int32 [C], plan int32 [B, 4] = (on, clip, off, snr_cdb), part
// fp32 [B, ceil(S / ds2_waveaug_segment()), 2], energy fp64 [B, 2] = (Ex, En), coef fp32 [B], out
// fp32 [B, S]. The plan kernel draws from Philox4x32-10 with key seed and counter (0, first_utt
// + b, step_lo, 0x40000000 | step_hi & 0x3fffffff) and takes any S >= 1. Bank and plan words are
// clamped into the bank on the device. -120: shape outside the contract, -121: policy outside
// its range (p_ppm <= 1000000, |snr| <= 2^20 centi-dB, lo <= hi), -122: misaligned.
int ds2_waveaug_segment();
int ds2_waveaug_plan(const int* lens, const int* length, int* plan, int B, int S, int C, int p_ppm, int snr_lo_cdb,
                     int snr_hi_cdb, unsigned seed_lo, unsigned seed_hi, unsigned step_lo, unsigned step_hi,
                     unsigned first_utt, hipStream_t st);
int ds2_waveaug_energy(const void* x, int in_i16, const int* lens, const int* plan, const float* data,
                       const int* start, const int* length, int C, long long Ntot, float* part, int B, int S,
                       hipStream_t st);
int ds2_waveaug_coef(const int* lens, const int* plan, const float* part, double* energy, float* coef, int B, int S,
                     hipStream_t st);
int ds2_waveaug_apply(const void* x, int in_i16, const int* lens, const int* plan, const float* coef,
                      const float* data, const int* start, const int* length, int C, long long Ntot, float* out, int B,
                      int S, hipStream_t st);

// ---- speed.hip ---------------------------------------------------------------------------
// Speed perturbation: every row of x fp32 / int16 [B, S] (contiguous, S < 2^30, B <= 65535) is
// resampled by its own variant of a policy of V <= 8 distinct percents, or copied (100 %). The
// policy travels by value: variant v with pct != 100 has L * pct == M * 100, K even, (L, M, K)
// inside csrc/resample.hip's contract, and its table h[off .. off + L * K) in the coefficient
// array (off % 4 == 0); a 100 % record has L = M = 1, K = 0, off = 0. plan int32 [B, 2] =
// (pct, n_out); lens, min_out int32 [B] or null; max_out 0: none. The plan kernel draws variant
// U(x0, V) from the Philox4x32-10 block with key seed and counter (1, first_utt + b, step_lo,
// 0x40000000 | step_hi & 0x3fffffff) and falls back to (100, n) when n == 0 or the candidate
// count ceil(n L / M) is below min_out[b] or above max_out. The apply kernel writes out fp32
// [B, n_out] and out_lens int32 [B]; plan words are clamped on the device (an unknown percent
// copies, a count stops at n_out). -130: shape outside the contract, -131: policy outside it,
// -132: n_out below ds2_speed_out_width when the caller did not vouch for it.
struct DS2SpeedTable {
  int V;
  int pct[8], L[8], M[8], K[8], off[8];
};

int ds2_speed_tile();
int ds2_speed_supported(const DS2SpeedTable* t, long long h_words);
long long ds2_speed_out_width(const DS2SpeedTable* t, long long S);   // worst case, a multiple of 160
int ds2_speed_plan(const int* lens, const int* min_out, int* plan, int B, int S, int max_out, const DS2SpeedTable* t,
                   unsigned seed_lo, unsigned seed_hi, unsigned step_lo, unsigned step_hi, unsigned first_utt,
                   hipStream_t st);
int ds2_speed_apply(const void* x, int in_i16, int B, int S, const int* lens, const int* plan, const float* h,
                    long long h_words, const DS2SpeedTable* t, float* out, int n_out, int tight, int* out_lens,
                    hipStream_t st);

}  // extern "C"
