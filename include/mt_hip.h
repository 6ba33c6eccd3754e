/* mt_hip.h -- C ABI of libmt_hip.so, the MI355X (gfx950) hot path of
 * cs4247/music-transcription:  30 s waveform chunk -> log-mel -> CNN-RNN -> 88-pitch logits.
 *
 * The reference has no FFI layer (it is pure Python on torch); each entry point
 * below names the reference call site whose arithmetic it replaces.  The Python
 * host (music-transcription_amd/) binds these with ctypes; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensor
 *     .data_ptr()), row-major contiguous, unless the name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - return value: 0 on success, negative MT_E* on error, never throws; the
 *     message of the last error on the calling thread is at mt_last_error();
 *   - no entry point allocates device memory or synchronises the device: scratch
 *     comes in as (workspace, workspace_bytes), sizes come from the *_bytes queries;
 *   - thread-compatible (one stream per caller thread); the only mutable global state is the mutex-protected table of
 *     persistent launches in flight (below).
 *
 * Persistent launches.  The LSTM recurrence kernels (mt_lstm_bidir_fwd*, mt_lstm_bidir_bwd*) wait on their own
 * workgroups, so all workgroups of all such launches in flight on a GPU must be resident together.  Launches on one
 * stream run in order; for launches on DIFFERENT streams the library checks at launch time that their CUs (workgroups /
 * occupancy per CU) fit the device and otherwise returns MT_EUNSUPPORTED at once -- it never queues a launch that could
 * stall the others (every in-kernel spin is bounded as well and reports through the status word of its sync workspace).
 * At hidden 512, batch <= 32: six plain forward recurrences, two with the fused input projection.
 */
#ifndef MT_HIP_H
#define MT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MT_OK            0
#define MT_EINVAL       -1   /* bad argument / unsupported shape                 */
#define MT_EWORKSPACE   -2   /* workspace too small                              */
#define MT_EHIP         -3   /* HIP runtime error (launch, memset, ...)          */
#define MT_EUNSUPPORTED -4   /* configuration outside what the kernels implement */

/* 16-bit operand type of the GEMM / convolution kernels (`_dt` entry points, mt_cnnrnn*_weights.operand_dtype).
 * Both run at the same MFMA rate with f32 accumulation.  Inference uses f16 (11 significand bits: logits within
 * ~1e-3 relative of the reference's fp32 arithmetic); the training step uses bf16 (f32's
 * exponent range for gradients; BASELINE configs[3] names bf16).  The un-suffixed entry points are the bf16 forms. */
#define MT_DT_BF16 0
#define MT_DT_F16  1
/* Flag OR-ed into `dt` of mt_gemm_lstm_gx_dt and into `flags` of mt_lstm_bidir_fwd_ex: the gate pre-activations
 * travel between the two as f16 -- same [group][t][dir][unit/8][gate][unit%8][chunk%32] layout, half the bytes of the largest
 * intermediate of the forward (492 -> 246 MB per layer at B = 32); round-to-nearest-even of W_ih x + b, added in f32 by the
 * cell update.  Inference only (the training step keeps its gates in f32).                                                  */
#define MT_GX_F16  0x10

#define MT_N_FFT 2048        /* librosa default the reference relies on (main.py:117-122) */
#define MT_N_PITCH 88

typedef void* mt_stream_t;

int         mt_version(void);
const char* mt_last_error(void);
/* Number of HIP devices visible, or negative error.  Does not create a context. */
int         mt_device_count(void);
/* Makes `device` current for the calling thread and checks that it is a gfx950 part (the only code object in the library).  No global
 * tables are built (plans and packed weights are caller-owned buffers), so calling it is optional; idempotent.  (mt_init.) */
int         mt_init(int device);
/* One size query for the path's scratch / intermediate buffers (mt_workspace_bytes(kind, dims...)): forwards to the per-buffer
 * queries below.  kind = MT_WS_*; MT_WS_MEL_PLAN takes n_mels in B; unknown kind -> 0 and mt_last_error().                          */
#define MT_WS_LSTM_GX        1
#define MT_WS_LSTM_HX        2
#define MT_WS_LSTM_CX        3
#define MT_WS_LSTM_SYNC      4
#define MT_WS_LSTM_BWD_PART  5
#define MT_WS_LSTM_DGX       6
#define MT_WS_MEL_PLAN       7
#define MT_WS_ADAM           8
size_t      mt_workspace_bytes(int kind, int B, int T, int H);
/* In-place SUM all-reduce of `count` elements over the ranks of the caller's RCCL communicator (`comm` = ncclComm_t), queued on `stream`:
 * the gradient step of data-parallel training (train/train_transcriber.py has none: single GPU; BASELINE configs[3]) for a host that is
 * not Python -- the flat gradient buffer, then mt_adam_clip_step_ex with grad_scale = 1 / world.  RCCL is opened on first use
 * (librccl.so.1), not linked.  The Python host uses torch.distributed instead.                          */
#define MT_AR_F32   0
#define MT_AR_BF16  1
#define MT_AR_F16   2
int         mt_allreduce(void* buf, size_t count, int dtype, void* comm, mt_stream_t stream);

/* ------------------------------------------------------------------ frontend
 * Replaces librosa.feature.melspectrogram + librosa.power_to_db as called at
 * main.py:117-125, data/dataset.py:155-156 and :195-196:
 *   center zero-pad n_fft/2, frames of 2048 @ hop, periodic Hann, |rFFT|^2,
 *   Slaney mel filterbank (fmin 0, fmax sr/2, norm 'slaney'), 10*log10(max(1e-10,S)),
 *   clamp to (per-chunk max - 80 dB).                                             */

/* Host-side tables (no GPU needed): dense filterbank (n_mels x 1025) as
 * librosa.filters.mel builds it; used by tests and by mt_mel_plan_init. */
int    mt_mel_filterbank_host(float* fb_host, int sr, int n_mels);
int    mt_mel_num_frames(int n_samples, int hop);           /* 1 + n_samples / hop */

/* Device-resident immutable tables for one (sr, hop, n_mels); `desc` (host memory, filled by
 * mt_mel_plan_init) carries what the launcher needs to know about them. */
typedef struct { int sr, hop, n_mels, ell_rows; } mt_mel_desc;
size_t mt_mel_plan_bytes(int n_mels);
int    mt_mel_plan_init(void* plan, size_t plan_bytes, int sr, int hop, int n_mels, mt_mel_desc* desc,
                        mt_stream_t stream);

/* wave[B][n_samples] f32 -> mel_db[B][n_mels][T] f32 (T = mt_mel_num_frames).
 * chunk_max_power[B] (f32 bit patterns, >= 0) receives each chunk's max mel POWER.
 * apply_clamp != 0: mel_db is final (clamped at max-80 dB), as power_to_db returns it.
 * apply_clamp == 0: mel_db is left unclamped; the consumer (mt_conv1_*) applies
 *                   max(x, 10*log10(max(1e-10, chunk_max_power[b])) - 80) on load.  */
int    mt_mel_db_f32(const void* plan, const mt_mel_desc* desc, const float* wave, int B, int n_samples,
                     float* mel_db, float* chunk_max_power, int apply_clamp, mt_stream_t stream);

/* Ragged batch of windows of a long device-resident store (csrc/rawbatch.hip), collated as collate_fn pads.
 * Window b = store[win_off[b] : win_off[b] + win_len[b]] (64-bit offsets, in floats); its samples at window
 * positions >= rec_end[b] read as 0 (a recording shorter than the window); frames are centre-padded at the
 * WINDOW's edges.  chunk_max_power[b] is the max over all 1 + win_len[b]/hop frames; mel_db[B][1][n_mels][T_out]
 * holds frames < t_keep[b] clamped at max-80 dB and 0.0 from t_keep[b] on.  Per window this equals
 * mt_mel_db_f32(apply_clamp=1) on a contiguous copy of it, trimmed and zero-padded, bit for bit.
 * max_win_len >= every win_len[b]; the store must hold one readable float past each window's readable end.
 * All tables are device pointers.                                                                           */
int    mt_mel_db_windows_f32(const void* plan, const mt_mel_desc* desc, const float* store, const long long* win_off,
                             const int* win_len, const int* rec_end, int B, int max_win_len, int T_out,
                             const int* t_keep, float* mel_db, float* chunk_max_power, mt_stream_t stream);

/* Piano-roll labels of the same windows: roll[B][88][T_out] f32 in {0,1}.  spans = int32 pairs (u, v): the sorted,
 * disjoint frame ranges [u, v) in which pitch 21 + p sounds in recording r (notes, sustain-pedal extension and
 * instrument widths already applied), pairs pitch_off[r*89 + p] .. pitch_off[r*89 + p + 1] - 1.
 * win_cols[b] >= 0 (chunk mode): column n < win_ncols[b] - 1 is any over frames [cols[c+n], cols[c+n+1]) (one frame
 * when equal), c = win_cols[b], and the last column is 0 (pretty_midi get_piano_roll(times=...)); win_cols[b] < 0
 * (full file): column n is frame n.  Columns >= t_keep[b] are 0.  cols may be NULL when no window is in chunk mode. */
int    mt_roll_windows(const int* spans, const long long* pitch_off, const int* cols, const int* win_rec,
                       const long long* win_cols, const int* win_ncols, const int* t_keep, int B, int T_out,
                       float* roll, mt_stream_t stream);

/* Training augmentation of the same windows (csrc/augment.hip): out[B][L_max] f32 (L_max a multiple of 4, >= every win_len[b]),
 * row b = win_len[b] samples of window b read at speed r_b = rate_q32[b] / 2^32, then zeros.  Output i interpolates the window at
 * pos = i * rate_q32[b] (64-bit): k = pos >> 32, frac = pos & 0xffffffff, ph = frac >> 24, mu = (frac & 0xffffff) * 2^-24,
 * c_j = tab[ph][j] + mu * (tab[ph + 1][j] - tab[ph][j]), y_i = sum_{j < 32} c_j * x[k - 15 + j]; x is the store relative to
 * win_off[b] and reads as 0 outside [-before[b], after[b]) (the window's recording; after[b] may be <= 0 or < win_len[b]).
 * tab[257][32] f32 is the caller's phase table (16-byte aligned; rows 0 and 256 unit impulses at taps 15 and 16, so that
 * rate_q32 = 2^32 copies the window bit for bit).  Every rate_q32[b] must lie in [rate_lo_q32, rate_hi_q32], itself within
 * 2^32 * (1 +- 0.03); the kernel clamps a rate outside the bounds it was given, so that no read leaves the staged span.
 * noise_rel (may be NULL: no noise) adds white noise after resampling: sigma_b = sqrt(mean y^2 over win_len[b]) *
 * noise_rel[b], out_i = y_i + sigma_b * g(seed, b, i) with g a standard normal from a counter-based hash (Box-Muller);
 * noise_rel[b] <= 0 or a silent window adds none.  The mean square is reduced in a fixed order: ws receives one f32 partial sum
 * of squares per (window, tile of 2048 outputs), ws[b * ceil(L_max / 2048) + t], and they are added in a fixed f64 tree.
 * ws / ws_bytes (mt_augment_ws_bytes) are needed only with noise_rel.  mt_mel_db_windows_f32 then takes `out` as its store
 * with win_off[b] = b * L_max and rec_end = win_len.  All tables are device pointers.                                  */
size_t mt_augment_ws_bytes(int B, int L_max);
int    mt_augment_windows(const float* store, const long long* win_off, const int* win_len, const int* before,
                          const int* after, const unsigned long long* rate_q32, unsigned long long rate_lo_q32,
                          unsigned long long rate_hi_q32, const float* noise_rel, unsigned seed, const float* tab, int B,
                          int L_max, float* out, void* ws, size_t ws_bytes, mt_stream_t stream);

/* Onset-regression targets of the same windows (csrc/onset_regress.hip, DESIGN.md 6c "Sub-frame onsets"): onset[B][88][T_out] f32 in
 * [0, 1], a triangle of half-width onset_width frames around every MIDI note-on.  on_tick = the note-ons of all recordings in ticks
 * of 100 us (int32), those of pitch 21 + p in recording r at tick_off[r*89 + p] .. tick_off[r*89 + p + 1] - 1, rising.  All integers, in
 * units of 12.5 us (a 16 kHz sample is 5, a tick 8, a frame of 512 samples 2560): frame t of window b is centred at source time
 *   tau = 5 start[b] + ((2560 t rate_q32[b] + 2^31) >> 32)      (start[b] = the window's first sample inside its recording; rate_q32
 * NULL = 2^32 for every window, else mt_augment_windows' speeds), W = 2560 onset_width, d = min over the pitch's note-ons of
 * |tau - 8 on_tick|, and onset = d < W ? (float)(W - d) / (float)W : 0 with one correctly rounded f32 division.  Columns >= t_keep[b] are
 * 0; a pitch without notes gives a zero row.  onset_width outside [2, 8] or T_out > 2^19: MT_EINVAL.  The units assume sr 16000 and hop
 * 512 (the caller's guard).  All tables are device pointers; one launch on `stream`, every cell of onset is written. */
int    mt_onset_regress_windows(const int* on_tick, const long long* tick_off, const int* win_rec, const int* start,
                                const unsigned long long* rate_q32, const int* t_keep, int B, int T_out, int onset_width,
                                float* onset, mt_stream_t stream);

/* Overlapping windows on one frame grid (csrc/stitch.hip, windows.py): src[Bw][P][Tw] holds the rows of Bw windows, which may
 * come from several recordings.  For each window b, local frames t in [keep_lo[b], keep_hi[b]) of every row p are copied to
 * dst[dst_row[b]][p][dst_frame0[b] + t] of dst[R][P][T_dst]; nothing else in dst is written (the caller pre-fills padding).
 * All tables are device pointers; their contents are the caller's contract (0 <= keep_lo <= keep_hi <= Tw, destination
 * frames < T_dst, rows < R).  64-bit indexing.                                                                          */
int    mt_stitch_windows(const float* src, int Bw, int P, int Tw, const int* dst_row, const long long* dst_frame0,
                         const int* keep_lo, const int* keep_hi, float* dst, int R, long long T_dst, mt_stream_t stream);

/* ------------------------------------------------------------------ CNN blocks
 * CNNRNNModel.cnn (cnn_rnn_model.py:29-39; Large: conv1, :178-183), eval mode; BatchNorm
 * running statistics are folded into (w, bias) by the host at load_state_dict time.
 * conv1: mel[B][n_mels][T] f32 (+ optional per-chunk dB floor from chunk_max_power, may be
 *        NULL) -> act1[B][n_mels/2][T][32] bf16, channels-last.
 *        w = folded Conv2d(1,32,3x3) weights [32][9] f32, bias [32] f32.
 * conv2: act1 -> X0[(t*B+b)*ldx + fo*64 + co] bf16 (the LSTM layer-0 GEMM A matrix; the
 *        reference's feature order c*F+f, cnn_rnn_model.py:60-62, is absorbed into W_ih's
 *        column order at pack time).  w2 = folded Conv2d(32,64,3x3) [64][tap=kh*3+kw][32] bf16. */
int    mt_conv1_bn_relu_pool(const float* mel, const float* chunk_max_power, const float* w, const float* bias,
                             void* act1, int B, int n_mels, int T, mt_stream_t stream);
int    mt_conv2_bn_relu_pool(const void* act1, const void* w2, const float* bias, void* X0, int ldx,
                             int B, int F1, int T, mt_stream_t stream);
/* The same with the 16-bit operand type chosen by the caller (dt = MT_DT_BF16 | MT_DT_F16). */
int    mt_conv1_bn_relu_pool_dt(const float* mel, const float* chunk_max_power, const float* w, const float* bias,
                                void* act1, int B, int n_mels, int T, int dt, mt_stream_t stream);
/* conv1 as the plain f32 fmaf chain on the vector ALU: the bit reference that mt_conv1_bn_relu_pool_dt (f32 matrix pipe) and
 * mt_conv12_bn_relu_pool_dt reproduce in every bit.  For tests; no product path calls it.                                   */
int    mt_conv1_valu_bn_relu_pool_dt(const float* mel, const float* chunk_max_power, const float* w, const float* bias,
                                     void* act1, int B, int n_mels, int T, int dt, mt_stream_t stream);
/* conv1 + conv2 in one kernel (models/cnn_rnn_model.py:29-39): X0 bit-identical to mt_conv1_bn_relu_pool_dt followed by
 * mt_conv2_bn_relu_pool_dt on the same operands; act1 is computed per tile in LDS and never exists in HBM.                */
int    mt_conv12_bn_relu_pool_dt(const float* mel, const float* chunk_max_power, const float* w1, const float* b1,
                                 const void* w2, const float* b2, void* X0, int ldx, int B, int n_mels, int T, int dt,
                                 mt_stream_t stream);
int    mt_conv2_bn_relu_pool_dt(const void* act1, const void* w2, const float* bias, void* X0, int ldx,
                                int B, int F1, int T, int dt, mt_stream_t stream);

/* ------------------------------------------------------------------ GEMM (bf16 MFMA, f32 accumulate)
 * C[M][N] (f32) = A[M][K] (bf16) * W[N][K]^T (bf16) + bias[N] (f32, may be NULL).
 * lda/ldw/ldc in elements.  The caller's A buffer must be readable up to row
 * roundup(M,128)-1 and W up to row roundup(N,128)-1 (pad rows may hold anything finite or
 * not: they only feed discarded outputs); K % 64 == 0.  Replaces the nn.Linear / nn.LSTM
 * input-projection matmuls (cnn_rnn_model.py:45-52,:55,:212-228,:250-256).               */
int    mt_gemm_bf16_f32acc(const void* A, int lda, const void* W, int ldw, const float* bias,
                           float* C, int ldc, int M, int N, int K, mt_stream_t stream);
/* LSTM input projection for BOTH directions of one layer: X[(t*B+b)][K] bf16, W_ih =
 * [fwd 4H rows; reverse 4H rows][K] bf16, bias[8H] = b_ih + b_hh, output in the layout
 * the recurrence streams: gx[b/32][t][dir][j/8][gate][j%8][b%32] f32 (mt_lstm_gx_bytes). */
int    mt_gemm_lstm_gx(const void* X, int ldx, const void* W_ih, int ldw, const float* bias, float* gx,
                       int B, int T, int H, int K, mt_stream_t stream);
/* Final projection with the reference's transpose fused: logits[b][n][t], rows m = t*B+b. */
int    mt_gemm_logits(const void* X, int ldx, const void* W, int ldw, const float* bias, float* logits,
                      int B, int T, int N, int K, mt_stream_t stream);
/* The layer-to-layer input projection and the final fc with A read STRAIGHT from the previous LSTM layer's hx images (f16
 * operands: the exchanged h is the operand type already), K = 2*Hprev, column k = dir*Hprev + unit, Hprev % 64 == 0: no
 * re-layout pass between the layers.  hx_prev as mt_lstm_bidir_fwd* wrote it for the same B, T.                      */
int    mt_gemm_lstm_gx_from_hx(const float* hx_prev, const void* W_ih, int ldw, const float* bias, float* gx,
                               int B, int T, int H, int Hprev, mt_stream_t stream);
/* The same; gx_f16 != 0 stores gx as f16 (see MT_GX_F16).                                                              */
int    mt_gemm_lstm_gx_from_hx_ex(const float* hx_prev, const void* W_ih, int ldw, const float* bias, float* gx,
                                  int B, int T, int H, int Hprev, int gx_f16, mt_stream_t stream);
int    mt_gemm_logits_from_hx(const float* hx_prev, const void* W, int ldw, const float* bias, float* logits,
                              int B, int T, int N, int Hprev, mt_stream_t stream);
/* The three GEMMs above with the operand type of A and W chosen by the caller (dt = MT_DT_BF16 | MT_DT_F16). */
int    mt_gemm_f32acc_dt(const void* A, int lda, const void* W, int ldw, const float* bias,
                         float* C, int ldc, int M, int N, int K, int dt, mt_stream_t stream);
int    mt_gemm_lstm_gx_dt(const void* X, int ldx, const void* W_ih, int ldw, const float* bias, float* gx,
                          int B, int T, int H, int K, int dt, mt_stream_t stream);
int    mt_gemm_logits_dt(const void* X, int ldx, const void* W, int ldw, const float* bias, float* logits,
                         int B, int T, int N, int K, int dt, mt_stream_t stream);
/* The two input projections with MT_GEMM_SCHED_BYTES of device scratch (`sched`, 16-byte aligned; zeroed by the call on
 * `stream`; nothing else may touch it until the launch has finished: one block per GEMM call of a forward in flight).  With it,
 * and for f16 gx (MT_GX_F16 / gx_f16) with B % 32 == 0, 256 | H and an even number >= 16 of 64-wide K-tiles, the projection runs
 * as PERSISTENT tiles: a workgroup walks a dynamic sequence of 256 x 256 tiles as one K-stream and the finished tile's f16
 * output leaves under the next tile's main loop (csrc/gemm.hip, gemm256p_kernel).  sched == NULL or any other shape: the
 * one-tile-per-workgroup kernels, bit-identical results.                                                                   */
#define MT_GEMM_SCHED_BYTES 64
size_t mt_gemm_sched_bytes(void);
int    mt_gemm_lstm_gx_sched(const void* X, int ldx, const void* W_ih, int ldw, const float* bias, float* gx,
                             int B, int T, int H, int K, int dt, void* sched, mt_stream_t stream);
int    mt_gemm_lstm_gx_from_hx_sched(const float* hx_prev, const void* W_ih, int ldw, const float* bias, float* gx,
                                     int B, int T, int H, int Hprev, int gx_f16, void* sched, mt_stream_t stream);

/* ------------------------------------------------------------------ bidirectional LSTM recurrence
 * nn.LSTM(batch_first, bidirectional) as the reference runs it (cnn_rnn_model.py:45-52,
 * :69-70): gate order i,f,g,o, zero initial state; fp32 state/gates/accumulation, W_hh h on the
 * f16 MFMA (W_hh and the exchanged h rounded to f16).  H % 16 == 0, H <= 1024.
 * w_hh = [fwd; reverse] x [4H][H] f32.  hx receives every step's h as f16 in the MFMA-operand
 * layout hx[b/32][t][dir][k/16][((k/8)%2)*32 + b%32][k%8] (mt_lstm_hx_bytes; typed float* here,
 * read it through mt_lstm_relayout_* / mt_lstm_unpack_f32).  sync_ws: mt_lstm_sync_bytes(); after the
 * stream has drained its word 0 is 0 (ok), 1 + step (flag spin timed out) or
 * 0x40000000 + step (payload spin timed out).                                              */
size_t mt_lstm_gx_bytes(int B, int T, int H);
size_t mt_lstm_hx_bytes(int B, int T, int H);
size_t mt_lstm_sync_bytes(int B, int H);
int    mt_lstm_bidir_fwd(const float* gx, const float* w_hh, float* hx, void* sync_ws, size_t sync_bytes,
                         int B, int T, int H, mt_stream_t stream);
/* A layer fed by the previous LSTM layer, with its input projection fused into the recurrence (no gx buffer, no GEMM, no
 * re-layout between the layers): gate pre-activations = W_ihx x_t + bias + W_hh h_{t-1}, x_t = the previous layer's h of
 * step t (both directions) read from ITS hx.  w_ihx [2][4H][2H] f32 (column = dir'*H + unit, zero columns for padded
 * units), bias [2][4H] = b_ih + b_hh.  H <= 512.                                                                       */
int    mt_lstm_bidir_fwd_xproj(const float* hx_prev, const float* w_ihx, const float* bias, const float* w_hh, float* hx,
                               void* sync_ws, size_t sync_bytes, int B, int T, int H, mt_stream_t stream);
/* As mt_lstm_bidir_fwd, with flags: 0, or MT_GX_F16 (gx holds f16 gate pre-activations).  (The XCD-local hand-off variants
 * that this entry point used to select -- "mode 1" with 8 and "mode 2" with 16 units per workgroup -- lost to the agent-scope
 * kernel with interleaved batch groups at every schedule and are gone, and mt_xcd_census with them.)                       */
int    mt_lstm_bidir_fwd_ex(const float* gx, const float* w_hh, float* hx, void* sync_ws, size_t sync_bytes,
                            int B, int T, int H, int flags, mt_stream_t stream);
/* Two workgroup sets when alone.  A plain inference launch with 2 .. 4 batch groups (H <= 512) carries twice the workgroups; when it
 * starts, the device looks at its count of persistent inference launches that are running: nobody else -> the two sets run half the
 * groups each ("wide"), otherwise the second set leaves at once ("narrow", the shape of a launch with one set).  Same bits either way.
 * A caller that runs several layers on one stream keeps its place in that count across them, so that the work between its layers
 * counts as running: MT_LSTM_KEEP on every layer but the last, MT_LSTM_HELD on every layer but the first (OR-ed into `flags`).
 * mt_lstm_set_width_mode: 0 = decide on the device (default), 1 = always narrow, 2 = always wide (admission still applies); for tests.
 * mt_lstm_width_offset: byte offset in the sync block of the decision word of the call's first launch, valid once the stream has
 * drained: 0 = a launch with one set only, 1 = narrow, 2 = wide.                                                                  */
#define MT_LSTM_HELD 0x100
#define MT_LSTM_KEEP 0x200
int    mt_lstm_set_width_mode(int mode);
size_t mt_lstm_width_offset(void);
/* 1 if launches that hold need[i] CUs each fit ncu CUs together with ONE launch's surplus (the largest of surplus[i]): at most one
 * launch is wide at a time.  The arithmetic of the admission check, without a device.                                            */
int    mt_persistent_fits(const double* need, const double* surplus, int n, int ncu);
/* CUs held by persistent launches still pending on streams other than `stream` on the current device (see above). */
int    mt_persistent_cus_in_flight(mt_stream_t stream);
/* hx -> X[(t*B+b)*ldx + dir*H + j] bf16 (next GEMM's A) / y[b][t][dir*H + j] f32 (torch layout). */
int    mt_lstm_relayout_bf16(const float* hx, void* X, int ldx, int B, int T, int H, mt_stream_t stream);
int    mt_lstm_unpack_f32(const float* hx, float* y, int B, int T, int H, mt_stream_t stream);

/* ------------------------------------------------------------------ whole-model forward
 * CNNRNNModel.forward in eval mode (cnn_rnn_model.py:57-74).  All pointers are device
 * pointers to tensors the host packed once from a reference state_dict
 * (music-transcription_amd/model.py: pack_cnnrnn).                                        */
#define MT_MAX_LSTM_LAYERS 8
typedef struct {
    int n_mels;                              /* input mel bins                                    */
    int hidden;                              /* LSTM hidden size (1..1024); laid out padded to 16 */
    int layers;                              /* LSTM layers (<= MT_MAX_LSTM_LAYERS)               */
    int operand_dtype;                       /* MT_DT_BF16 / MT_DT_F16: type of every 16-bit weight below and of the */
                                             /*   activations between the kernels (model.py packs f16 for inference) */
    const float* conv1_w;                    /* [32][9]  BN-folded                                */
    const float* conv1_b;                    /* [32]                                              */
    const void*  conv2_w;                    /* 16-bit [64][9][32] BN-folded                        */
    const float* conv2_b;                    /* [64]                                              */
    const void*  w_ih[MT_MAX_LSTM_LAYERS];   /* bf16 [roundup(8Hp,128)][K_l], Hp = roundup(H,16), */
                                             /*   gate row p*Hp + j (zero for j >= H); layer 0 columns in */
                                             /*   fo*64+co order, K_0 = (n_mels/4)*64;            */
                                             /*   K_l = roundup(2H,64), zero-padded, for l > 0    */
    const float* b_gates[MT_MAX_LSTM_LAYERS];/* f32 [8Hp] = b_ih + b_hh, [fwd; reverse]           */
    const float* w_hh[MT_MAX_LSTM_LAYERS];   /* f32 [2][4Hp][Hp]                                  */
    const void*  fc_w;                       /* bf16 [128][roundup(2H,64)], rows >= 88 zero       */
    const float* fc_b;                       /* f32 [88]                                          */
    const float* w_ihx[MT_MAX_LSTM_LAYERS];  /* layers l > 0 (optional, NULL = project with the GEMM): f32 [2][4Hp][2Hp], */
                                             /*   column dir'*Hp + k: the input projection fused into the recurrence      */
                                             /*   (mt_lstm_bidir_fwd_xproj; agent-scope hand-off, Hp <= 512)               */
} mt_cnnrnn_weights;

size_t mt_cnnrnn_workspace_bytes(const mt_cnnrnn_weights* w, int B, int T);
/* 1 when mt_cnnrnn_forward* runs conv1 + conv2 as one kernel (the default; MT_CONV_FUSED=0 in the environment selects the two
 * kernels; same X0 bit for bit, act1 never in HBM): the conv1 stage of mt_cnnrnn_forward_ex's event list is then empty.    */
int    mt_cnnrnn_conv_fused(void);
size_t mt_cnnrnn_status_offset(const mt_cnnrnn_weights* w, int B, int T, int layer);
/* mel[B][n_mels][T] f32 (dB; chunk_max_power may be NULL when mel is already clamped)
 * -> logits[B][88][T] f32.                                                                */
int    mt_cnnrnn_forward(const mt_cnnrnn_weights* w, const float* mel, const float* chunk_max_power,
                         int B, int T, float* logits, void* workspace, size_t workspace_bytes,
                         mt_stream_t stream);
/* Same, recording the caller's hipEvent_t handles (events[0] before the first kernel, then
 * one after each stage: conv1, conv2, (input-projection GEMM, recurrence, re-layout) x layers,
 * fc) so that a benchmark can time each kernel on the launch stream.  events may be NULL.   */
int    mt_cnnrnn_num_stages(int layers);
int    mt_cnnrnn_forward_ex(const mt_cnnrnn_weights* w, const float* mel, const float* chunk_max_power,
                            int B, int T, float* logits, void* workspace, size_t workspace_bytes,
                            void* const* events, int n_events, mt_stream_t stream);

/* ------------------------------------------------------------------ CNNRNNModelLarge pieces
 * Channels-last bf16 convolution with folded BatchNorm (ResidualBlock, freq_aware_conv;
 * cnn_rnn_model.py:76-99,:186-202):  out = act(conv_{KHx3,pad(KH/2,1)}(A) [+ conv_1x1(S)] + bias),
 * optional MaxPool2d((2,1)).  A [B][F][T][C1], S [B][F][T][C2] (residual skip input, may be NULL),
 * W [Cout][KH*3*C1 + C2] bf16 (K order: tap = kh*3+kw, ci; then the skip channels).
 * out_mode 0: [B][Fout][T][Cout] bf16;  1: GEMM-A rows X[(t*B+b)*ldx + fo*Cout + co].        */
int    mt_conv_cl_bf16(const void* A, const void* S, const void* W, const float* bias, void* out,
                       int B, int F, int T, int C1, int C2, int Cout, int KH, int relu, int pool,
                       int out_mode, int ldx, mt_stream_t stream);
/* Batched GEMMs: batch z -> (z1, z2) = (z / zdiv, z % zdiv), element offsets z1*s?1 + z2*s?2.  */
int    mt_gemm_batched_f32(const void* A, int lda, long long sA1, long long sA2, const void* W, int ldw,
                           long long sW1, long long sW2, const float* bias, float* C, int ldc,
                           long long sC1, long long sC2, int M, int N, int K, int batch, int zdiv,
                           mt_stream_t stream);
int    mt_gemm_batched_bf16out(const void* A, int lda, long long sA1, long long sA2, const void* W, int ldw,
                               long long sW1, long long sW2, const float* bias, void* C, int ldc,
                               long long sC1, long long sC2, int M, int N, int K, int batch, int zdiv,
                               int relu, mt_stream_t stream);
/* hx -> feature rows with a column offset, dropping padded hidden units (k >= Hv); X (bf16) and/or Y (f32). */
int    mt_lstm_relayout_ex(const float* hx, void* X, int ldx, float* Y, int ldy, int col_off,
                           int B, int T, int H, int Hv, mt_stream_t stream);
/* `_dt` forms of the Large model's pieces: operand type (and type of a 16-bit output) dt = MT_DT_BF16 | MT_DT_F16. */
int    mt_conv_cl_dt(const void* A, const void* S, const void* W, const float* bias, void* out,
                     int B, int F, int T, int C1, int C2, int Cout, int KH, int relu, int pool,
                     int out_mode, int ldx, int dt, mt_stream_t stream);
int    mt_gemm_batched_f32_dt(const void* A, int lda, long long sA1, long long sA2, const void* W, int ldw,
                              long long sW1, long long sW2, const float* bias, float* C, int ldc,
                              long long sC1, long long sC2, int M, int N, int K, int batch, int zdiv, int dt,
                              mt_stream_t stream);
int    mt_gemm_batched_h16out_dt(const void* A, int lda, long long sA1, long long sA2, const void* W, int ldw,
                                 long long sW1, long long sW2, const float* bias, void* C, int ldc,
                                 long long sC1, long long sC2, int M, int N, int K, int batch, int zdiv,
                                 int relu, int dt, mt_stream_t stream);
int    mt_lstm_relayout_dt(const float* hx, void* X, int ldx, float* Y, int ldy, int col_off,
                           int B, int T, int H, int Hv, int dt, mt_stream_t stream);
/* MultiHeadAttention pieces (cnn_rnn_model.py:118-139): P = softmax(clamp(S*scale, +-clip)) -> bf16 with
 * the key axis zero-padded to Tp; V^T per (chunk, head); y = LayerNorm(resid + proj) -> bf16.       */
int    mt_attn_softmax_clamped(const float* S, int lds, void* P, int Tp, int T, long long rows,
                               float scale, float clip, mt_stream_t stream);
int    mt_attn_transpose_v(const void* qkv, int ld3, int voff, void* VT, int B, int T, int Tp,
                           int heads, int dp, mt_stream_t stream);
/* Fused attention core (eval mode): ao[(t*B+b)*ldo + head*dp + d] = sum_j softmax_j(clamp(Q K^T * scale, +-clip))[t][j] V[j][d] per
 * (chunk, head), scores never written (cnn_rnn_model.py:118-139: scale, clamp BEFORE softmax -- so exp() needs no running
 * maximum).  qkv [(t*B+b)][ld3]: Q at column head*dp, K at Ca + head*dp (16-bit, dt); VT as mt_attn_transpose_v writes it for
 * Tp = roundup(T, 64).  dp in {64, 128, 192} (else MT_EUNSUPPORTED), clip <= 10.  csrc/attn_fused.hip.                       */
int    mt_attn_fused_clamped(const void* qkv, int ld3, int Ca, const void* VT, int Tp, int B, int T, int heads, int dp,
                             float scale, float clip, void* ao, int ldo, int dt, mt_stream_t stream);
int    mt_layernorm_residual(const float* resid, int ldr, const float* proj, int ldp, const float* gamma,
                             const float* beta, void* y, int ldy, long long rows, int n, float eps,
                             mt_stream_t stream);
int    mt_attn_softmax_clamped_dt(const float* S, int lds, void* P, int Tp, int T, long long rows,
                                  float scale, float clip, int dt, mt_stream_t stream);
int    mt_layernorm_residual_dt(const float* resid, int ldr, const float* proj, int ldp, const float* gamma,
                                const float* beta, void* y, int ldy, long long rows, int n, float eps, int dt,
                                mt_stream_t stream);

/* CNNRNNModelLarge.forward, eval mode (cnn_rnn_model.py:262-348).  Packed by model.py: pack_large. */
typedef struct {
    int n_mels, hidden, layers, hidden_local;     /* real sizes (hidden_local = hidden / 2)            */
    int use_attention, use_heads, heads, head_dim_pad;  /* head_dim padded to a multiple of 64         */
    float attn_scale;                             /* (real head_dim)^-1/2                              */
    int operand_dtype;                            /* MT_DT_BF16 / MT_DT_F16 (as mt_cnnrnn_weights)     */
    const float* conv1_w; const float* conv1_b;   /* [32][9], [32]                                     */
    const void*  rb1c1_w; const float* rb1c1_b;   /* bf16 [64][9*32]                                   */
    const void*  rb1c2_w; const float* rb1c2_b;   /* bf16 [64][9*64 + 32]  (conv2 + 1x1 skip)          */
    const void*  rb2c1_w; const float* rb2c1_b;   /* bf16 [128][9*64]                                  */
    const void*  rb2c2_w; const float* rb2c2_b;   /* bf16 [128][9*128 + 64]                            */
    const void*  fa_w;    const float* fa_b;      /* bf16 [256][21*128]                                */
    const void*  main_w_ih[MT_MAX_LSTM_LAYERS]; const float* main_b[MT_MAX_LSTM_LAYERS]; const float* main_w_hh[MT_MAX_LSTM_LAYERS];
    const void*  local_w_ih; const float* local_b; const float* local_w_hh;
    const void*  qkv_w;  const float* qkv_b;      /* bf16 [roundup(3*heads*dp,128)][Cp], Cp = roundup(comb,64) */
    const void*  proj_w; const float* proj_b;     /* bf16 [roundup(comb,128)][heads*dp]                */
    const float* ln_g;   const float* ln_b;       /* [comb]                                            */
    const void*  shared_w; const float* shared_b; /* bf16 [roundup(hidden,128)][Cp]                    */
    const void*  heads_w;  const float* heads_b;  /* bf16 [384][roundup(hidden,64)]: frame, onset, offset */
    const void*  fc_w;     const float* fc_b;     /* no-heads variant: bf16 [128][Cp]                  */
    const float* main_w_ihx[MT_MAX_LSTM_LAYERS];  /* main layers l > 0, optional: f32 [2][4Hp][2Hp] for the input projection */
                                                  /*   fused into the recurrence (as mt_cnnrnn_weights.w_ihx)                 */
} mt_cnnrnn_large_weights;
size_t mt_cnnrnn_large_workspace_bytes(const mt_cnnrnn_large_weights* w, int B, int T);
size_t mt_cnnrnn_large_status_offset(const mt_cnnrnn_large_weights* w, int B, int T, int idx);
/* logits3: [3][B][88][T] (frame, onset, offset) when use_heads, else [B][88][T]. */
int    mt_cnnrnn_large_forward(const mt_cnnrnn_large_weights* w, const float* mel, const float* chunk_max_power,
                               int B, int T, float* logits3, void* workspace, size_t workspace_bytes,
                               mt_stream_t stream);
/* As above; with side_stream + two caller-owned hipEvent_t (all three non-NULL) the local LSTM branch runs on side_stream
 * beside the main LSTM stack (fork after the CNN, join before the attention).                                        */
int    mt_cnnrnn_large_forward_ex(const mt_cnnrnn_large_weights* w, const float* mel, const float* chunk_max_power,
                                  int B, int T, float* logits3, void* workspace, size_t workspace_bytes,
                                  mt_stream_t stream, mt_stream_t side_stream, void* ev_fork, void* ev_join);

/* Everything on `stream`, recording the caller's hipEvent_t handles at the stage boundaries (events[0] before the first kernel,
 * then one after each of the mt_cnnrnn_large_num_stages(layers) stages: conv1, res_block1, res_block2, freq_aware_conv, local
 * LSTM (projection, recurrence, re-layout), main LSTM layers (projection, recurrence, re-layout) x layers, attention +
 * LayerNorm, heads) so that a benchmark can time each kernel group on the launch stream.                               */
int    mt_cnnrnn_large_num_stages(int layers);
int    mt_cnnrnn_large_forward_ev(const mt_cnnrnn_large_weights* w, const float* mel, const float* chunk_max_power,
                                  int B, int T, float* logits3, void* workspace, size_t workspace_bytes,
                                  void* const* events, int n_events, mt_stream_t stream);

/* ------------------------------------------------------------------ loss, prediction, F1
 * Masked BCE-with-logits (transcription_model.py:110-162,:196-217):
 *   loss[0] (=, or += when accumulate) weight * sum_{valid} bce(logit, target) / max(n_valid_frames*P, 1)
 *   grad (may be NULL) = d loss / d logits = weight * (sigmoid(x) - y) * mask / denom.
 * lengths (int64, device, may be NULL = all frames valid); n_valid_frames = sum_b min(lengths[b], T)
 * (or B*T), known to the host.  workspace: mt_bce_workspace_bytes().  Bitwise reproducible.  */
size_t mt_bce_workspace_bytes(void);
int    mt_bce_masked_fwd_bwd(const float* logits, const float* targets, const long long* lengths,
                             long long n_valid_frames, float weight, int accumulate, float* loss, float* grad,
                             void* workspace, size_t workspace_bytes, int B, int P, int T, mt_stream_t stream);
/* onset/offset targets from a roll (transcription_model.py:176-185): rows x T, diff along T. */
int    mt_onset_offset_targets(const float* roll, float* onset, float* offset, long long rows, int T,
                               mt_stream_t stream);
/* Class-weighted / focal BCE for the frame, onset and offset heads in one pass (csrc/heads_loss.hip, DESIGN.md 6b "Weighted and focal
 * loss").  Per valid cell of head h, logit x, target y in [0, 1], w = pos_weight[h], g = gamma[h]:
 *   a = softplus(x), b = softplus(-x), l = w y exp(-g a) b + (1 - y) exp(-g b) a         (w = 1, g = 0: the BCE above)
 *   loss_h = head_weight[h] sum_valid l / max(n_valid_frames*P, 1);  grad_h = head_weight[h] (dl/dx) / denom, exactly 0 in masked frames.
 * loss (device, 4 floats) = {total, frame, onset, offset}, each part times its head weight, total = (frame + onset) + offset.
 * Logits, roll, onset_roll and gradients are [B][P][T].  onset_logits and offset_logits both NULL: one head (loss[2] = loss[3] = 0, the
 * onset / offset gradients are not written).  The offset target and, with onset_roll == NULL, the onset target are those of
 * mt_onset_offset_targets bit for bit, formed from the roll inside the kernel (within a row, whatever lengths says); with onset_roll the
 * onset head is trained against it.  NaN / Inf in a masked frame of any input reaches neither the loss nor a gradient; a non-finite roll
 * value in the first masked frame counts as 0 in the last valid frame's offset target.  lengths, n_valid_frames: as
 * mt_bce_masked_fwd_bwd.  head_weight, pos_weight, gamma: HOST arrays of 3 (frame, onset, offset), taken by value at the call; all three
 * entries are checked also for one head.  Any gradient pointer may be NULL.  workspace: mt_heads_loss_workspace_bytes().
 * MT_EINVAL, nothing written: a null frame_logits / roll / loss / workspace / host array, exactly one of onset_logits and offset_logits,
 * onset_roll without onset_logits, a non-positive dim, pos_weight <= 0, head_weight < 0, gamma outside [0, 8], or a non-finite value.
 * MT_EWORKSPACE: workspace too small.  Two launches on `stream`, no atomics, no synchronisation, allocation or copy; bitwise reproducible. */
size_t mt_heads_loss_workspace_bytes(void);
int    mt_heads_loss_fwd_bwd(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* roll,
                             const float* onset_roll, const long long* lengths, long long n_valid_frames, const float* head_weight,
                             const float* pos_weight, const float* gamma, float* loss, float* frame_grad, float* onset_grad,
                             float* offset_grad, void* workspace, size_t workspace_bytes, int B, int P, int T, mt_stream_t stream);
/* roll = (sigmoid(logits) > threshold) as float {0,1} (transcription_model.py:262-265, main.py:153-156). */
int    mt_predict_threshold(const float* logits, float* roll, long long n, float threshold, mt_stream_t stream);
/* counts[b] = {TP, FP, FN} (uint64) over the first lengths[b] frames (evaluate.py:361-373). */
int    mt_f1_counts(const float* pred, const float* target, const long long* lengths,
                    unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
/* counts[b][k] = {TP, FP, FN} of (sigmoid(logits) > thresholds[k]) for 1 <= K <= 16 thresholds (else MT_EINVAL) in one pass:
 * the data side of evaluate.py's threshold tuning (:524-618) without re-running the model.          */
int    mt_f1_sweep_counts(const float* logits, const float* target, const long long* lengths,
                          const float* thresholds, int K, unsigned long long* counts, int B, int P, int T,
                          mt_stream_t stream);

/* Roll -> notes on the device: combine_piano_rolls + the run-length part of pianoroll_to_midi (main.py:164-226,
 * scripts/evaluate.py:54-88).  The NB chunks of src [NB][P][T] are one roll of NB*T frames per pitch; src_mode 0: logits
 * (active = sigmoid(x) > threshold, as mt_predict_threshold), 1: roll values (active = x > 0).  counts[p] = notes of pitch p;
 * note k of pitch p is frames [starts[i], ends[i]) at i = sum_{q<p} counts[q] + k -- the reference's note order.  Nothing is
 * written for a pitch whose notes would not fit `capacity`: the host compares sum(counts) with it.  Only the notes leave the GPU. */
int    mt_roll_to_notes(const float* src, int src_mode, float threshold, int NB, int P, int T, int* counts, int* starts, int* ends,
                        int capacity, mt_stream_t stream);

/* Note-level evaluation (csrc/notes.hip, DESIGN.md "Note-level F1"): counts[b] = {n_ref, n_est, tp_onset, tp_onset_offset} (uint64)
 * of mir_eval's precision_recall_f1_overlap on the 32 ms frame grid.  Estimated notes: with onset_logits == NULL the runs of
 * (sigmoid(frame) > thr_frame) (the mt_roll_to_notes decoder); otherwise the onset-gated decoder -- a note opens at each rising edge
 * of (sigmoid(onset) > thr_onset) and lasts while frame OR onset is active.  Reference notes: the runs of (ref_roll > 0).  Frames
 * at or past lengths[b] (int64, device, NULL = all T) are inactive on both sides.  A match needs |d onset| <= 1 frame, and for
 * tp_onset_offset also |d offset| <= 1 or 5 |d offset| <= reference length; each tp is a maximum matching.  frame_logits,
 * onset_logits and ref_roll are [B][P][T] rows (onset_logits may be out[1] of the Large forward).  0 < thresholds < 1.  */
int    mt_note_match_counts(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset,
                            const float* ref_roll, const long long* lengths, unsigned long long* counts, int B, int P, int T,
                            mt_stream_t stream);
/* mt_note_match_counts against a note list instead of a roll: same decoders, activity expression, lengths and counts, but the
 * reference notes of row (b, p) are ref_on / ref_off[ref_ptr[b*P + p] .. ref_ptr[b*P + p + 1]) (int32, device; ref_ptr has B*P + 1
 * entries), in ticks of 100 us, sorted by onset, 0 <= on < off; they may be arbitrarily close (re-struck keys).  One frame is 320
 * ticks: estimated note [s, e) in frames has times 320 s, 320 e.  A match needs |d onset| <= 500 ticks, and for tp_onset_offset also
 * 5 |d offset| <= max(2500, reference length); each tp is a maximum matching.  With L = min(T, lengths[b]) frames
 * valid, reference notes with on >= 320 L are not counted and offsets are clipped to 320 L.  Needs 320 T < 2^31.  Exact integers. */
int    mt_note_match_list(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset,
                          const int* ref_on, const int* ref_off, const long long* ref_ptr, const long long* lengths,
                          unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
/* mt_note_match_counts / mt_note_match_list for a grid of thresholds in one pass: counts[b][i][j] (uint64 [B][Kf][Ko][4], zeroed on the
 * stream) is bit for bit what the single-pair entry point returns for (thr_frame[i], thr_onset[j]) on the same inputs.  thr_frame[Kf]
 * and thr_onset[Ko] are HOST arrays, taken by value at the call (no device copy, no synchronisation); any order, repeats allowed,
 * every value in (0, 1).  1 <= Kf, Ko <= 16 and Kf * Ko <= 64.  With onset_logits == NULL (the frame decoder) Ko must be 1 and
 * thr_onset may be NULL.  Every logit is read, and its sigmoid evaluated, once per launch.  Dimension limits as the single-pair calls. */
int    mt_note_sweep_counts(const float* frame_logits, const float* onset_logits, const float* thr_frame, int Kf, const float* thr_onset,
                            int Ko, const float* ref_roll, const long long* lengths, unsigned long long* counts, int B, int P, int T,
                            mt_stream_t stream);
int    mt_note_sweep_list(const float* frame_logits, const float* onset_logits, const float* thr_frame, int Kf, const float* thr_onset,
                          int Ko, const int* ref_on, const int* ref_off, const long long* ref_ptr, const long long* lengths,
                          unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
/* The onset-gated decoder with mt_roll_to_notes' contract: the NB chunks of frame_logits / onset_logits [NB][P][T] are one
 * recording of NB*T frames per pitch; counts[p], starts / ends in the reference's note order, capacity protocol unchanged. */
int    mt_heads_to_notes(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, int NB, int P, int T,
                         int* counts, int* starts, int* ends, int capacity, mt_stream_t stream);
/* The offset-gated decoder behind the three entry points above: the onset-gated rule, and in addition a rising edge of
 * (sigmoid(offset) > thr_offset) at frame t >= the note's start makes t the note's last frame (end t + 1).  Only edges cut -- an offset
 * already active before the start does not -- and only onset edges open notes, so starts and the number of notes are the onset-gated
 * decoder's and every end is <= its end; with the offset head nowhere active the notes are identical.  offset_logits has the layout of
 * onset_logits (it may be out[2] of the Large forward); frames at or past lengths[b] are inactive for all three heads.  Each call has
 * the contract of its namesake -- reference notes, matching, counts, chunk concatenation, note order, capacity protocol -- except that
 * onset_logits and offset_logits must be non-NULL and all three thresholds in (0, 1): otherwise MT_EINVAL and nothing is written. */
int    mt_note_match_counts_off(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                float thr_onset, float thr_offset, const float* ref_roll, const long long* lengths,
                                unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
int    mt_note_match_list_off(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                              float thr_onset, float thr_offset, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                              const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
int    mt_heads_to_notes_off(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                             float thr_onset, float thr_offset, int NB, int P, int T, int* counts, int* starts, int* ends, int capacity,
                             mt_stream_t stream);
/* The notes of a padded batch of whole recordings (csrc/notes_batch.hip): row (b, p) is frame_logits[(b*P + p)*T + t]
 * (onset_logits alike, NULL = the frame decoder) and its valid frames are [0, L_b), L_b = clamp(lengths[b], 0, T) (int64, device,
 * NULL = all T).  Frames at or past L_b are inactive and never read -- the padding may hold anything, NaN included -- and a note still
 * open at L_b ends at L_b.  The notes of a row are exactly those of mt_roll_to_notes (src_mode 0) / mt_heads_to_notes on a contiguous
 * [1][1][L_b] copy of it.  counts[b*P + p] (int32) and row_off[0 .. B*P] (int64, the exclusive prefix of counts in row order,
 * row_off[B*P] = all notes) are always written; note k of row (b, p) is frames [starts[i], ends[i]) at i = row_off[b*P + p] + k: per
 * recording the reference's note order.  A row is written only when row_off + count <= capacity and nothing at or past `capacity` is
 * touched: the host compares row_off[B*P] with it (capacity 0: counts only, starts / ends may be NULL).  Up to three launches on
 * `stream`; no synchronisation, allocation or copy.  0 < thresholds < 1; B*P and T below 2^31; all indexing is 64-bit. */
int    mt_notes_batch(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const long long* lengths,
                      int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends, long long capacity,
                      mt_stream_t stream);
/* Note cleanup in the decoders (csrc/note_decode.h clean_step, DESIGN.md 6c "Note cleanup"), two parameters in frames of 32 ms.  Per pitch row of L
 * valid frames: inactive runs of a = f | o of at most bridge_frames (0..63) frames that have an active frame of the row directly
 * before and after them are filled (the frame decoder fills f and takes its onsets from the result; the onset mask of the other two
 * is untouched, so a re-struck key still splits, and an offset edge still cuts through a bridged gap); the decoder runs on that; then
 * every note [s, e) with e - s < min_frames (1..64) is removed, however it closed, its neighbours untouched.  (1, 0) changes nothing,
 * and is served by the cleaning kernels all the same.  Each call has the contract of its _off namesake (mt_notes_batch_clean: of
 * mt_notes_batch) with these exceptions: offset_logits may be NULL (the onset-gated decoder; thr_offset is not read), in
 * mt_heads_to_notes_clean onset_logits may then be NULL too (the frame decoder: mt_roll_to_notes' notes, src_mode 0); offset_logits
 * without onset_logits, or min_frames / bridge_frames out of range: MT_EINVAL and nothing is written. */
int    mt_note_match_counts_clean(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                  float thr_onset, float thr_offset, const float* ref_roll, const long long* lengths,
                                  unsigned long long* counts, int B, int P, int T, int min_frames, int bridge_frames, mt_stream_t stream);
int    mt_note_match_list_clean(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                float thr_onset, float thr_offset, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                const long long* lengths, unsigned long long* counts, int B, int P, int T, int min_frames, int bridge_frames,
                                mt_stream_t stream);
int    mt_heads_to_notes_clean(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                               float thr_onset, float thr_offset, int NB, int P, int T, int* counts, int* starts, int* ends, int capacity,
                               int min_frames, int bridge_frames, mt_stream_t stream);
int    mt_notes_batch_clean(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const long long* lengths,
                            int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends, long long capacity,
                            int min_frames, int bridge_frames, mt_stream_t stream);
/* Peak-picked onsets in the decoders (csrc/note_decode.h peak_mask, DESIGN.md 6c "Peak-picked onsets"), for an onset head trained
 * against the triangular target of mt_onset_regress_targets.  Each call is its _clean namesake -- the same arguments, contract and
 * cleanup, (min_frames, bridge_frames) = (1, 0) for none -- with another rule for where a note opens.  Per pitch row with valid frames
 * [0, L) and onset logits x (with chunks, mt_heads_to_notes_peak: the chunks concatenated in time, neighbours across chunk
 * boundaries), frame t is an onset iff 1 / (1 + exp(-x[t])) > thr_onset (the expression of the other decoders), x[t] > x[u] for every u
 * of [0, L) in [t - peak_reach, t - 1], and x[t] >= x[u] for every u of [0, L) in [t + 1, t + peak_reach]: a local maximum of the
 * logits, not of their sigmoids, which saturate into ties.  A plateau gives its first frame, and the onsets of a row are more than
 * peak_reach frames apart.  Frames outside [0, L) take no part and are never loaded.  The rest is the decoder of the namesake: the
 * activity is a = f | (sigmoid(x) > thr_onset), a note opens at every onset frame and stays open while a holds, until a drops or the
 * next onset frame; the offset-gated decoder uses the onset frames where it used the onset mask's rising edges; bridging fills a and
 * leaves the onset frames alone; short notes are dropped last.  onset_logits == NULL (the frame decoder has no onset head) or
 * peak_reach outside 1..8: MT_EINVAL, nothing is launched or written.  offset_logits may be NULL (the onset-gated decoder).  What the
 * rule does to note F1 on MAESTRO has not been measured. */
int    mt_note_match_counts_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                 float thr_onset, float thr_offset, const float* ref_roll, const long long* lengths,
                                 unsigned long long* counts, int B, int P, int T, int min_frames, int bridge_frames, int peak_reach,
                                 mt_stream_t stream);
int    mt_note_match_list_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                               float thr_onset, float thr_offset, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                               const long long* lengths, unsigned long long* counts, int B, int P, int T, int min_frames, int bridge_frames,
                               int peak_reach, mt_stream_t stream);
int    mt_heads_to_notes_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                              float thr_onset, float thr_offset, int NB, int P, int T, int* counts, int* starts, int* ends, int capacity,
                              int min_frames, int bridge_frames, int peak_reach, mt_stream_t stream);
int    mt_notes_batch_peak(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const long long* lengths,
                           int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends, long long capacity,
                           int min_frames, int bridge_frames, int peak_reach, mt_stream_t stream);
/* Sub-frame onsets of decoded notes (csrc/onset_regress.hip, DESIGN.md 6c "Sub-frame onsets"): on_tick[i] (int32, ticks of 100 us) for
 * the n notes [starts[i], ends[i]) of any onset-gated decoder above, cleaned or not.  row_off (int64, rows + 1 entries, rising from 0
 * to n) gives the notes of row r as row_off[r] .. row_off[r + 1] - 1; the kernel finds a note's row by binary search.  chunks == 0:
 * onset_logits[NB][P][T] is a padded batch, rows = NB * P, row b*P + p has L = clamp(lengths[b], 0, T) valid frames (lengths int64,
 * device, NULL = all T).  chunks != 0: the NB chunks are one recording of L = NB * T frames per pitch, rows = P, frame g at chunk g / T,
 * t = g % T, and lengths must be NULL.  Per note, with q[g] = 1 / (1 + exp(-x[g])) in f32 inside [0, L) and 0 outside (nothing outside
 * is loaded: the padding may hold NaN): the peak k starts at s and steps to k + 1 while k + 1 <= min(s + reach, e - 1, L - 1) and
 * q[k + 1] > q[k]; with A = q[k - 1], B = q[k], C = q[k + 1], m = min(A, C): shift = 0 if B - m < 2^-10, else (C - A) / (2 (B - A)) if
 * C > A, else (C - A) / (2 (B - C)), clamped to [-0.5, 0.5]; on_tick = clamp(320 k + (int)rintf(320 shift), 0, 320 e - 1).  As k >= s and
 * the notes of a row do not overlap, the ticks of a row stay sorted.  reach in [0, 8]; n notes are refined (n = 0 launches nothing and
 * needs no pointers); 320 L must stay below 2^31.  One launch on `stream`, one thread per note. */
int    mt_refine_onsets(const int* starts, const int* ends, const long long* row_off, long long rows, long long n,
                        const float* onset_logits, int NB, int P, long long T, const long long* lengths, int chunks, int reach,
                        int* on_tick, mt_stream_t stream);
/* Note matching in ticks for estimates off the frame grid (csrc/note_ticks.hip, DESIGN.md 6c "Sub-frame onsets", Scoring): the counts of
 * mt_note_match_list for an estimated note LIST, such as the notes of mt_notes_batch with the onsets of mt_refine_onsets (off = 320 e).
 * Both sides are note lists in the layout of mt_note_match_list's reference: on / off int32 ticks of 100 us on the device, ptr int64
 * with B*P + 1 entries rising from 0, row (b, p) owning [ptr[b*P + p], ptr[b*P + p + 1]); within a row on is non-decreasing (equal
 * onsets are allowed) and 0 <= on < off.  counts[b] = {n_ref, n_est, tp_onset, tp_onset_offset} (uint64), zeroed on the stream and then
 * fully written: nothing depends on what counts or workspace held.  A match needs |d on| <= 500 ticks, and for tp_onset_offset also
 * 5 |d off| <= max(2500, ref_off - ref_on), in 64 bits; each tp is the size of a MAXIMUM matching of its row's graph, summed over the
 * recording's P rows.  No row length, component size or search depth changes the result.  lengths (int64, device, B entries in frames,
 * NULL = no clipping): with L = max(0, lengths[b]), reference notes with on >= 320 L are not counted and reference offsets are clipped
 * to 320 L (mt_note_match_list's rule); estimates are taken as given.  An empty list is legal and its on / off may be NULL.
 * workspace: mt_note_match_ticks_workspace(n_est, n_ref) bytes on the device for lists of n_est = est_ptr[B*P] and n_ref =
 * ref_ptr[B*P] notes (at least 16; int32 words match[n_est] | stamp[n_est] | lo[n_ref] | hi[n_ref] | stack[2][n_ref], every word written
 * before it is read).  A null ptr table, counts or workspace, on without off, B <= 0, P <= 0 or workspace_bytes below
 * mt_note_match_ticks_workspace(0, 0): MT_EINVAL, nothing launched.  The two note totals are on the device, and the call neither copies
 * nor synchronises, so the kernel itself compares workspace_bytes with what its tables need; a row whose tables need more, whose slices
 * leave the tables or whose onsets are out of order reads no note and writes no workspace word, and bit 63 of the four counts[b] is set
 * instead.  One memset and one launch on `stream`, one wave64 per pitch row: the reference notes' estimate slices by binary search, then
 * one lane per connected component of the row (a greedy pass for tp_onset, whose graph is convex; augmenting paths for tp_onset_offset). */
size_t mt_note_match_ticks_workspace(long long n_est, long long n_ref);
int    mt_note_match_ticks(const int* est_on, const int* est_off, const long long* est_ptr, const int* ref_on, const int* ref_off,
                           const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P,
                           void* workspace, size_t workspace_bytes, mt_stream_t stream);
/* Frame smoothing (csrc/smooth.hip, DESIGN.md 6c "Frame smoothing"): per pitch row, the Viterbi path of a two-state (off / on) HMM over
 * the frame head, written as logits.  Evidence q_t = rint(clamp(x_t - logit(thr), -64, 64) * 64), forced to q_t >= 1 where the frame is
 * active as mt_predict_threshold has it and to q_t <= 0 where it is not; a = rint(64 * on_penalty), b = rint(64 * off_penalty); the
 * path s maximises sum s_t q_t - a #(0->1) - b #(1->0) over the row's valid frames (a tie from on goes to off, from off stays off).
 * out[t] = s_t ? +64.0f : -64.0f, so every consumer of frame logits reads the path at any threshold in [1e-6, 1 - 1e-6].  With both
 * penalties 0 the path is the thresholded activity, bit for bit.
 *   mt_frame_smooth:        a padded batch [B][P][T], valid frames [0, L_b), L_b = clamp(lengths[b], 0, T) (int64, device, NULL = all
 *                           T), 64-bit row addressing as mt_notes_batch.  Frames at or past L_b are neither read nor written.
 *   mt_frame_smooth_chunks: the NB chunks [NB][P][T] as one row of NB * T frames per pitch, as mt_heads_to_notes walks them.
 * out may be frame_logits itself (in place: a frame is read before anything is stored at its place); any other overlap of the two
 * buffers, a threshold outside (0, 1), a penalty outside [0, 64] (NaN included), a null pointer or bad dims: MT_EINVAL, no launch.
 * One launch on `stream`; no workspace, synchronisation, allocation or copy. */
int    mt_frame_smooth(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, const long long* lengths,
                       int B, int P, long long T, mt_stream_t stream);
int    mt_frame_smooth_chunks(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, int NB, int P, int T,
                              mt_stream_t stream);
/* Long rows (DESIGN.md 6c "Long rows: segments per wave"): the same output, bit for bit, from one workgroup of `waves` wave64s per row,
 * each walking a contiguous stretch of the row's 64-frame windows.  Arguments, limits and refusals are those of the twin without
 * _split; on top of them waves outside [2, 16], or rows * waves at or past 2^26 (rows = B * P, or P for chunks): MT_EINVAL, no launch.
 * mt_frame_smooth / mt_frame_smooth_chunks choose between the two kernels themselves, by the launch's rows and windows per row;
 * MT_SMOOTH_SPLIT=0 in the environment keeps them to one wave per row, MT_SMOOTH_SPLIT=2..16 forces that many on rows of at least that
 * many windows. */
int    mt_frame_smooth_split(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, const long long* lengths,
                             int B, int P, long long T, int waves, mt_stream_t stream);
int    mt_frame_smooth_chunks_split(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, int NB, int P,
                                    int T, int waves, mt_stream_t stream);
/* mt_note_match_counts_clean / mt_note_match_list_clean for a grid of every decoder parameter in one pass (DESIGN.md 6c "Decoder
 * grid"): counts[b][i][j][k][c] (uint64 [B][Kf][Ko][Kk][Kc][4], zeroed on the stream) is bit for bit what the _clean entry point
 * returns for (thr_frame[i], thr_onset[j], thr_offset[k], min_frames = clean[c][0], bridge_frames = clean[c][1]) on the same inputs.
 * The threshold arrays and clean (int [Kc][2]; NULL = {{1, 0}}, then Kc must be 1) are HOST arrays, taken by value at the call (no
 * device copy, allocation or synchronisation); any order, repeats allowed.  Every axis has 1..16 values and Kf * Ko * Kk * Kc <= 64;
 * thresholds in (0, 1), min_frames 1..64, bridge_frames 0..63.  offset_logits == NULL: the onset-gated decoder, Kk must be 1 and
 * thr_offset may be NULL; onset_logits == NULL as well: the frame decoder, Ko must be 1 too and thr_onset may be NULL; offset_logits
 * without onset_logits is refused.  Every logit is read, and its sigmoid evaluated, once per launch.  Dimension limits as the
 * single-configuration calls.  Any violation: MT_EINVAL before the first device call, nothing written. */
int    mt_note_grid_counts(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame, int Kf,
                           const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const float* ref_roll,
                           const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
int    mt_note_grid_list(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame, int Kf,
                         const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const int* ref_on,
                         const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P,
                         int T, mt_stream_t stream);
/* Frame smoothing inside the decoder grid (DESIGN.md 6c "Smoothing in the decoder grid").
 *   mt_frame_smooth_paths: the Viterbi paths of mt_frame_smooth for K candidates (thr[k], on_penalty[k], off_penalty[k]) in one launch,
 *     as bit masks: bit l of paths[k][row][w] (uint64 [K][B * P][W], W = (T + 63) / 64, device) is 1 iff mt_frame_smooth at candidate k
 *     writes +64 at frame 64 w + l of that row.  Every word is written; bits at or past a row's length are 0 (a row of length 0: all
 *     zeros).  thr, on_penalty, off_penalty: HOST arrays of K entries, 1 <= K <= 16, taken by value at the call.  work: device scratch of
 *     the same size as paths, contents unspecified afterwards.  paths, work and frame_logits must not overlap.  lengths as
 *     mt_frame_smooth; B * P below 2^21, T below 2^31.  A null pointer, K outside 1..16, a threshold outside (0, 1), a penalty outside
 *     [0, 64] (NaN included), bad dims or overlapping buffers: MT_EINVAL, no launch, nothing written.  With both penalties 0 the path
 *     is the thresholded activity, bit for bit.  One launch on `stream`; no synchronisation, allocation or copy.
 *   mt_note_grid_counts_paths / mt_note_grid_list_paths: mt_note_grid_counts / mt_note_grid_list with a frame axis of Kf such
 *     candidates in place of Kf thresholds: counts[b][i][j][k][c] is what the grid gives when the frame head's activity at frame t of
 *     row r is bit t % 64 of paths[i][r][t / 64] (uint64 [Kf][B * P][(T + 63) / 64], device).  No frame logits are read.  Limits,
 *     the other arguments and the refusals are those of mt_note_grid_counts / mt_note_grid_list. */
int    mt_frame_smooth_paths(const float* frame_logits, const float* thr, const float* on_penalty, const float* off_penalty, int K,
                             const long long* lengths, int B, int P, long long T, unsigned long long* paths, unsigned long long* work,
                             mt_stream_t stream);
int    mt_note_grid_counts_paths(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                 const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                 const float* ref_roll, const long long* lengths, unsigned long long* counts, int B, int P, int T,
                                 mt_stream_t stream);
int    mt_note_grid_list_paths(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                               const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const int* ref_on,
                               const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B,
                               int P, int T, mt_stream_t stream);
/* Peak-picked onsets inside the decoder grid (DESIGN.md 6c "Peak picking in the decoder grid"): the four grid entry points with one
 * more axis, Kr candidate reaches (peak_reach: a HOST array of Kr ints, taken by value at the call).  counts[b][i][j][k][c][r]
 * (uint64 [B][Kf][Ko][Kk][Kc][Kr][4], zeroed on the stream) is bit for bit what mt_note_match_counts_peak / mt_note_match_list_peak
 * returns at peak_reach[r] and the cell's other parameters (on paths: on the activity the paths stand for), and for peak_reach[r] == 0
 * (the edge rule) what the namesake without _peak puts into the cell.  onset_logits is required; 1 <= Kr <= 16, every reach in 0..8,
 * Kf * Ko * Kk * Kc * Kr <= 64; the other arguments, limits and refusals are the namesake's.  Any violation: MT_EINVAL before the
 * first device call, nothing written. */
int    mt_note_grid_counts_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame,
                                int Kf, const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                const int* peak_reach, int Kr, const float* ref_roll, const long long* lengths, unsigned long long* counts,
                                int B, int P, int T, mt_stream_t stream);
int    mt_note_grid_list_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame,
                              int Kf, const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                              const int* peak_reach, int Kr, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                              const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
int    mt_note_grid_counts_paths_peak(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                      const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                      const int* peak_reach, int Kr, const float* ref_roll, const long long* lengths,
                                      unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
int    mt_note_grid_list_paths_peak(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                    const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                    const int* peak_reach, int Kr, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                    const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream);
/* The decoder grid in ticks (csrc/notes_grid_ticks.hip, csrc/note_ticks.hip; DESIGN.md 6c "Decoder grid in ticks"): every cell of the
 * grid of mt_note_grid_list_peak decoded into its own note list with refined onsets, and all of those lists scored in one launch.
 * mt_notes_grid_ticks: frame / onset / offset logits [B][P][T] (offset_logits NULL: the onset-gated decoder, Kk = 1), lengths int64 [B]
 * or NULL, and the axes of mt_note_grid_list_peak passed the same way (host arrays, taken by value; peak_reach is required, {0} = the
 * edge rule alone), K = Kf * Ko * Kk * Kc * Kr <= 64 cells, cell index frame-major with the reach innermost; refine_reach in [0, 8].
 * Out, cell-major: counts (int32, K*B*P) and row_off (int64, K*B*P + 1, the exclusive prefix of counts) at [(cell * B + b) * P + p], and for
 * note n of that row on_tick[row_off[..] + n] = the onset mt_refine_onsets gives the note (to the bit), off_tick = 320 * its end frame.  The
 * slice of a cell is, element for element, the table of mt_notes_batch_peak (reach R >= 1; mt_notes_batch_clean for R = 0) followed by
 * mt_refine_onsets at the cell's parameters and, with offset_logits, that of mt_heads_to_notes_peak / _clean on each recording's valid
 * frames.  capacity = the entries on_tick / off_tick can hold, in [0, 2^31): 0 counts only (the two may be NULL); when row_off[K*B*P]
 * exceeds it nothing past it is written, no note is refined, and the caller comes back with larger buffers (the one read-back of the
 * pair).  Every word of counts, row_off and the first row_off[K*B*P] entries of on_tick / off_tick is written.  64 * B * P and 320 * T
 * must fit 31 bits.  Any violation: MT_EINVAL before the first device call.  Four launches on `stream` (count, prefix, fill, refine).
 * mt_note_match_ticks_cells: mt_note_match_ticks for estimate tables of K * B * P rows against a reference of B * P rows; estimate row r
 * is matched against reference row r mod (B * P), counts[cell][b] (uint64 [K][B][4]).  The workspace holds the reference-indexed arrays
 * once per cell: mt_note_match_ticks_cells_workspace(n_est, n_ref, K) bytes, n_est = est_ptr[K*B*P].  The kernel's own checks, bit 63
 * on a bad row included, are mt_note_match_ticks' and hold per (cell, recording); K = 1 is mt_note_match_ticks. */
int    mt_notes_grid_ticks(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame, int Kf,
                           const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const int* peak_reach,
                           int Kr, int refine_reach, const long long* lengths, int B, int P, int T, int* counts, long long* row_off,
                           int* on_tick, int* off_tick, long long capacity, mt_stream_t stream);
size_t mt_note_match_ticks_cells_workspace(long long n_est, long long n_ref, int K);
int    mt_note_match_ticks_cells(const int* est_on, const int* est_off, const long long* est_ptr, const int* ref_on, const int* ref_off,
                                 const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int K, int B, int P,
                                 void* workspace, size_t workspace_bytes, mt_stream_t stream);

/* ------------------------------------------------------------------ optimizer step (training)
 * clip_grad_norm_(max_norm) + torch.optim.Adam with coupled L2 weight decay over flat f32 buffers
 * (train_transcriber.py:134-144, train_cnn.py:290); a NaN/Inf gradient norm skips the step (:137-142).
 * step = 1-based step count.  stats (2 floats, may be NULL) = {norm before clipping, 1 if stepped else 0}.
 * With data parallelism, all-reduce `grads` over RCCL before calling this: the mean, or (_ex) the SUM with
 * grad_scale = 1 / world -- the scale is applied on the fly in the norm and in the update, `grads` is not written.
 * _ex, grad_scale > 0; keep_ranges: HOST array of n_keep <= 16 ascending disjoint [lo, hi) element ranges inside [0, n), empty
 * (lo == hi) and adjacent ones allowed (NULL / 0 = everything); anything else is MT_EINVAL and nothing is written.
 * Only those elements are counted in the norm, clipped and updated; the rest keep params and moments -- torch's
 * behaviour for parameters whose .grad is None (the onset / offset heads under the reference's frame-only loss,
 * train_transcriber.py:119 + cnn_rnn_model.py:343-349: no weight decay, no moment update).                  */
size_t mt_adam_workspace_bytes(void);
int    mt_adam_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                         float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                         int step, float* stats, void* workspace, size_t workspace_bytes, mt_stream_t stream);
int    mt_adam_clip_step_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                            float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                            int step, float grad_scale, const long long* keep_ranges, int n_keep,
                            float* stats, void* workspace, size_t workspace_bytes, mt_stream_t stream);
/* _ema: mt_adam_clip_step_ex plus an exponential moving average of the parameters in the same pass (36 bytes per element instead
 * of 28).  `ema` (device, n floats, not NULL) starts as a copy of params; ema_weight = 1 - decay of this step, in (0, 1]; anything
 * else is MT_EINVAL and nothing is written.  Every element the step updates also gets ema' = fmaf(ema_weight, p' - ema, ema)
 * (p' == ema gives ema' == ema exactly).  params, exp_avg, exp_avg_sq and stats are those of mt_adam_clip_step_ex bit for bit.
 * Elements outside the keep ranges, and every element of a skipped step (stats[1] == 0), keep their `ema`.                        */
int    mt_adam_clip_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, long long n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                             int step, float grad_scale, const long long* keep_ranges, int n_keep, float ema_weight,
                             float* stats, void* workspace, size_t workspace_bytes, mt_stream_t stream);
/* Exchanges two device buffers of n floats in place (the averaged weights go under the model and back without a temporary copy).
 * a == b, n <= 0, overlapping buffers or a pointer that is not float-aligned: MT_EINVAL.  16 bytes per lane where a and b sit at
 * the same offset inside a 16-byte line, one float per lane for the misaligned head and tail and where the offsets differ.       */
int    mt_swap_f32(float* a, float* b, long long n, mt_stream_t stream);

/* ------------------------------------------------------------------ training step
 * The kernels behind `loss.backward()` of train/train_transcriber.py:130 for CNNRNNModel in train mode
 * (cnn_rnn_model.py:29-74: BatchNorm2d with BATCH statistics, ReLU, MaxPool2d((2,1)), nn.LSTM, nn.Linear),
 * orchestrated by music-transcription_amd/train_step.py.  Dense contractions of the backward pass reuse
 * mt_gemm_* and mt_conv_cl_bf16 on operands these entry points lay out.  bf16 = raw uint16 bits.          */
/* conv1 (1->32, 3x3) pre-BN statistics, recomputed from the input: sums64[c] = sum z, sums64[32+c] = sum z^2
 * over all (b, f, t); x [B][F][T] f32, w [32][9], bias [32] (raw parameters).  Zeroes sums64 first.        */
int    mt_conv1_stats(const float* x, const float* w, const float* bias, double* sums64, int B, int F, int T,
                      mt_stream_t stream);
/* sums (sum, sum of squares over `count` elements per channel) -> batch mean / rstd = 1/sqrt(var_biased+eps);
 * running_mean/var (may be NULL) updated as nn.BatchNorm2d does (momentum, unbiased variance); optionally the
 * conv parameters with the batch statistics folded in: w_folded = w*gamma*rstd [C][taps],
 * b_folded = (b-mean)*gamma*rstd + beta (pass NULL to skip).                                              */
int    mt_bn_finalize(const double* sums, double count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float* mean_out,
                      float* rstd_out, int C, const float* w, const float* b, float* w_folded, float* b_folded,
                      int taps, mt_stream_t stream);
/* z [N][C] bf16 channels-last, C in {32,64,128,256}: sums[0..C) = sum z, sums[C..2C) = sum z^2 (zeroed first). */
int    mt_bn_stats_cl(const void* z, long long N, int C, double* sums, mt_stream_t stream);
/* z [B][F][T][64] bf16 (pre-BN conv2 output) -> X[(t*B+b)*ldx + fo*64 + c] bf16 = BN + ReLU + MaxPool((2,1)). */
int    mt_bn_relu_pool_apply(const void* z, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, void* X, int ldx, int B, int F, int T, mt_stream_t stream);
/* Backward of mt_bn_relu_pool_apply: dX f32 [(t*B+b)*ldd + fo*64 + c] -> dz [B][F][T][64] bf16, dgamma[64],
 * dbeta[64] (may be NULL).  dz_lo (may be NULL): the bf16 rounding remainder of dz (dz ~= dz + dz_lo to 2^-17),
 * for the cancellation-prone conv weight gradient.  sums128: 128 doubles of scratch.                       */
int    mt_bn_pool_bwd(const float* dX, int ldd, const void* z, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, double* sums128, void* dz, void* dz_lo,
                      float* dgamma, float* dbeta, int B, int F, int T, mt_stream_t stream);
/* Pool routing that ties exactly where the f32 conv results tie (nn.MaxPool2d on f32 activations routes a tie to the first
 * row; two rows that merely round to the same bf16 value are NOT a tie): mt_conv_cl_tie is the raw convolution (bf16 in,
 * channels-last bf16 out, no activation / pool) that also writes, per frequency-row pair (2fo, 2fo+1), position and channel,
 * the order bits of its f32 accumulators -- tie[(((b*(F/2) + fo)*T + t)*(Cout/32) + co/32)*2 + {0, 1}] bit co%32 =
 * {z(2fo) > z(2fo+1), z(2fo) < z(2fo+1)} -- and mt_bn_pool_bwd_tie routes with them (tie == NULL: as mt_bn_pool_bwd).   */
int    mt_conv_cl_tie(const void* A, const void* W, const float* bias, void* out, unsigned* tie, int B, int F, int T,
                      int C1, int Cout, int KH, mt_stream_t stream);
int    mt_bn_pool_bwd_tie(const float* dX, int ldd, const void* z, const float* mean, const float* rstd,
                          const float* gamma, const float* beta, double* sums128, void* dz, void* dz_lo,
                          float* dgamma, float* dbeta, const unsigned* tie, int B, int F, int T, mt_stream_t stream);
/* Weight and bias gradient of the second conv (Conv2d(32, 64, 3, padding=1), cnn_rnn_model.py:35) from the
 * channels-last activation a1 [B][F][T][32] and the two bf16 pieces of dz [B][F][T][64] (mt_bn_pool_bwd), with the
 * POSITION as the MFMA contraction index: no im2col, no transposed copy.  n_wg persistent workgroups
 * (mt_conv2_wgrad_workgroups()) each leave a partial P[wg][64][288] (column = tap*32 + ci) and Pb[wg][64]
 * (bias: hi piece only); mt_sum_slices_f32 adds them in a fixed order.                                          */
int    mt_conv2_wgrad_workgroups(void);
int    mt_conv2_wgrad(const void* a1, const void* dz_hi, const void* dz_lo, float* P, float* Pb, int n_wg,
                      int B, int F, int T, mt_stream_t stream);
/* Layer-0 W_ih of one direction of an nn.LSTM (f32 [4H][C*F], reference feature order c*F + f: models/cnn_rnn_model.py:60-62,
 * :292-294) -> rows row0 + p*Hp + j of the projection GEMM's 16-bit operand `out` (row pitch ldo elements) in the kernels' feature
 * order f*C + c; rows j in [H, Hp) are written as zeros.  dt = MT_DT_BF16 | MT_DT_F16.  C*(F|1)*4 bytes of LDS (<= 64 KB).
 * What _pack_bilstm (music-transcription_amd/model.py) did with an index gather + cast per direction.                     */
int    mt_pack_wih_cf(const float* w, void* out, long long ldo, int row0, int H, int Hp, int C, int F, int dt,
                      mt_stream_t stream);
/* One job of mt_pack_jobs: dst rectangle [Rp][Cp] (row pitch ld elements; dt = MT_DT_BF16 | MT_DT_F16 | MT_PACK_F32) from f32 sources.
 * With r = r1*Rn2 + r2 and c = c1*Cn2 + c2: dst[r][c] = src[r1*sr1 + r2*sr2 + c1*sc1 + c2*sc2] (+ src2[same offset] when src2 != NULL)
 * where r1 < R1v, r2 < R2v, c1 < C1v, c2 < C2v, and 0 elsewhere (strides in elements, may be negative).  tr != 0: the source is
 * contiguous along the dst rows.  tile0 = number of 32 x 32 tiles of the jobs in front of this one (ascending; job 0 has 0).
 * The table replaces the per-step torch expressions of pack_train_large (music-transcription_amd/train_step_large.py), which
 * restate what the reference keeps implicit in nn.Module parameters (/root/reference/models/cnn_rnn_model.py:186-260).          */
#define MT_PACK_F32 2
typedef struct mt_pack_job {
    const void* src; const void* src2; void* dst;
    long long ld, sr1, sr2, sc1, sc2;
    int dt, Rp, Cp, Rn2, R1v, R2v, Cn2, C1v, C2v, tr, tile0, reserved;
} mt_pack_job;
/* Runs a table of njobs jobs (DEVICE memory, ntiles = total number of 32 x 32 tiles) in one launch.                        */
int    mt_pack_jobs(const void* jobs_dev, int njobs, int ntiles, mt_stream_t stream);
/* dst[c*ldd + r] = src[r*lds + c] (bf16), r < R, c < C; every dst element with c < Cd, r < ldd is written
 * (zero outside the source).                                                                               */
int    mt_transpose_bf16(const void* src, long long lds, long long R, int C, void* dst, long long ldd, int Cd,
                         mt_stream_t stream);
/* dst[i0][i1][i2][i3] (contiguous) = alpha * src[i0*s0 + i1*s1 + i2*s2 + i3*s3]: GEMM-layout gradients ->
 * the reference's parameter shapes (state_dict order).                                                     */
int    mt_gather4_f32(const float* src, float* dst, int n0, int n1, int n2, int n3, long long s0, long long s1,
                      long long s2, long long s3, float alpha, mt_stream_t stream);
/* out[r*ldo + c] = sum_z P[z*stride + r*ldp + c]: reduction of split-K partial products (fixed order).     */
int    mt_sum_slices_f32(const float* P, long long stride, int ldp, int S, float* out, int ldo, int rows,
                         int cols, mt_stream_t stream);
/* out[r] = sum_{c<n} A[r*ld + c] (bf16 rows): bias gradients from the transposed GEMM operands.            */
int    mt_rowsum_bf16(const void* A, long long ld, long long n, float* out, int rows, mt_stream_t stream);
/* conv1 + BN + ReLU + pool backward with z1 recomputed from x: da [B][F/2][T][ldc] bf16 (channels 0..31) ->
 * dW [32][9], db [32], dgamma [32], dbeta [32].  scratch384: 384 doubles.                                  */
int    mt_conv1_bwd(const float* x, const float* w, const float* bias, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, const void* da, int ldc, double* scratch384,
                    float* dW, float* db, float* dgamma, float* dbeta, int B, int F, int T, mt_stream_t stream);
/* Train-mode recurrence: as mt_lstm_bidir_fwd; additionally the ACTIVATED gates overwrite gx in place and the
 * cell states go to cx [B/32][T][2][H/8][8][32] f32 (mt_lstm_cx_bytes).                                    */
size_t mt_lstm_cx_bytes(int B, int T, int H);
int    mt_lstm_bidir_fwd_train(float* gx_inout, const float* w_hh, float* hx, float* cx, void* sync_ws,
                               size_t sync_bytes, int B, int T, int H, mt_stream_t stream);
/* hx -> X[(t*B+b)*ldx + d*Hv + j] bf16 with nn.LSTM's inter-layer (inverted) dropout p; the mask is a
 * counter-based hash of (seed, layer, element) that mt_lstm_dh_relayout regenerates.                       */
int    mt_lstm_relayout_train(const float* hx, void* X, int ldx, int B, int T, int H, int Hv, float p,
                              unsigned seed, unsigned layer, mt_stream_t stream);
/* dX f32 [(t*B+b)*ld + d*Hv + j] (gradient of the layer output) -> dh [B/32][T][2][H/8][8][32] f32.        */
int    mt_lstm_dh_relayout(const float* dX, int ld, float* dh, int B, int T, int H, int Hv, float p,
                           unsigned seed, unsigned layer, mt_stream_t stream);
/* The same dh, straight from the GEMM that produces the gradient of a layer's output (dX = dY . W^T with
 * rows m = t*B+b, N = 2*Hv columns d*Hv + j, W [roundup(2 Hv, 128) rows][K] bf16): the layer above's input
 * gradient dG_{l+1} . W_ih_{l+1} (train/train_transcriber.py:104-131 loss.backward() through nn.LSTM,
 * cnn_rnn_model.py:45-52) or the fc layer's dL . W_fc (:54, :73) -- no f32 dX round trip, no re-layout pass.
 * Entries of padded units (j >= Hv) and chunks (b >= B) are NOT written: dh must be zero there already.       */
int    mt_gemm_lstm_dh(const void* dY, int ldy, const void* W, int ldw, float* dh, int B, int T, int H, int Hv,
                       int K, float p, unsigned seed, unsigned layer, mt_stream_t stream);
/* Backward through time (both directions of one layer; persistent kernel, lstm_bwd.hip): gates/cx from
 * mt_lstm_bidir_fwd_train, dh from mt_lstm_dh_relayout, w_hh [2][4H][H] f32 -> dgx: d(gate pre-activations)
 * as bf16 MFMA-operand images (mt_lstm_dgx_bytes).  H % 16 == 0, H <= 512.  part_ws: scratch for the per-step
 * partial products of the reduce-scatter (mt_lstm_bwd_part_bytes); sync_ws: mt_lstm_sync_bytes.             */
size_t mt_lstm_dgx_bytes(int B, int T, int H);
size_t mt_lstm_bwd_part_bytes(int B, int T, int H);
int    mt_lstm_bidir_bwd(const float* gates, const float* cx, const float* dh, const float* w_hh, void* dgx,
                         void* part_ws, size_t part_bytes, void* sync_ws, size_t sync_bytes, int B, int T, int H,
                         mt_stream_t stream);
/* The poison fill of part_ws alone (any stream), and the launch with flags bit 0 = "part_ws is already poisoned": lets the
 * caller hide the 1-GB fill of the next layer's workspace under the current layer's recurrence.                       */
int    mt_lstm_bwd_poison(void* part_ws, size_t part_bytes, int B, int T, int H, mt_stream_t stream);
int    mt_lstm_bidir_bwd_ex(const float* gates, const float* cx, const float* dh, const float* w_hh, void* dgx,
                            void* part_ws, size_t part_bytes, void* sync_ws, size_t sync_bytes, int B, int T, int H,
                            int flags, mt_stream_t stream);
/* dgx -> dG [(t*B+b)*ldg + d*4H + gate*H + j] bf16 and dGT [(d*4H + gate*H + j)*ldt + t*B + b] bf16
 * (pre-zeroed by the caller: padded rows / columns are not written).  Either output may be NULL (skipped). */
int    mt_lstm_dg_unpack(const void* dgx, void* dG, int ldg, void* dGT, long long ldt, int B, int T, int H,
                         mt_stream_t stream);
/* hx -> HT[(d*rows_per_dir + k)*ld + t*B + b] = bf16 h of the forward pass's PREVIOUS step (zero at the
 * sequence boundary): W operand of dW_hh[d] = dG_d^T . Hprev_d.                                            */
int    mt_lstm_hprev_t(const float* hx, void* HT, long long ld, int rows_per_dir, int B, int T, int H,
                       mt_stream_t stream);
/* dlogits [B][P][T] f32 -> dL [(t*B+b)*128 + p] bf16 and dLT [p*ldt + t*B + b] bf16 (p < 128, zero for p >= P). */
int    mt_dlogits_pack(const float* dlogits, void* dL, void* dLT, long long ldt, int B, int P, int T,
                       mt_stream_t stream);

/* ------------------------------------------------------------------ training step of CNNRNNModelLarge
 * The pieces between the dense contractions of `loss.backward()` for models/cnn_rnn_model.py:262-348 in train mode
 * (train/train_transcriber.py:104-131), orchestrated by music-transcription_amd/train_step_large.py.  All 16-bit
 * tensors are bf16.                                                                                                  */
/* mask[b*C + c] = keep ? 1/(1-p) : 0 -- nn.Dropout2d (cnn_rnn_model.py:188,:192,:202) zeroes whole channels of a sample. */
int    mt_dropout2d_mask(float* mask, int B, int C, float p, unsigned seed, unsigned layer, mt_stream_t stream);
/* out = Dropout2d(MaxPool2d((2,1))(ReLU(BN_a(za) [+ BN_b(zb)]))) with BATCH statistics (mean / rstd from mt_bn_finalize):
 * ResidualBlock.forward (cnn_rnn_model.py:93-99: zb = the 1x1 skip branch, no pool / pool1 behind res_block1) and
 * freq_aware_conv (:196-201).  za, zb [B][F][T][C] raw conv outputs (zb, mask2d may be NULL; relu, pool flags);
 * out_mode 0: [B][Fo][T][C], 1: GEMM-A rows X[(t*B+b)*ldx + fo*C + c].  C in {32, 64, 128, 256}.                   */
int    mt_bn_act_fwd(const void* za, const float* mean_a, const float* rstd_a, const float* gamma_a, const float* beta_a,
                     const void* zb, const float* mean_b, const float* rstd_b, const float* gamma_b, const float* beta_b,
                     const float* mask2d, void* out, int out_mode, int ldx, int B, int F, int T, int C, int relu, int pool,
                     mt_stream_t stream);
/* Backward of mt_bn_act_fwd.  Gradient of the output: dout_cl (bf16 [B][Fo][T][ldd_cl]) or dout_x (f32 GEMM-row
 * layout, ldd_x) -- exactly one.  Outputs: dza [B][F][T][pitch_a], dzb [B][F][T][pitch_b] (when zb), each with an
 * optional second bf16 piece (dza_lo, dzb_lo: the rounding remainder -- BatchNorm forces sum dz = 0 and sum dz*z = 0, so
 * the conv weight gradient is a heavily cancelling sum and runs over both pieces), parameter gradients (any may be
 * NULL).  sums: 3*C doubles of scratch.
 * Pool ties route to the first row, as nn.MaxPool2d does.                                                           */
int    mt_bn_act_bwd(const void* dout_cl, int ldd_cl, const float* dout_x, int ldd_x,
                     const void* za, const float* mean_a, const float* rstd_a, const float* gamma_a, const float* beta_a,
                     const void* zb, const float* mean_b, const float* rstd_b, const float* gamma_b, const float* beta_b,
                     const float* mask2d, double* sums, void* dza, int pitch_a, void* dza_lo, void* dzb, int pitch_b, void* dzb_lo,
                     float* dgamma_a, float* dbeta_a, float* dgamma_b, float* dbeta_b,
                     int B, int F, int T, int C, int relu, int pool, mt_stream_t stream);
/* (r3) Weight gradient of a channels-last convolution (csrc/conv_wgrad.hip; replaces round 2's position planes + batched GEMM): what autograd computes for the
 * convolutions of ResidualBlock and freq_aware_conv (cnn_rnn_model.py:76-124,:186-196) under train_transcriber.py:130.
 *   out[co][ci][kh][kw] (f32, the reference's weight layout) = sum over (b, f, t) of
 *       (dz_hi + dz_lo)[b][f][t][co] * x[b][f + kh - KH/2][t + kw - KW/2][ci]            (zero outside the image)
 * dz_hi / dz_lo: bf16 [B][F][T][dz_pitch] (the gradient and its rounding remainder; dz_lo may be NULL), x: bf16
 * [B][F][T][x_pitch].  Cout % 64 == 0, Cin % 32 == 0, KH odd, KW = 3 or 1, pitches % 8 == 0, 16-byte aligned tensors,
 * F*T*pitch*2 < 2 GB.  ws: mt_conv_wgrad_ws_bytes() of scratch (partial sums per K split, added in a fixed order).      */
size_t mt_conv_wgrad_ws_bytes(int B, int F, int T, int Cout, int Cin, int KH, int KW);
int    mt_conv_wgrad(const void* dz_hi, const void* dz_lo, int dz_pitch, const void* x, int x_pitch, int B, int F, int T,
                     int Cout, int Cin, int KH, int KW, void* ws, size_t ws_bytes, float* out, mt_stream_t stream);
/* General form of mt_conv_cl_dt: A / S are channel slices (pitchA / pitchS elements between positions) and accum != 0
 * adds the result to `out` -- the input gradient of freq_aware_conv (256 output channels) is two calls.              */
int    mt_conv_cl_ex(const void* A, int pitchA, const void* S, int pitchS, const void* W, const float* bias, void* out,
                     int B, int F, int T, int C1, int C2, int Cout, int KH, int relu, int pool, int out_mode, int ldx,
                     int accum, int dt, mt_stream_t stream);
int    mt_transpose_bf16_batched(const void* src, long long lds, long long sstride, int R, int C, void* dst, long long ldd,
                                 long long dstride, int Cd, int batch, mt_stream_t stream);
/* MultiHeadAttention in train mode (cnn_rnn_model.py:128-133): Pd = dropout_p(softmax(clamp(S*scale, +-clip))) as the
 * bf16 GEMM operand; backward through dropout, softmax and clamp (no gradient where |S*scale| > clip):
 * dPd f32 [rows][ldp] -> dS bf16 [rows][Tp].  P is recomputed from S.                                               */
int    mt_attn_softmax_train(const float* S, int lds, void* P, int Tp, int T, long long rows, float scale, float clip,
                             float p, unsigned seed, unsigned layer, mt_stream_t stream);
int    mt_attn_clamped_bwd(const float* S, int lds, const float* dPd, int ldp, void* dS, int Tp, int T, long long rows,
                           float scale, float clip, float p, unsigned seed, unsigned layer, mt_stream_t stream);
/* LayerNorm(resid + proj) (cnn_rnn_model.py:322) with saved statistics stats[row] = {mean, rstd}, and its backward:
 * dy f32 -> dx f32 (the gradient of resid AND of proj); part = [mt_layernorm_residual_bwd_slices()][2][n] partial
 * column sums (row 0: dgamma, row 1: dbeta) for mt_sum_slices_f32.                                                  */
int    mt_layernorm_residual_train(const float* resid, int ldr, const float* proj, int ldp, const float* gamma,
                                   const float* beta, void* y, int ldy, float* stats, long long rows, int n, float eps,
                                   mt_stream_t stream);
int    mt_layernorm_residual_bwd_slices(void);
int    mt_layernorm_residual_bwd(const float* resid, int ldr, const float* proj, int ldp, const float* gamma,
                                 const float* stats, const float* dy, int ldd, float* dx, int ldx, float* part,
                                 long long rows, int n, mt_stream_t stream);
/* shared_fc backward through Dropout(ReLU(.)) given the layer's OUTPUT Y: dZ = (Y > 0) ? dY / (1-p) : 0 (bf16).      */
int    mt_heads_relu_dropout_bwd(const float* dY, int ldd, const void* Y, int ldy, void* dZ, int ldz, long long M, int N,
                                 float p, mt_stream_t stream);
/* dlogits f32 [NH][B][P][T] (frame / onset / offset heads) -> dL[(t*B+b)*ldl + head*P + p], dLT[(head*P+p)*ldt + t*B+b] bf16
 * (entries beyond NH*P are not written: the caller zeroes the buffers).                                             */
int    mt_dlogits_pack_heads(const float* dlogits, void* dL, int ldl, void* dLT, long long ldt, int NH, int B, int P, int T,
                             mt_stream_t stream);
/* Element-wise helpers: f32 rows -> bf16 GEMM operand (scaled); in-place inverted dropout (counter-based hash of the
 * element index m*N + n, or i); out = alpha*a + beta*b over rows.                                                   */
int    mt_f32_to_bf16_rows(const float* src, int lds, void* dst, int ldd, long long M, int N, float alpha, mt_stream_t stream);
int    mt_dropout_bf16_rows(void* X, int ld, long long M, int N, float p, unsigned seed, unsigned layer, mt_stream_t stream);
int    mt_dropout_f32(float* x, long long n, float p, unsigned seed, unsigned layer, mt_stream_t stream);
int    mt_axpby_rows_f32(const float* a, int lda, const float* b, int ldb, float* out, int ldo, long long M, int N,
                         float alpha, float beta, mt_stream_t stream);

/* ------------------------------------------------------------------ audio decode
 * PCM frames -> mono float at the target rate, replacing the host side of librosa.load(path, sr=16000, mono=True)
 * (main.py:76, data/dataset.py:124-130): channel mean + polyphase FIR, y[j] = sum_i x[i] h[(j+n_pre_remove)*down - i*up]
 * (= scipy.signal.resample_poly with the pre-padded filter h; the host builds h and the offsets, frontend.py).
 * src: interleaved [n_in][channels], fmt 0 = int16, 1 = int32 (left-aligned), 2 = float32.  soxr-exactness: unpinned. */
int    mt_resample_poly(const void* src, long long n_in, int channels, int fmt, const float* h, int h_len, int up, int down,
                        long long n_pre_remove, float* out, long long n_out, mt_stream_t stream);
/* The same sum with the filter in polyphase-major order hp[phase][k] = h[phase + k*up], taps_per_phase = ceil(h_len / up) taps per
 * phase (zero-padded): what the host path uses for its designed filter (pass band 0.913 of the lower Nyquist frequency, stop
 * band from that Nyquist frequency, >= 120 dB: ~500 taps per output at 44.1 -> 16 kHz; music-transcription_amd/transcribe.py). */
int    mt_resample_polyphase(const void* src, long long n_in, int channels, int fmt, const float* hp, int taps_per_phase, int up, int down,
                             long long n_pre_remove, float* out, long long n_out, mt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MT_HIP_H */
