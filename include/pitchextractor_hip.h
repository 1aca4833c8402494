/*
 * pitchextractor_hip.h -- C ABI of the MI355X (gfx950) JDC pitch-extractor
 * training hot path.  Built into pitchextractor_amd/libpitchextractor_hip.so.
 *
 * The reference (martinambrus/PitchExtractor) is pure Python on stock PyTorch
 * ops and has no FFI of its own; each entry point below names the reference
 * call site (file:line in the reference tree) whose work it replaces.
 *
 * Conventions (all entry points):
 *   - extern "C", plain C types only; every pointer is a DEVICE pointer owned
 *     by the caller unless the parameter name ends in _host;
 *   - `stream` is the caller's hipStream_t passed as void*; nothing here
 *     synchronises the device or allocates in steady state (plans/tables are
 *     created once by an explicit *_create);
 *   - activations are channels-last: [B][T][F][C] float32 ("NHWC", T = frames,
 *     F = mel/frequency axis, C = channels); conv weights are handed over in
 *     the reference's OIHW order and repacked on the device;
 *   - return value: 0 = ok, negative = invalid argument (PE_E_*), positive =
 *     hipError_t of a failed runtime call;
 *   - MFMA-bound entry points take the product form as their first parameter,
 *     `int products` (enum pe_products below), and keep one contract in every
 *     form; entry points that read or write the conv stack's activations also
 *     take `int act16` (0 = fp32 tensors, 1 = bf16 tensors, see "bf16
 *     ACTIVATION STORAGE").  A form or activation type that none of an entry
 *     point's kernels serves returns PE_E_UNSUPPORTED; a `products` value
 *     outside the enum returns PE_E_ARG.  Both are answered before any
 *     pointer is looked at; a served form sees the entry point's own argument
 *     checks first.  Served forms (act16 = 1: under PE_PROD_BF16 only):
 *
 *       entry point                                   NATIVE X3 H2 BF16 F16  act16
 *       pe_gemm_nt, pe_gemm_tn                           x    x  x   x    x    x
 *       pe_conv3x3_fwd, pe_conv3x3_wgrad                 x    x  x   x    x    x
 *       pe_conv3x3_fwd_wf                                -    x  x   x    x    x
 *       pe_wfrag_pack, pe_wfrag_bytes (else 0 bytes)     -    x  x   x    x
 *       pe_lstm_whh_grad                                 x    x  x   x    x
 *       pe_lstm_fwd_persistent, pe_lstm_bwd_persistent   -    x  -   x    x
 *       pe_attn_fwd, pe_attn_bwd                         x    -  -   x    -
 */
#ifndef PITCHEXTRACTOR_HIP_H
#define PITCHEXTRACTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_OK 0
#define PE_E_ARG (-1)       /* bad size / null pointer            */
#define PE_E_UNSUPPORTED (-2) /* shape outside what the kernels take */
#define PE_E_WORKSPACE (-3) /* workspace too small                 */

/* How the products of an MFMA-bound entry point run; accumulation is fp32 and tensors in memory keep their type in
 * every form. */
enum pe_products {
  PE_PROD_NATIVE = 0, /* fp32 products on v_mfma_f32_32x32x2_f32 */
  PE_PROD_X3 = 1,     /* fp32-accurate: operands split exactly into three bf16 terms, six bf16 MFMAs per product */
  PE_PROD_H2 = 2,     /* two fp16 terms of each operand scaled by a power of two, three fp16 MFMAs (the default) */
  PE_PROD_BF16 = 3,   /* operands rounded to bf16 (mixed precision) */
  PE_PROD_F16 = 4     /* operands rounded to IEEE half (mixed precision; the caller scales the loss) */
};

/* library / device ------------------------------------------------------- */
int pe_abi_version(void);
/* number of HIP devices visible, or negative hipError_t */
int pe_device_count(void);
/* *stream_out = a new non-blocking stream of the current device at its lowest priority (side work that must not
 * compete with the critical chain); created in this library's HIP runtime, owned by the caller. */
int pe_stream_create_low_priority(void** stream_out);

/* ---- mel front end ---------------------------------------------------------
 * Replaces MelDataset.to_melspec = torchaudio.transforms.MelSpectrogram(
 *   sample_rate=24000, n_fft=1024, win_length=1024, hop_length=300, n_mels=80)
 * (meldataset.py:34-40,58-77,644) and the log/normalise of meldataset.py:650,
 * batched over utterances.  center=True, reflect pad n_fft/2, periodic Hann,
 * power 2, HTK mel scale, f_min 0, f_max sr/2, norm None.
 */
typedef struct pe_mel_plan pe_mel_plan;
/* Only n_fft == win_length == 1024 is implemented (PE_E_UNSUPPORTED otherwise). */
int pe_mel_plan_create(pe_mel_plan** plan, int sample_rate, int n_fft, int win_length,
                       int hop_length, int n_mels, float f_min, float f_max);
int pe_mel_plan_destroy(pe_mel_plan* plan);
/* frames produced for an n_samples utterance: 1 + n_samples / hop */
int pe_mel_num_frames(const pe_mel_plan* plan, int n_samples);
/* wave: [batch] rows of n_samples float32, row stride wave_stride (elements).
 * out:  element (b, m, t) at out[b*out_sb + m*out_sm + t*out_st], for
 *       t < out_frames.  Frames t >= 1 + n_samples/hop are written as pad_value
 *       (Collater zero padding, meldataset.py:806-816).
 * log_mode 0: mel power; 1: (log(log_eps + mel) - mean) / std. */
int pe_mel_forward(const pe_mel_plan* plan, const float* wave, int batch, int n_samples,
                   long wave_stride, float* out, long out_sb, long out_sm, long out_st,
                   int out_frames, int log_mode, float log_eps, float mean, float std,
                   float pad_value, void* stream);
/* Ragged batch: utterance b has n_samples[b] <= max_samples samples (device int array) and, when
 * frame_start != NULL, output frame t shows source frame t + frame_start[b] -- the random crop of
 * meldataset.py:668-672 applied on the frame axis without recomputing anything.  Items with
 * n_samples[b] <= n_fft/2 produce padding only. */
int pe_mel_forward_ragged(const pe_mel_plan* plan, const float* wave, int batch, int max_samples,
                          long wave_stride, const int* n_samples, const int* frame_start, float* out,
                          long out_sb, long out_sm, long out_st, int out_frames, int log_mode,
                          float log_eps, float mean, float std, float pad_value, void* stream);
/* Chunked batch (inference.predict_f0_batch): item i of n_chunks is described by row i of `chunks` (n_chunks x
 * pe_mel_chunk_fields() int64 on the device; host_chunks its host copy) = {sample offset of its row in wave, samples
 * of that row, first source frame}: output frame t < chunk_size of item i shows frame chunks[i][2] + t of the row
 * at wave + chunks[i][0], reflect-padded at the ROW's ends; frames at or past the row's 1 + n / hop are pad_value.
 * Written at caller-given strides like pe_mel_forward (out_sm == 1 gives the model's (chunk, 1, frames, mels) input
 * directly).  Checked on host_chunks before any device call: PE_E_ARG for a null pointer, a negative entry, a row of
 * at most n_fft/2 samples or one that ends past wave_elems; PE_E_UNSUPPORTED for more than 65535 chunks or a row of
 * 2^31 samples or more. */
int pe_mel_chunk_fields(void);
int pe_mel_forward_chunks(const pe_mel_plan* plan, const float* wave, long wave_elems, const long* chunks,
                          const long* host_chunks, int n_chunks, int chunk_size, float* out, long out_sb,
                          long out_sm, long out_st, int log_mode, float log_eps, float mean, float std,
                          float pad_value, void* stream);
/* Backward of pe_mel_forward / pe_mel_forward_ragged with respect to the wave (the chunk-table mode has none).
 * grad_out: d loss / d out, element (b, m, t) at grad_out[b*g_sb + m*g_sm + t*g_st] for t < out_frames, read at the
 *       strides the forward writes `out` at.  Positions the forward wrote as padding (source frame t + frame_start[b]
 *       at or past 1 + n/hop) carry no gradient and are never read: a NaN there does not reach grad_wave.
 * grad_wave: [batch] rows of n_samples (max_samples) float32, row stride grad_wave_stride; every element is written
 *       exactly once (no atomics: the caller need not clear it), samples at or past a ragged row's length and rows
 *       of at most n_fft/2 samples as 0.
 * The spectrum and the mel of every frame are recomputed from `wave`; `mean` does not enter the gradient.  A row's
 * gradient is the same bits alone, in a batch of any size and at any row stride.  Two launches.
 * workspace: pe_mel_backward_workspace_bytes(plan, batch, n_samples or max_samples, out_frames) bytes, never read
 * before written (0 for a null plan or a non-positive size).
 * Checked on the host before any device call: PE_E_ARG for a null pointer, a non-positive size, std == 0, a row
 * stride below the row length or a fixed-batch n_samples <= n_fft/2; PE_E_UNSUPPORTED for batch > 65535, rows of
 * more than 2^30 samples, a hop whose block segment does not fit in LDS, or a filterbank with more than two filters
 * on one bin; PE_E_WORKSPACE when workspace_bytes is too small. */
size_t pe_mel_backward_workspace_bytes(const pe_mel_plan* plan, int batch, int max_samples, int out_frames);
int pe_mel_backward(const pe_mel_plan* plan, const float* wave, int batch, int n_samples, long wave_stride,
                    const float* grad_out, long g_sb, long g_sm, long g_st, int out_frames, int log_mode,
                    float log_eps, float mean, float std, float* grad_wave, long grad_wave_stride,
                    void* workspace, size_t workspace_bytes, void* stream);
int pe_mel_backward_ragged(const pe_mel_plan* plan, const float* wave, int batch, int max_samples,
                           long wave_stride, const int* n_samples, const int* frame_start,
                           const float* grad_out, long g_sb, long g_sm, long g_st, int out_frames,
                           int log_mode, float log_eps, float mean, float std, float* grad_wave,
                           long grad_wave_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ---- stitching chunk outputs into rows (inference.predict_f0_batch) --------------------------------------------------
 * pe_stitch_chunks: x is (n_chunks, chunk_size, C) float32, frame (k, f) at x + (k * chunk_size + f) * ld_x, unit
 * stride over the C columns, 1 <= C <= 1024, ld_x >= C; det (nullable) is (n_chunks, chunk_size) dense.  The
 * destination is n_dst frames, frame d at out + d * ld_out (ld_out >= C), and det_out[d] (given exactly when det is).
 * runs (n_runs x pe_stitch_run_fields() int64 on the device; host_runs its host copy) = per run {chunk a, frame in a,
 * first destination frame, length, n_ov, j0, chunk b, frame in b}, sorted by destination and not overlapping.
 * n_ov == 0: destination frame dst + i is a copy of frame (a, fa + i), no arithmetic.  n_ov > 0 (a seam): with
 * float32 w = (j0 + i + 1) / (n_ov + 1) it is A + w * (B - A) in float32, A = frame (a, fa + i), B = frame (b, fb + i);
 * j0 + length <= n_ov.  Destination frames that no run covers are written as 0 in every column.  Every destination
 * element is written exactly once, by one launch, without atomics.  Checked on host_runs before any device call:
 * PE_E_ARG for a null pointer, a negative size, a run that leaves its chunk, the chunk batch or the destination, runs
 * out of order or overlapping, or det given without det_out (or the reverse); PE_E_UNSUPPORTED for C outside
 * 1 .. 1024. */
int pe_stitch_run_fields(void);
int pe_stitch_chunks(const float* x, long ld_x, const float* det, const long* runs, const long* host_runs,
                     int n_runs, int n_chunks, int chunk_size, int C, float* out, long ld_out, float* det_out,
                     long n_dst, void* stream);


/* ---- dense fp32 GEMMs on the MFMA engine -----------------------------------
 * pe_gemm_nt: C[M][N] = A[M][K] . B[N][K]^T + bias0[n] + bias1[n] (+ C when accumulate).
 *   nn.Linear / LSTM input projection (model.py:220-227) / 1x1 convs (model.py:53,167).
 * pe_gemm_tn: C[M][N] = sum_k A[k][m] * B[k][n] (+ C): weight gradients, k split across
 *   workgroups into workspace slabs that are reduced in a fixed order (deterministic).
 * Every form of pe_products.  PE_PROD_X3: x = hi + mid + lo exactly in bf16 and six of the nine cross products are
 * accumulated; the dropped terms are below 2^-23 of each product, i.e. under the rounding of an fp32 product.
 * PE_PROD_H2: x * s = hi + lo with hi = RN_f16(x s), lo = RN_f16(x s - hi); hi_a lo_b + lo_a hi_b + hi_a hi_b is
 * accumulated and lo_a lo_b (<= 2^-24 |a b|) dropped: per-product error <= 2^-21 |a b|, unbiased.  Each operand tensor
 * carries a power-of-two scale s = 2^(140 - E), E = biased exponent of its largest magnitude, which the kernel derives
 * from *amax_a / *amax_b (device words holding the IEEE bits of max |x|: pe_absmax, or the epilogue of the kernel that
 * produced the tensor); a value smaller than the tensor's true maximum makes fp16 overflow possible, a larger one only
 * costs resolution (2^-38 of the stated maximum, absolute).  The scale words are read under PE_PROD_H2 only (PE_E_ARG
 * without them) and may be NULL otherwise.  PE_PROD_BF16 / PE_PROD_F16 round the operands on the way into LDS
 * (reference trainer.py:103 autocast).  act16 = 1 (PE_PROD_BF16 only): A and C (nt) or A and B (tn) are bf16 tensors. */
int pe_gemm_nt(int products, int act16, const void* A, long lda, const float* B, long ldb, void* C, long ldc, int M,
               int N, int K, const float* bias0, const float* bias1, int accumulate, const unsigned* amax_a,
               const unsigned* amax_b, void* stream);
/* out[0] = IEEE bits of max |x| over a [rows][cols] matrix with leading dimension ld (cols, ld % 4 == 0, x 16-byte
 * aligned); zeroes out[0] first.  Exact and order-independent (integer max of the magnitudes' bit patterns). */
int pe_absmax(const float* x, long rows, int cols, long ld, unsigned* out, void* stream);
/* out[s] = IEEE bits of max |base[seg_off[s] .. + seg_len[s])| for s < nseg, one launch (seg_off / seg_len: device
 * arrays; every parameter of a model that lives in one flat buffer). */
int pe_absmax_segments(const float* base, const long* seg_off, const long* seg_len, int nseg, unsigned* out,
                       void* stream);
size_t pe_gemm_tn_workspace_bytes(int M, int N, int K);
int pe_gemm_tn(int products, int act16, const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M,
               int N, int K, int accumulate, float* workspace, size_t workspace_bytes, const unsigned* amax_a,
               const unsigned* amax_b, void* stream);
int pe_transpose2d(const float* in, float* out, int rows, int cols, void* stream);

/* ---- 3x3 / pad 1 convolutions (model.py:23-28,157-161), channels-last -------
 * pe_conv3x3_repack: OIHW weights -> w_fwd [Cout][kh][kw][Cin] and/or the flipped, transposed
 *   w_dgrad [Cin][2-kh][2-kw][Cout] (either may be NULL).
 * pe_conv3x3_fwd:  y[B][T][F][N] (+)= conv(x[B][T][F][C], w_packed[N][9*C]); the data gradient
 *   is the same call with (dy, w_dgrad, C = Cout, N = Cin).
 * pe_conv3x3_wgrad: dw (OIHW) = sum_pixels dy (x) shifted x.
 * pe_conv3x3_c1_*: the Cin = 1 first layer; x element (b,t,f) at x[b*sb + t*st + f*sf].
 * Forms and scale words as pe_gemm_nt (amax_x / amax_w / amax_dy: the absmax words of x, the weight and dy). */
int pe_conv3x3_repack(const float* w_oihw, float* w_fwd, float* w_dgrad, int Cout, int Cin, void* stream);
int pe_conv3x3_fwd(int products, int act16, const void* x, const float* w_packed, void* y, int B, int T, int F, int C,
                   int N, int accumulate, const unsigned* amax_x, const unsigned* amax_w, void* stream);
/* Weights pre-packed as MFMA B-operand fragments in the terms of `products` (x3: three exact bf16 terms; h2: two fp16
 * terms of w * 2^(140 - E), E from *amax = pe_absmax of w; bf16 / f16: one RNE-rounded term; no native form).  w is
 * [N][K] row-major fp32 (K % 16 == 0); fragment (kb, nb, term) holds, for lane 32 h + r, w[32 nb + r][16 kb + 8 h .. + 7]
 * in 16 bytes, the 64 lanes contiguous (1 KB).  The halo convolution pe_conv3x3_fwd_wf then loads its weight operands
 * straight from L2 into registers: LDS carries only activations.  It takes fragments packed for the same form (under
 * h2, with the same *amax_w).
 * pe_conv3x3_wf_supported: 1 if (F, C, N) is served by the fragment-fed kernel (else use pe_conv3x3_fwd).
 * pe_wfrag_bytes: 0 for a form without fragments or K % 16 != 0. */
size_t pe_wfrag_bytes(int products, int N, int K);
int pe_wfrag_pack(int products, const float* w, long ld, int N, int K, const unsigned* amax, void* wfrag, void* stream);
int pe_conv3x3_wf_supported(int F, int C, int N);
int pe_conv3x3_fwd_wf(int products, int act16, const void* x, const void* wfrag, void* y, int B, int T, int F, int C,
                      int N, int accumulate, double* bn_partials, const unsigned* amax_x, const unsigned* amax_w,
                      void* stream);
/* bn_partials (optional): [pe_conv3x3_wf_stat_parts(B,T,F)][2][N] doubles -- per pixel tile, the column sums and sums
 * of squares of the FINAL outputs; pe_bn_finalize_stats turns them into the statistics of the BatchNorm that follows
 * (no separate pass over the activation). */
int pe_conv3x3_wf_stat_parts(int B, int T, int F);
size_t pe_conv3x3_wgrad_workspace_bytes(int B, int T, int F, int Cin, int Cout);
int pe_conv3x3_wgrad(int products, int act16, const void* x, const void* dy, float* dw_oihw, int B, int T, int F,
                     int Cin, int Cout, float* workspace, size_t workspace_bytes, const unsigned* amax_x,
                     const unsigned* amax_dy, void* stream);
/* first convolution (1 -> 64 channels).  bn_partials (nullable): [pe_conv3x3_c1_stat_parts()][2][64] doubles that
 * receive per-workgroup sums / sums of squares of the output channels (input of pe_bn_finalize_stats). */
int pe_conv3x3_c1_stat_parts(int B, int T, int F);
int pe_conv3x3_c1_fwd(int act16, const float* x, long sb, long st, long sf, const float* w_oihw, void* y, int B, int T,
                      int F, double* bn_partials, void* stream);
int pe_conv3x3_c1_wgrad(int act16, const float* x, long sb, long st, long sf, const void* dy, float* dw_oihw, int B,
                        int T, int F, float* workspace, size_t workspace_bytes, void* stream);
/* data gradient of the first convolution: dx[b][t][f] = sum_{co,i,j} w[co][0][i][j] * dy[b][t-i+1][f-j+1][co], dy
 * channels-last [B][T][F][64] (zero outside the grid), dx dense [B][T][F] fp32.  One pass over dy, no atomics, the
 * same bits however large B is.  act16: 0 = fp32 dy, 1 = bf16, 2 = fp16.  F % 4 != 0 or B*T*F near 2^31:
 * PE_E_UNSUPPORTED. */
int pe_conv3x3_c1_dgrad(int act16, const void* dy, const float* w_oihw, float* dx, int B, int T, int F, void* stream);

/* ---- fused self-attention (model.py:231-239: nn.MultiheadAttention inside TransformerEncoderLayer) -------------
 * qkv [B*T][ld_qkv] packed projections (Q | K | V, head h at columns h*dh of each part); o [B*T][ld_o] merged
 * heads; lse [B*H*T]; masks [B*H*T][T] bytes (1 = kept), element quad i = row * T/4 + key/4 draws Philox counter
 * offset + i exactly like pe_dropout_fwd on the (B*H*T) x T probability matrix.  One workgroup per (batch, head),
 * scores stay in registers; the backward recomputes them from lse.  pe_attn_supported: 1 for T = 192, dh = 64
 * (other shapes: pe_bgemm + pe_softmax_*).
 * PE_PROD_NATIVE: fp32 MFMAs.  PE_PROD_BF16: the matmul operands (Q, K, V, dO, the probabilities and the score
 * gradients) rounded to bf16 and multiplied on v_mfma_f32_16x16x16_bf16, as torch.autocast runs the attention of
 * trainer.py:226-235; softmax, log-sum-exp, accumulation and every tensor in memory stay fp32, masks and Philox counters
 * as above.  No other form. */
int pe_attn_supported(int T, int dh);
int pe_attn_fwd(int products, const float* qkv, long ld_qkv, float* o, long ld_o, float* lse,
                const unsigned char* mask_in, unsigned char* mask_out, int B, int T, int H, int dh, float scale,
                float p_drop, unsigned long long seed, unsigned long long offset, void* stream);
int pe_attn_bwd(int products, const float* qkv, long ld_qkv, const float* o, const float* d_o, long ld_o,
                const float* lse, const unsigned char* mask, float* dqkv, int B, int T, int H, int dh, float scale,
                float p_drop, void* stream);

/* ---- BatchNorm2d (train statistics) / LeakyReLU / MaxPool2d((1,k)) / dropout -
 * Activations are [rows = B*T][F][C].  pe_bn_train_stats: batch mean / biased variance over all
 * n_pix = rows*F pixels (model.py:25,37,54,150,159), running-stat update with `momentum` and the
 * unbiased variance, plus the fused affine scale = gamma*invstd, shift = beta - mean*scale.
 * pe_bn_act_pool_fwd: y = maxpool_k(lrelu(x*scale + shift)) written at
 *   y[(row*Fout + fo)*ldy + coff + c] (model.py:36-41,148-153).
 * pe_bn_act_pool_bwd: gradient of that block w.r.t. x, gamma, beta.  eval_mode = 0: train-mode BN (mean / invstd are
 *   the batch statistics).  eval_mode = 1: the forward ran on running statistics (pe_bn_eval_affine filled scale, shift,
 *   mean = running_mean, invstd = 1/sqrt(running_var + eps)): dx = scale * lrelu'(z) * unpool(dy) with no mean or
 *   projection term, dgamma = sum dz * (x - mean) * invstd, dbeta = sum dz -- nn.BatchNorm2d.eval() under autograd.
 *   With eval_mode = 1, dgamma and dbeta may both be NULL: no per-channel reduction runs and workspace may be NULL.
 * amax_out (optional, these two and pe_maxpool_bwd_add): a device word the caller zeroed; the pass max-merges the
 *   IEEE bits of the largest magnitude it stored into it (atomicMax), which is the scale source an "h2" product
 *   reading the output needs (PE_PROD_H2) -- no separate pe_absmax pass.  pe_maxpool_bwd_add merges the values it
 *   rewrote into dx's word: the result bounds max |dx| from above.
 * act16 (every pass of this section but pe_bn_finalize_stats / pe_bn_eval_affine): 0 = fp32 activation tensors, 1 =
 *   bf16 (see "bf16 ACTIVATION STORAGE").  pe_bn_act_pool_bwd takes pool in {1, 2, 4} (the widths the model pools by),
 *   for both storage types; any other width is PE_E_UNSUPPORTED.  The forward pass takes any pool > 0. */
size_t pe_bn_workspace_bytes(int C);
int pe_bn_train_stats(int act16, const void* x, long n_pix, int C, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                      float* scale, float* shift, void* workspace, size_t workspace_bytes, void* stream);
int pe_bn_finalize_stats(const double* partials, int nparts, long n_pix, int C, const float* gamma, const float* beta,
                         float eps, float momentum, float* running_mean, float* running_var, float* mean,
                         float* invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes,
                         void* stream);   /* workspace: pe_bn_workspace_bytes(C) */
int pe_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int C, float* scale, float* shift, float* mean,
                      float* invstd, void* stream);
int pe_bn_act_pool_fwd(int act16, const void* x, const float* scale, const float* shift, float slope, void* y, long rows,
                       int Fin, int C, int pool, long ldy, int coff, unsigned* amax_out, void* stream);
int pe_bn_act_pool_bwd(int act16, const void* x, const void* dy, const float* scale, const float* shift,
                       const float* mean, const float* invstd, float slope, void* dx, float* dgamma, float* dbeta,
                       long rows, int Fin, int C, int pool, long lddy, int coff, int eval_mode, void* workspace,
                       size_t workspace_bytes, unsigned* amax_out, void* stream);
/* detector-branch MaxPool2d((1,40|20|10)) (model.py:45-49,103-105) into a channel slice.  argmax_out (optional,
 * [rows * (Fin / pool)][C] bytes): the window position of each maximum (the first one, as torch's backward routes it);
 * pe_maxpool_bwd_add given that array as `argmax` scatters dy without reading x (x may then be NULL). */
int pe_maxpool_fwd(int act16, const void* x, void* y, long rows, int Fin, int C, int pool, long ldy, int coff,
                   unsigned char* argmax_out, void* stream);
int pe_maxpool_bwd_add(int act16, const void* x, const unsigned char* argmax, const void* dy, void* dx, long rows,
                       int Fin, int C, int pool, long lddy, int coff, unsigned* amax_out, void* stream);
/* A detector tap folded into the BN passes of the block that reads the same tensor: one read of x leaves y / amax_out as
 * pe_bn_act_pool_fwd does AND the plain max-pool of x over tap_pool (at tap_y[(row*(Fin/tap_pool) + w)*tap_ldy +
 * tap_coff + c]) with its positions (tap_arg, optional) as pe_maxpool_fwd does; the backward writes dx with the tap
 * gradient already added and amax_out as pe_bn_act_pool_bwd followed by pe_maxpool_bwd_add(argmax = tap_arg) leave
 * them.  Bit for bit the two passes they replace.  Served (pe_bn_act_pool_tap_supported = 1, else PE_E_UNSUPPORTED):
 * pool in {1, 2, 4}, tap_pool % pool == 0, Fin % tap_pool == 0, tap_pool <= 255 when positions are wanted, rows * Fin
 * below 2^31, and the alignment of the plain passes. */
int pe_bn_act_pool_tap_supported(long rows, int Fin, int C, int pool, int tap_pool, int with_arg);
int pe_bn_act_pool_tap_fwd(int act16, const void* x, const float* scale, const float* shift, float slope, void* y,
                           long rows, int Fin, int C, int pool, long ldy, int coff, unsigned* amax_out, void* tap_y,
                           long tap_ldy, int tap_coff, int tap_pool, unsigned char* tap_arg, void* stream);
int pe_bn_act_pool_tap_bwd(int act16, const void* x, const void* dy, const float* scale, const float* shift,
                           const float* mean, const float* invstd, float slope, void* dx, float* dgamma, float* dbeta,
                           long rows, int Fin, int C, int pool, long lddy, int coff, int eval_mode, void* workspace,
                           size_t workspace_bytes, unsigned* amax_out, const void* tap_dy, long tap_lddy, int tap_coff,
                           int tap_pool, const unsigned char* tap_arg, void* stream);
/* nn.Dropout (model.py:40,56; LSTM inter-layer): Philox4x32-10 keyed by (seed, offset + quad index);
 * mask bytes (1 = kept) can be exported (mask_out) or replayed (mask_in). */
int pe_dropout_fwd(int act16, const void* x, long ldx, void* y, long ldy, const unsigned char* mask_in,
                   unsigned char* mask_out, long rows, int cols, float p, unsigned long long seed,
                   unsigned long long offset, void* stream);
/* (B,256,T,2) -> permute(0,2,1,3) -> (B,T,512) of model.py:93,112 and its transpose; seq is fp32 in both */
int pe_nhwc_to_seq(int act16, const void* x, long ldx, int coff, float* seq, long rows, int C, void* stream);
int pe_seq_to_nhwc(int act16, const float* seq, void* x, long ldx, int coff, long rows, int C, int accumulate,
                   void* stream);
int pe_copy2d(int act16, const void* src, long lds, void* dst, long ldd, long rows, int cols, int accumulate,
              void* stream);

/* ---- LSTM recurrence (nn.LSTM of model.py:218-227; gates i,f,g,o; zero initial state) ----
 * Up to 4 cells (directions x models) advance together, one launch per time step.
 * pe_lstm_fwd:  gates[c] holds X.W_ih^T + b_ih + b_hh on entry ([B][T][4H]) and the activated gates
 *   on exit; y[c] (already offset to this direction's H-wide slice, row stride ldy) receives h_t,
 *   cbuf[c] ([B][T][H]) the cell states.
 * pe_lstm_bwd:  gates[c] holds activated gates on entry and d(pre-activation gates) on exit;
 *   whh_t[c] = W_hh^T [H][4H]; dy[c] = dL/dh (same addressing as y); dcarry[c] = [B][H] scratch. */
int pe_lstm_fwd(int ncells, const float* const* whh, float* const* gates, float* const* y,
                float* const* cbuf, const int* reverse, long ldy, int B, int T, int H, void* stream);
int pe_lstm_bwd(int ncells, const float* const* whh_t, float* const* gates, const float* const* cbuf,
                const float* const* dy, float* const* dcarry, const int* reverse, long lddy, int B, int T,
                int H, void* stream);
/* Persistent variants: one launch for all T steps, W_hh slice resident in registers, group barriers
 * between steps (agent-scope release/acquire).  `sync` = pe_lstm_persistent_sync_bytes() of device
 * memory, zero-initialised once by the caller: the group counters, then the backward kernel's exchange
 * region (the step's gate gradients in MFMA fragment order, two slots per batch tile).  Word 0 is a
 * sticky error flag (non-zero = a bounded spin timed out: results invalid).  Only when pe_lstm_persistent_supported() returns 1. */
size_t pe_lstm_persistent_sync_bytes(int ncells, int B);
int pe_lstm_persistent_supported(int ncells, int B, int H);
/* Persistent recurrences (H = 384): ONE launch per layer for all cells, W_hh resident on chip, workgroups hand h /
 * partial dh tiles to each other through memory.  The recurrent products are 16-bit-term MFMAs: PE_PROD_X3 (the exact
 * three-term bf16 split, fp32-accurate), PE_PROD_BF16 / PE_PROD_F16 (W_hh and the h / dgates rows rounded to 16 bits,
 * fp32 accumulate and cell state).  There is no native-fp32 or h2 persistent form (PE_E_UNSUPPORTED): pe_lstm_fwd /
 * pe_lstm_bwd (one launch per time step) serve those modes and every shape pe_lstm_persistent_supported() declines.
 * dbias_rows (nullable): per cell a [pe_lstm_bwd_persistent_dbias_rows()][4H] buffer that receives the per-batch-tile
 * column sums of the gate gradients (their row sum is dL/db_ih = dL/db_hh), replacing a pe_colsum pass over the
 * [B*T][4H] gradient tensor.
 * dgates_amax (nullable): per cell a device word the caller zeroed; the kernel max-merges the IEEE bits of the largest
 * gate-gradient magnitude into it (the "h2" scale source of the dX / dW products). */
int pe_lstm_bwd_persistent_dbias_rows(int ncells, int B, int T, int H, long lddy);
int pe_lstm_fwd_persistent(int products, int ncells, const float* const* whh, float* const* gates, float* const* y,
                           float* const* cbuf, const int* reverse, long ldy, int B, int T, int H, unsigned* sync,
                           void* stream);
int pe_lstm_bwd_persistent(int products, int ncells, const float* const* whh_t, float* const* gates,
                           const float* const* cbuf, const float* const* dy, const int* reverse, long lddy, int B,
                           int T, int H, float* const* dbias_rows, unsigned* const* dgates_amax, unsigned* sync,
                           void* stream);
/* Diagnostic (tools/stamp_lstm.py): 1 = run the stamped instantiations of the x3 kernels (s_memtime per region of an
 * iteration; grid <= 128 workgroups).  Returns the previous setting.  The product path never calls it. */
int pe_lstm_configure_stamps(int enable);
size_t pe_lstm_whh_grad_workspace_bytes(int B, int T, int H);
/* dW_hh = sum over batch and time of dgates^T . y shifted one step; every form of pe_products (scale words as
 * pe_gemm_nt: amax_dgates, amax_y) */
int pe_lstm_whh_grad(int products, const float* dgates, const float* y, long ldy, float* dwhh, int B, int T, int H,
                     int reverse, float* workspace, size_t workspace_bytes, const unsigned* amax_dgates,
                     const unsigned* amax_y, void* stream);
size_t pe_colsum_workspace_bytes(int cols);
int pe_colsum(const float* x, long rows, int cols, long ld, float* out0, float* out1, void* workspace,
              size_t workspace_bytes, void* stream);

/* ---- heads, losses, optimiser ------------------------------------------------
 * pe_head_fwd: y[r] = sum_{o<n_out} (x[r].w[o] + bias[o]) -- Linear(D,1) (n_out 1) and
 *   Linear(D,2).sum(-1) (n_out 2) of model.py:67-70,96-98,115-117.
 * pe_f0_sil_loss: out3 = {lambda*SmoothL1 + BCE, lambda*SmoothL1, BCE} (train.py:104-106,
 *   trainer.py:237-239) and the gradients w.r.t. both prediction vectors (times grad_scale).
 * pe_adamw_step: torch.optim.AdamW (optimizers.py:55-62) on a flat buffer; the caller passes the
 *   current lr / beta1 (OneCycleLR rewrites both every step) and the bias corrections
 *   1 - beta^step computed in double (step >= 1: a correction outside (0, 1] is PE_E_ARG -- step 0 would make
 *   the step size infinite). Gradients are multiplied by grad_scale first. */
int pe_head_fwd(const float* x, long ldx, const float* w, const float* bias, int n_out, float* y, long R,
                int D, void* stream);
size_t pe_head_bwd_workspace_bytes(int D);
/* dw and db both NULL: dx only (x and the workspace are not read). */
int pe_head_bwd(const float* x, long ldx, const float* w, const float* dy, int n_out, float* dx, long lddx,
                float* dw, float* db, long R, int D, void* workspace, size_t workspace_bytes, void* stream);
int pe_f0_sil_loss(const float* f0_pred, const float* f0, const float* sil_pred, const float* sil,
                   float lambda_f0, long R, float grad_scale, float* out3, float* d_f0_pred,
                   float* d_sil_pred, void* stream);
/* 360-bin F0 classification loss (build-defined, the reference has none): CREPE bins
 * bin = clamp(rint((1200 log2(f0/10) - 1997.3794084376191) / 20), 0, C-1) on voiced frames (f0 > 0), CE averaged
 * over voiced frames, total = lambda * CE + BCEWithLogits(sil).  out4 = {total, lambda*CE, BCE, voiced count}. */
size_t pe_f0_bins_ce_workspace_bytes(long R);
int pe_f0_bins_ce_loss(const float* logits, long ldl, int C, const float* f0, const float* sil_pred,
                       const float* sil, float lambda_f0, long R, float grad_scale, float* out4,
                       float* d_logits, long ldd, float* d_sil_pred, float* workspace, size_t workspace_bytes,
                       void* stream);
/* skip_if_nonzero (nullable): a device float; when it is non-zero at execution time the launch updates nothing (the
 * trainer's fault word, agreed across ranks inside the gradient all-reduce: no host round trip before the update). */
int pe_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, double bias_correction1,
                  double bias_correction2, float grad_scale, const float* skip_if_nonzero, void* stream);
/* GradScaler support (reference trainer.py:241-244): *flag = 1 if any of x[0..n) is inf or nan, else 0. */
int pe_nonfinite_flag(const float* x, long n, int* flag, void* stream);

/* ---- bf16 ACTIVATION STORAGE for mixed precision (`act16 = 1`) -----------------------------------------------------
 * The reference's autocast keeps conv / linear outputs and what backward saves of them in 16 bits (trainer.py:226-235,
 * README.md:36).  Entry points with an `act16` parameter store the conv stack's activation and activation-gradient
 * tensors (x, y, dy, dx, the GEMM operand A and result C) as bf16 in HBM when it is 1: half the bytes of every
 * BatchNorm / pooling / staging pass and of the saved-for-backward footprint.  Arithmetic, BatchNorm statistics,
 * weights, weight gradients and biases stay fp32; a store rounds to nearest even.  Statistics a kernel leaves behind
 * (bn_partials) are those of the ROUNDED values, i.e. of the tensor BatchNorm then reads.  Layouts, strides (in
 * elements) and argument meaning are unchanged; activation pointers need 8-byte alignment.  The product entry points
 * serve act16 = 1 under PE_PROD_BF16 only. */

/* ---- Transformer temporal head (model.py:178-193,229-241,253-255) ---------------------------
 * pe_bgemm: batched 64x64-tiled fp32 MFMA GEMM over `batch` matrices; matrix b of operand X lives
 *   at X + (b / inner) * x_outer + (b % inner) * x_inner (e.g. batch item / head inside the packed
 *   QKV projection).  mode 0: C = alpha A B^T (A [M][K], B [N][K]); 1: C = alpha A B (B [K][N]);
 *   2: C = alpha A^T B (A [K][M], B [K][N]).
 * pe_softmax_fwd: s[row][:L] = softmax(scale * s[row][:L]) in place; pe_softmax_bwd: dp <- ds.
 * pe_layernorm_fwd: z = a (+ b) (+ pe[row % period]); y = LN(z) * gamma + beta (eps inside the
 *   sqrt); z_out (optional) keeps z for the backward; D in {256, 512, 768, 1024}.
 * pe_gelu_*: exact erf GELU (activation="gelu") and its derivative. */
int pe_bgemm(int mode, const float* A, long lda, long a_outer, long a_inner, const float* B, long ldb,
             long b_outer, long b_inner, float* C, long ldc, long c_outer, long c_inner, int inner, int batch,
             int M, int N, int K, float alpha, int accumulate, void* stream);
int pe_softmax_fwd(float* s, long rows, int L, float scale, void* stream);
int pe_softmax_bwd(const float* p, float* dp, long rows, int L, float scale, void* stream);
int pe_layernorm_fwd(const float* a, const float* b, const float* pe, int period, const float* gamma,
                     const float* beta, float eps, float* z_out, float* y, float* mean, float* rstd, long rows,
                     int D, void* stream);
size_t pe_layernorm_bwd_workspace_bytes(int D);
/* pe_layernorm_bwd / pe_layernorm_bwd_fused with dgamma and dbeta both NULL: dz only (the parameter sums are not
 * reduced; the workspace is still needed). */
int pe_layernorm_bwd(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma,
                     float* dz, float* dgamma, float* dbeta, long rows, int D, void* workspace,
                     size_t workspace_bytes, void* stream);
int pe_gelu_fwd(const float* x, float* y, long n, void* stream);
int pe_gelu_bwd(const float* x, const float* dy, float* dx, long n, void* stream);
/* Dropout folded into the neighbouring pass of an encoder layer (nn.TransformerEncoderLayer, model.py:231-239:
 * x = norm1(x + dropout1(sa)); x = norm2(x + dropout2(linear2(dropout(gelu(linear1(x))))))).  Element <-> Philox
 * counter mapping, keep rule and 1/(1-p) scaling are pe_dropout_fwd's on a dense tensor, so the results equal the
 * separate passes bit for bit; mask_in replays given bytes, mask_out (optional) records them; 0 < p < 1.
 * pe_layernorm_dropout_fwd: z = a + dropout(b) (+ pe); y = LN(z).
 * pe_layernorm_bwd_fused: dy2 (optional) is added to dy first (the residual branch's gradient); dz_drop (with
 *   drop_mask, both or neither) additionally receives dropout_bwd(dz).
 * pe_gelu_dropout_fwd: y = dropout(gelu(x)); pe_gelu_dropout_bwd: dx = dropout_bwd(dy) * gelu'(x). */
int pe_layernorm_dropout_fwd(const float* a, const float* b, const float* pe, int period, const float* gamma,
                             const float* beta, float eps, float* z_out, float* y, float* mean, float* rstd,
                             long rows, int D, const unsigned char* mask_in, unsigned char* mask_out, float p,
                             unsigned long long seed, unsigned long long offset, void* stream);
int pe_layernorm_bwd_fused(const float* dy, const float* dy2, const float* z, const float* mean, const float* rstd,
                           const float* gamma, float* dz, const unsigned char* drop_mask, float p, float* dz_drop,
                           float* dgamma, float* dbeta, long rows, int D, void* workspace, size_t workspace_bytes,
                           void* stream);
int pe_gelu_dropout_fwd(const float* x, float* y, long n, const unsigned char* mask_in, unsigned char* mask_out,
                        float p, unsigned long long seed, unsigned long long offset, void* stream);
int pe_gelu_dropout_bwd(const float* x, const float* dy, const unsigned char* mask, float p, float* dx, long n,
                        void* stream);

/* ---- resampler (meldataset.py:621-627 -> torchaudio.functional.resample defaults) ----
 * sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99; y has ceil(new * n_in / orig) samples. */
typedef struct pe_resample_plan pe_resample_plan;
int pe_resample_plan_create(pe_resample_plan** plan, int orig_freq, int new_freq, int lowpass_filter_width,
                            float rolloff);
int pe_resample_plan_destroy(pe_resample_plan* plan);
long pe_resample_out_len(const pe_resample_plan* plan, long n_in);
int pe_resample_forward(const pe_resample_plan* plan, const float* x, int batch, int n_in, long x_stride, float* y,
                        long y_stride, int n_out, void* stream);
/* The transpose of pe_resample_forward: dx (batch rows of n_in, every element written) from dy (batch rows of n_out
 * <= pe_resample_out_len(n_in); dy past n_out is not read).  One thread per input sample gathers its terms with one
 * fmaf chain in ascending output index over the plan's own taps, so a row's result depends on the row alone.
 * PE_E_ARG as for the forward; PE_E_UNSUPPORTED: batch > 65535, or a ratio whose tile of dy passes 64 KB of LDS. */
int pe_resample_backward(const pe_resample_plan* plan, const float* dy, int batch, int n_out, long dy_stride,
                         float* dx, long dx_stride, int n_in, void* stream);

/* Multi-rate ragged resampler: one plan for a list of up to 16 source rates (a rate equal to new_freq copies;
 * a plan of copies only allocates nothing on the device) and one target; same taps as pe_resample_plan_create.  pe_resample_ragged_forward resamples `batch` rows in one launch:
 * row r reads n_in[r] samples at x + x_off[r] at source rate orig_freqs[rate_idx[r]] (device arrays) and writes
 * its pe_resample_ragged_out_len outputs at y + r * y_stride, then zeros up to y_width.  Each row is bit-identical
 * to pe_resample_forward on that row alone.  host_n_in / host_rate_idx are host copies of n_in / rate_idx, checked
 * before any device call (PE_E_ARG: null pointer, rate index out of range, y_stride < y_width, a row longer than
 * y_width).  Asynchronous on `stream`; no allocation. */
typedef struct pe_resample_ragged_plan pe_resample_ragged_plan;
int pe_resample_ragged_plan_create(pe_resample_ragged_plan** plan, const int* orig_freqs, int n_rates, int new_freq,
                                   int lowpass_filter_width, float rolloff);
int pe_resample_ragged_plan_destroy(pe_resample_ragged_plan* plan);
long pe_resample_ragged_out_len(const pe_resample_ragged_plan* plan, int rate_index, long n_in);
int pe_resample_ragged_forward(const pe_resample_ragged_plan* plan, const float* x, const long* x_off, const int* n_in,
                               const int* rate_idx, const int* host_n_in, const int* host_rate_idx, int batch,
                               float* y, long y_stride, int y_width, void* stream);
/* The transpose of pe_resample_ragged_forward in one launch: row r reads its pe_resample_ragged_out_len values at
 * dy + r * dy_stride (nothing past them) and writes n_in[r] gradients at dx + x_off[r], the layout the forward read.
 * dx_width > 0: padded rows, each also zeroed from n_in[r] to dx_width; dx_width == 0: packed rows, nothing else is
 * written.  A row at the target rate is a copy of dy.  Each row is bit-identical to pe_resample_backward on that row
 * alone.  PE_E_ARG: null pointer, rate index out of range, a row's output longer than dy_stride, a row longer than
 * dx_width; PE_E_UNSUPPORTED as for pe_resample_backward.  Asynchronous on `stream`; no allocation. */
int pe_resample_ragged_backward(const pe_resample_ragged_plan* plan, const float* dy, long dy_stride,
                                const long* x_off, const int* n_in, const int* rate_idx, const int* host_n_in,
                                const int* host_rate_idx, int batch, float* dx, int dx_width, void* stream);

/* ---- pitch-shift augmentation (reference meldataset.py:324-517 -> librosa.effects.pitch_shift defaults) ----
 * STFT 2048 / hop 512 / periodic Hann / centre zero padding -> phase vocoder at rate 2^(-n_steps/12) -> iSTFT to
 * round(N / rate) samples -> resampy sinc resampling (res_type 0 = kaiser_best, 1 = kaiser_fast) back to N samples.
 * pe_pitch_shift_plan (host only, no device call) lays out a ragged batch of n_rows rows: row r reads n[r] samples at
 * x + x_off[r], shifts them by n_steps[r] (|n_steps| <= 24) and writes output samples [j_lo[r], j_lo[r] + j_cnt[r])
 * (<= n[r]) to out + out_row[r] * out_stride (out_stride >= j_cnt[r]).  It fills meta (n_rows x
 * pe_pitch_shift_plan_fields() int64), ratios (n_rows x {rate, resample ratio}) and totals {STFT frames, stretched
 * columns, stretched samples, output samples}, the sizes of the workspaces the four stages below read and write:
 * spec (frames x 1025 complex), cols (columns x 1025 complex), frames (columns x 2048), stretched (samples), out.
 * Only the prefix of a row that the output window depends on is computed.  n_fft / hop other than 2048 / 512 are
 * PE_E_UNSUPPORTED.  table: the resampling filter followed by its first differences (2 x (zeros * 512 + 1) floats).
 * pe_pitch_shift_resample: out = resampled * gains[r] (+ noise, laid out like the output windows, optional). */
int pe_pitch_shift_plan(int n_rows, const long* n, const float* n_steps, const long* x_off, const long* j_lo,
                        const long* j_cnt, const long* out_row, long out_stride, int sr, int n_fft, int hop,
                        int res_type, long* meta, double* ratios, long* totals);
int pe_pitch_shift_plan_fields(void);
int pe_pitch_shift_stft(const float* x, const long* meta, int n_rows, long n_frames, float* spec, void* stream);
int pe_pitch_shift_vocoder(const float* spec, const long* meta, const double* ratios, int n_rows, long n_cols,
                           float* cols, void* stream);
int pe_pitch_shift_istft(const float* cols, const long* meta, int n_rows, long n_cols, long n_samples, float* frames,
                         float* stretched, void* stream);
int pe_pitch_shift_resample(const float* stretched, const long* meta, const double* ratios, const float* table,
                            int res_type, const float* gains, const float* noise, int n_rows, long n_out, float* out,
                            void* stream);

/* ---- WORLD vocoder synthesis (reference Utils/synthetic.py:194-220 -> pyworld.synthesize, WORLD's Synthesis) ----
 * One minimum-phase impulse response of fft_size samples per glottal pulse, overlap-added; fft_size 512 / 1024 / 2048
 * (another power of two is PE_E_UNSUPPORTED, anything else PE_E_ARG).  The pulse positions are a sequential float64
 * recurrence and come from the host (pitchextractor_amd/world.py: time_base), or from pe_world_time_base below.
 * pe_world_plan (host only, no device call) lays out a ragged batch: row r has n_frames[r] frames (f0, nullable: the
 * rows' curves back to back, checked to be finite) and pulse_cnt[r] pulses, the rows' tables back to back in index
 * (sample, strictly increasing, inside the row's int(n_frames * frame_period_ms * fs / 1000) samples, consecutive
 * pulses at most fft_size apart), shift (seconds, 0 <= shift * fs <= 1) and voiced.  Frame f of the row's spectral
 * envelope is the fft_size / 2 + 1 floats at sp + sp_off[r] + f * sp_stride[r]; a stride of 0 broadcasts one template to
 * every frame.  ap likewise (ap_off NULL or ap_off[r] < 0: all zeros).  The aperiodic noise of the row is the standard
 * normals at noise + noise_off[r], one per sample of the row (noise_off NULL or < 0: drawn in the kernel, Philox4x32-10
 * keyed by (seeds[r], sample) and Box-Muller).  Output samples [j_lo[r], j_lo[r] + j_cnt[r]) go to
 * out + out_row[r] * out_stride (out_stride >= j_cnt[r]).  Only pulses whose response meets the window are planned.
 * The plan fills meta (n_rows x pe_world_plan_fields() int64), pulses (planned pulses x 6 int64: sample, the two
 * frames, noise samples, voiced, row), pulse_f (planned pulses x {frame fraction, shift * fs}; size both for the
 * batch's pulse count) and totals {planned pulses, output samples}.
 * pe_world_responses: responses (planned pulses x fft_size floats), one workgroup per pulse; table: exp(-2 pi i m /
 * fft_size) for m < fft_size (re, im), then the fft_size floats of WORLD's DC remover.
 * pe_world_overlap_add: out = gains[r] * sum of the responses covering the sample, in ascending pulse order (no
 * atomics: a row is bit-identical alone and in any batch) + out_noise (optional, laid out like the output windows). */
int pe_world_plan_fields(void);
int pe_world_plan(int n_rows, const long* n_frames, const double* f0, const long* pulse_cnt, const long* index,
                  const double* shift, const unsigned char* voiced, const long* sp_off, const long* sp_stride,
                  const long* ap_off, const long* ap_stride, const long* noise_off, const long* seeds,
                  const long* j_lo, const long* j_cnt, const long* out_row, long out_stride, double fs,
                  double frame_period_ms, int fft_size, long* meta, long* pulses, double* pulse_f, long* totals);
int pe_world_responses(const float* sp, const float* ap, const float* noise, const long* meta, const long* pulses,
                       const double* pulse_f, const float* table, int n_rows, long n_pulses, int fft_size,
                       float* responses, void* stream);
int pe_world_overlap_add(const float* responses, const long* meta, const long* pulses, const float* gains,
                         const float* out_noise, int n_rows, long n_out, int fft_size, float* out, void* stream);

/* ---- WORLD time base on the device: pulse positions from an exact integer phase (csrc/world_time_base.hip) ---------
 * GetTimeBase + GetPulseLocationsForTimeBase for a ragged batch, opt-in beside the host's float64 recurrence.  Row r
 * has L = n_frames[r] >= 2 frames and n = int(L * frame_period_ms * fs / 1000) samples; cf_ext / cv_ext hold the rows'
 * extended coarse curves back to back, L + 1 doubles per row each (F0 with the frames below the synthesizer's floor at
 * 0 and voicing as 0 / 1, each with one extrapolated frame 2 a[L-1] - a[L-2], the F0's clamped at 0 from below), built
 * by the caller on the host.  With fp = frame_period_ms / 1000, t = i / fs and j the frame with j fp <= t < (j + 1) fp
 * (from floor(t / fp), corrected by comparisons, within [0, L - 1]): interp(c) = ((c[j+1] - c[j]) / ((j + 1) fp - j fp))
 * * (t - j fp) + c[j]; vuv_i = interp(cv) > 0.5; f0i = vuv_i ? interp(cf) : 500; inc_i = rint(f0i / fs * 2^64) as an
 * unsigned 64-bit integer; T_i = the exact 128-bit sum of inc_0 .. inc_i with hi_i its high and lo_i its low word.
 * Sample i <= n - 2 carries pulse number hi_i iff hi_(i+1) == hi_i + 1, with shift = (double(2^64 - lo_i) /
 * double(inc_(i+1))) / fs seconds and voiced = vuv_i; the row has hi_(n-1) pulses.  All of it is IEEE double without
 * contraction and integer addition, so a row's tables are the same bits alone, in any batch and for any piece size.
 * pe_world_time_base_plan (host only, no device call) fills meta (n_rows x pe_world_time_base_plan_fields() int64:
 * sample prefix, n, L, curve offset, pieces of 4096 samples counted from the row's own start, piece prefix, first pulse
 * slot, slot capacity = floor(n * max(cf_ext, 500) / fs) + 1) and totals {pieces, pulse slots, samples}.  PE_E_ARG: a
 * null pointer, n_rows outside 0 .. 65535, L < 2, a non-finite or negative curve value, a value of cf_ext, or 500, at
 * or above fs / 2, a non-finite or non-positive fs or frame_period_ms, a row of 2^31 - 8 samples or more.
 * pe_world_time_base chains three launches on the stream, none of which waits on another workgroup and none of which
 * uses an atomic: piece sums (one workgroup per (row, piece)), the exclusive scan of each row's piece sums and
 * counts[r] = hi_(n-1) (one workgroup per row), the pulses (one workgroup per (row, piece); every slot has exactly one
 * writer).  stages: bit 0 / 1 / 2 selects the launches (7: all; a later stage alone reads what an earlier call left
 * in the workspace).  host_meta: the host copy of meta (PE_E_ARG unless it is the plan's for fs and frame_period_ms).
 * index / shift / vuv: totals[1] slots, row r's pulses from its first slot on, the slots beyond counts[r] untouched.
 * status: one int the caller zeroes; set to 1 if a pulse fell at or beyond its row's capacity (it was not written;
 * impossible with the plan's own meta).  f0i / lo / hi (each nullable, totals[2] values): per-sample f0i, lo_i and hi_i,
 * for tests.  workspace: pe_world_time_base_workspace_bytes(totals[0]) bytes, else PE_E_WORKSPACE. */
int pe_world_time_base_plan_fields(void);
int pe_world_time_base_plan(int n_rows, const long* n_frames, const double* cf_ext, const double* cv_ext, double fs,
                            double frame_period_ms, long* meta, long* totals);
size_t pe_world_time_base_workspace_bytes(long pieces);
int pe_world_time_base(const double* cf_ext, const double* cv_ext, const long* meta, const long* host_meta,
                       int n_rows, double fs, double frame_period_ms, int stages, long* index, double* shift,
                       unsigned char* vuv, long* counts, int* status, double* f0i, unsigned long* lo, long* hi,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- WORLD CheapTrick: the spectral envelope of a recording (pyworld.cheaptrick, WORLD's cheaptrick.cpp) ----------
 * One frame per F0 value, frame f at f * frame_period_ms with f0 = F0[f] (500 Hz where F0[f] <= 3 fs / (fft_size - 3),
 * or is not a number): F0-adaptive window, power spectrum, DC correction, linear smoothing of width 2 f0 / 3, + 2^-52,
 * smoothing with recovery (lifter parameter q1).  float32 per frame; the two randn safeguards are dropped; the linear
 * smoothing sums the covered bins and the two partial edge bins.  F0 belongs below fs / 2 (it is clamped there).
 * fft_size 512 / 1024 / 2048, and 3 fs / (fft_size - 3) <= f0_floor: otherwise PE_E_UNSUPPORTED; PE_E_ARG for a
 * non-positive or non-finite fs, frame_period_ms or f0_floor, a null pointer, n_rows outside 0 .. 65535.
 * pe_cheaptrick_plan (host only, no device call) lays out a ragged batch: row r is the x_len[r] >= 0 samples at
 * x + x_off[r] (at least one where frames are asked for), its F0 the f0_len[r] floats at f0 + f0_off[r]; frames
 * [first_frame[r], first_frame[r] + n_frames[r]) of it (within f0_len[r]) are analysed, frame first_frame[r] + q going
 * to the fft_size / 2 + 1 floats at sp + out_off[r] + q * out_stride[r] (out_stride[r] >= fft_size / 2 + 1).  It fills
 * meta (n_rows x pe_cheaptrick_plan_fields() int64) and totals {frames}.
 * pe_cheaptrick: one launch, one workgroup per (row, frame); host_meta: the host copy of meta (PE_E_ARG unless it is
 * the plan's); table: exp(-2 pi i m / fft_size) for m < fft_size (re, im), what pe_world_responses' table opens with.
 * A row's frames are bit-identical alone, at any offset, padded, anywhere in a batch and in any frame sub-range. */
int pe_cheaptrick_plan_fields(void);
int pe_cheaptrick_plan(int n_rows, const long* x_off, const long* x_len, const long* f0_off, const long* f0_len,
                       const long* first_frame, const long* n_frames, const long* out_off, const long* out_stride,
                       double fs, double frame_period_ms, double f0_floor, int fft_size, long* meta, long* totals);
int pe_cheaptrick(const float* x, const float* f0, const long* meta, const long* host_meta, const float* table,
                  int n_rows, double fs, double frame_period_ms, double q1, double f0_floor, int fft_size, float* sp,
                  void* stream);

/* ---- WORLD D4C: the band aperiodicity of a recording (pyworld.d4c, WORLD's d4c.cpp) --------------------------------
 * One frame per F0 value, frame f at f * frame_period_ms.  LoveTrain (Blackman window of 3 periods of max(F0, 40),
 * N_l = 2^(1 + floor(log2(3 fs / 40 + 1))) points): a0 = power in [100, 4000] Hz / power in [100, 7900] Hz, 0 where
 * F0[f] <= 0 or is not a number, or the denominator is 0.  F0[f] <= 0 or a0 <= threshold is the unvoiced verdict; so is
 * a smoothed power spectrum that is not positive in every bin.  Otherwise, with f0 = max(47, F0[f]) and N_d = 2^(1 +
 * floor(log2(4 fs / 47 + 1))) points: static centroid, smoothed power, static group delay, and per 3 kHz band i <
 * bands = int(min(15000, fs / 2 - 3000) / 3000) the coarse aperiodicity in dB, min(0, . + (F0[f] - 100) / 50).
 * float32 per frame; the window's randn is dropped; the linear smoothing is CheapTrick's interval mean.  F0 belongs
 * below fs / 2 (it is clamped there).  PE_E_UNSUPPORTED: fs / 2 <= 7900, N_d or N_l above 4096, bands above 5,
 * fft_size not 512 / 1024 / 2048; PE_E_ARG: a non-positive or non-finite fs or frame_period_ms, a non-finite
 * threshold, a null pointer, n_rows outside 0 .. 65535.
 * pe_d4c_plan (host only, no device call): pe_cheaptrick_plan's arguments and layout (frame first_frame[r] + q of row
 * r goes to the fft_size / 2 + 1 floats at ap + out_off[r] + q * out_stride[r]); fills meta (n_rows x
 * pe_d4c_plan_fields() int64) and totals {frames, N_d, N_l, bands, L} (L: points of the Nuttall window).  The layout
 * is guaranteed to be one: both plans fill meta through the same code and the three launch entry points check it with
 * the same walk, so a meta from either plan (same rows, frames and fft_size) is accepted by pe_cheaptrick, pe_d4c_bands
 * and pe_d4c_expand alike, and pe_d4c_plan_fields() == pe_cheaptrick_plan_fields().
 * pe_d4c_bands: one launch, one workgroup per (row, frame); host_meta: the host copy of meta (PE_E_ARG unless it is the
 * plan's); table: exp(-2 pi i m / N_d) for m < N_d (re, im), then the same for N_l.  band: frames x (1 + bands)
 * floats in plan order, {a0, coarse[0 .. bands)}; coarse is NaN in a frame with the unvoiced verdict.
 * pe_d4c_expand: one launch; a frame's band values to its bins: the knots (0, -60), (3000 (i + 1), coarse[i]), (fs / 2,
 * -1e-12) in dB interpolated at k fs / fft_size, ap = 10^(dB / 20); 1 - 1e-12 in every bin of an unvoiced frame.
 * A row's frames are bit-identical alone, at any offset, padded, anywhere in a batch and in any frame sub-range. */
int pe_d4c_plan_fields(void);
int pe_d4c_plan(int n_rows, const long* x_off, const long* x_len, const long* f0_off, const long* f0_len,
                const long* first_frame, const long* n_frames, const long* out_off, const long* out_stride, double fs,
                double frame_period_ms, int fft_size, long* meta, long* totals);
int pe_d4c_bands(const float* x, const float* f0, const long* meta, const long* host_meta, const float* table,
                 int n_rows, double fs, double frame_period_ms, double threshold, int fft_size, float* band,
                 void* stream);
int pe_d4c_expand(const float* band, const long* meta, const long* host_meta, int n_rows, double fs, int fft_size,
                  float* ap, void* stream);

/* ---- Voice transforms of WORLD frames: formant warp, tempo, tilt, breath (csrc/world_warp.hip) -----------------------
 * Row r has src_frames[r] source frames of fft_size / 2 + 1 floats, frame f at sp_in + in_off[r] + f * in_stride[r]
 * (in_stride >= 0; 0: one frame for every f) and, where ap_off is given and ap_off[r] >= 0, at ap_in + ap_off[r] +
 * f * ap_stride[r].  Its out_frames[r] output frames go to sp_out (and ap_out, for a row with an ap) + out_off[r] +
 * q * out_stride[r], out_stride[r] >= fft_size / 2 + 1.  Output frame q of the batch (rows back to back) reads the
 * source position pos_frame[q] + pos_frac[q], 0 <= pos_frac < 1 (formed in float64 by the caller; pe_f0_dio_events'
 * convention), within [0, src_frames[r] - 1].  params: n_rows x {alpha, f_hi, tilt_db_per_octave, breath_db} floats.
 * Output bin k at f = k fs / fft_size: the frequency map w(f) = alpha f for f <= f_hi min(alpha, 1) / alpha and the
 * straight line from there to (fs / 2, fs / 2) (Jaitly & Hinton 2013); sp_out(f) = exp of the bilinear interpolation
 * of ln sp_in over the two source frames and the two source bins around w^-1(f), plus tilt_db_per_octave *
 * log2(max(f, 125) / 1000) dB (sp is a power: 10 log10); ap_out(f) = the same read of ap_in, linear, times
 * 10^(breath_db / 20), clamped to [0, 1].  sp_in must be positive.  With alpha == 1, no tilt and pos_frac == 0 the
 * frame's sp is copied bit for bit, and its ap when breath_db == 0 as well.  float32; the buffers must not overlap.
 * pe_world_warp_plan (host only, no device call): fills meta (n_rows x pe_world_warp_plan_fields() int64: the frame
 * plan's fields, then in_stride, ap_off or -1, ap_stride) and totals {output frames}.  PE_E_ARG: a null pointer
 * (ap_off may be null: no row has an ap; pos_frame / pos_frac may be null when there is no output frame), n_rows
 * outside 0 .. 65535, a non-finite or non-positive fs, a negative count, offset or stride, an output stride below
 * fft_size / 2 + 1, output frames of a row without source frames, alpha outside [0.5, 2] or any non-finite parameter,
 * f_hi outside (0, fs / 2) (the map would not rise strictly on [0, fs / 2]), a position outside [0, src_frames[r] - 1]
 * or a fraction outside [0, 1).  PE_E_UNSUPPORTED: fft_size not 512 / 1024 / 2048.
 * pe_world_warp: one launch, one workgroup per (row, output frame); host_meta: the host copy of meta (PE_E_ARG unless
 * it is the plan's); meta, pos_frame, pos_frac, params: device copies of what the plan took.  ap_in / ap_out may be
 * null when no row has an ap.  No rows or no output frames: PE_OK without a launch.  A row's frames are bit-identical
 * alone, at any offset, padded, anywhere in a batch and into a wider stride. */
int pe_world_warp_plan_fields(void);
int pe_world_warp_plan(int n_rows, const long* src_frames, const long* in_off, const long* in_stride,
                       const long* ap_off, const long* ap_stride, const long* out_frames, const long* out_off,
                       const long* out_stride, const int* pos_frame, const float* pos_frac, const float* params,
                       double fs, int fft_size, long* meta, long* totals);
int pe_world_warp(const float* sp_in, const float* ap_in, const long* meta, const long* host_meta,
                  const int* pos_frame, const float* pos_frac, const float* params, int n_rows, double fs,
                  int fft_size, float* sp_out, float* ap_out, void* stream);

/* ---- F0 bin decoding (build-defined; the inverse of pe_f0_bins_ce_loss) and pitch metrics --------------------
 * logits: N sequences of T frames of C bins, frame (n, t) at logits + n * ld_n + t * ld_t (2 <= C <= 1024, more is
 * PE_E_UNSUPPORTED).  Bin b stands for cents(b) = 20 b + 1997.3794084376191, f(b) = 10 * 2^(cents(b) / 1200) Hz.
 * lengths (nullable, N int32 on the device, 1 <= lengths[n] <= T): frames at t >= lengths[n] are ignored and their
 * outputs are 0.  Outputs are dense (N, T).
 *
 * pe_f0_decode_frames: per frame, the bin (bins_in[n * T + t] when bins_in is given, else the arg max of the row, the
 * LOWEST index on ties), its frequency and confidence = softmax(row)[bin].  PE_F0_ARGMAX: f0 = f(bin);
 * PE_F0_WEIGHTED: f0 = 10 * 2^(cents / 1200) with cents the average of cents(c) over c in [bin - 4, bin + 4] (cut at
 * the row ends) under the weights exp(l_c - l_bin).  bins_out may be NULL when bins_in is given; the two must not overlap.
 *
 * pe_f0_viterbi: bins_out[n][0 .. L) = the path maximising l_0[b_0] + sum_t (log A(b_{t-1}, b_t) + l_t[b_t]) with
 * A(i, j) = max(12 - |i - j|, 0) / sum_j' max(12 - |i - j'|, 0), ties to the lowest index.  One workgroup per
 * sequence; back-pointers stay in LDS when T * C bytes fit beside the two delta rows, else they go to `workspace`
 * (pe_f0_viterbi_workspace_bytes, 0 when none is needed; PE_E_WORKSPACE when it is needed and too small).
 *
 * pe_pitch_metrics (reference Utils/dynamic_pitch_tools.py:79-104): over n frames, voiced = f0_ref > 0, cents re
 * 55 Hz in double.  out6 (device doubles) = {rms cents error over voiced frames with the prediction clipped below
 * at 1e-5 (rms_cents_error), share of voiced frames with a positive prediction within threshold_cents, the same on
 * the circular (octave-forgiving) distance, share of frames whose voicing differs, voiced frames, frames}; the
 * first three are NaN when no frame is voiced.  One workgroup. */
#define PE_F0_ARGMAX 0
#define PE_F0_WEIGHTED 1
int pe_f0_decode_frames(const float* logits, long ld_t, long ld_n, int C, const int* lengths, const int* bins_in,
                        int N, int T, int method, int* bins_out, float* f0_out, float* conf_out, void* stream);
size_t pe_f0_viterbi_workspace_bytes(int N, int T, int C);
int pe_f0_viterbi(const float* logits, long ld_t, long ld_n, int C, const int* lengths, int N, int T, int* bins_out,
                  void* workspace, size_t workspace_bytes, void* stream);
int pe_pitch_metrics(const float* f0_pred, const float* f0_ref, long n, double threshold_cents, double* out6,
                     void* stream);

/* ---- Row statistics of a ragged batch, for any row plan ---------------------------------------------------------
 * Every row plan of the F0 trackers (pe_f0_track_plan, pe_f0_dio_plan) is n_rows x K int64 and opens with the same
 * header: field 0 = the row's offset in x, field 1 = its length in samples.  pe_row_stats reads only that header, at
 * the caller's stride meta_fields = K (PE_E_ARG below 2): stats[r] = {mean, max |x - mean|}, each row reduced in 64
 * pieces in a fixed order through `workspace` (pe_row_stats_workspace_bytes; PE_E_WORKSPACE when too small), so a
 * row's statistics depend on neither the batch around it nor the plan that describes it. */
size_t pe_row_stats_workspace_bytes(int n_rows);
int pe_row_stats(const float* x, const long* meta, int meta_fields, int n_rows, float* stats, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- F0 tracking: Boersma's autocorrelation method (Praat "Sound: To Pitch (ac)"), ragged batches --------------
 * config7 = {min_pitch, max_pitch, silence_threshold, voicing_threshold, octave_cost, octave_jump_cost,
 * voiced_unvoiced_cost} (doubles).  PE_E_ARG: null pointer, sr <= 0, hop <= 0, a non-finite value, min_pitch <= 0,
 * min_pitch >= min(max_pitch, sr / 2), a non-positive threshold, a negative cost.  PE_E_UNSUPPORTED: an FFT length
 * (the power of two >= 1.5 x window samples) outside 1024 .. 8192.  Every check runs before any device call.
 *
 * pe_f0_track_plan (host only, no device call): row r has n[r] samples at x + x_off[r].  consts8 = {window samples,
 * period samples, FFT length, lag bound (exclusive), half window, half period, table floats, frames whose
 * back-pointers stay in LDS}; dconsts2 = {ceiling = min(max_pitch, sr / 2), time step}; meta (n_rows x
 * pe_f0_track_plan_fields() int64, to be copied to the device) holds each row's sample offset / length, frame count
 * floor((n / sr - 3 / min_pitch) / time_step) + 1 (0 when the row is shorter than one window), frame prefix offset
 * and back-pointer spill offset (-1: LDS); t1[r] = centre time of the row's first frame; totals2 = {frames of the
 * batch, workspace bytes of pe_f0_track_path}.  Frame counts and times are float64 expressions evaluated in one
 * fixed order (tests/f0_track_ref.py states them).
 *
 * tables (device, consts8[6] floats): exp(-2 pi i m / C), m < C = FFT length / 2; exp(-2 pi i k / (2 C)), k <= C;
 * the Hann window 0.5 - 0.5 cos(2 pi (j + 1) / (window + 1)); its normalised autocorrelation for lags 0 .. half
 * window.  stats: pe_row_stats' output for this plan.  pe_f0_track_frames: per frame g (rows back to
 * back) up to 15 candidates, cand_f / cand_s [g][15] (Hz, strength; [0] is the unvoiced candidate, voiced ones in
 * lag order) and their count cand_n[g].  pe_f0_track_path: f0[g] = frequency of the best path's candidate, 0 where
 * it is unvoiced (frequency 0 or >= ceiling); rows with more than consts8[7] frames keep 16 bytes of back-pointers
 * per frame in `workspace` (PE_E_WORKSPACE when too small).  host_meta: the host copy of meta. */
int pe_f0_track_plan_fields(void);
int pe_f0_track_plan(int n_rows, const long* n, const long* x_off, int sr, int hop, const double* config7,
                     long* consts8, double* dconsts2, long* meta, double* t1, long* totals2);
int pe_f0_track_frames(const float* x, const long* meta, const long* host_meta, const double* t1,
                       const float* stats, const float* tables, long n_table, int n_rows, int sr, int hop,
                       const double* config7, float* cand_f, float* cand_s, int* cand_n, void* stream);
int pe_f0_track_path(const float* cand_f, const float* cand_s, const int* cand_n, const long* meta,
                     const long* host_meta, int n_rows, int sr, int hop, const double* config7, float* f0,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- F0 tracking: WORLD DIO + StoneMask (pyworld's defaults, no decimation), ragged batches ---------------------
 * config4 = {f0_floor, f0_ceil, channels_in_octave, allowed_range} (doubles).  PE_E_ARG: null pointer, sr <= 0,
 * hop <= 0, a non-finite value, f0_floor <= 0, f0_floor >= f0_ceil, channels_in_octave <= 0, allowed_range <= 0, a
 * host_meta that is not the plan's.  PE_E_UNSUPPORTED: sr outside 8000 .. 48000, f0_ceil >= sr / 2, hop > sr, more
 * than 16 bands, a combined filter (2 round(sr / 50) + 4 half_average_length[0] taps) that needs a block transform
 * above 8192 points, an f0_floor whose StoneMask transform exceeds 4096 points.  Every check runs before any device
 * call.  The restatement tests/dio_ref.py states every convention.
 *
 * pe_f0_dio_plan (host only): consts10 = {bands, block transform N, taps of the longest combined filter, block step
 * N - taps + 1, samples read ahead of a block, voice_range_minimum, table floats, samples per event chunk,
 * round(sr / 50), StoneMask root-table floats}; half16[b] = half_average_length; dconsts17 = {frame_period ms,
 * boundary[b]}; meta (n_rows x pe_f0_dio_plan_fields() int64, to be copied to the device) = per row {sample offset,
 * samples, frames = (int)(1000 n / sr / frame_period) + 1, frame prefix, sample prefix, blocks, block prefix, event
 * slot prefix (n / 2 + 1 slots per row, band and kind), event chunks, chunk prefix}; totals6 = {frames, samples,
 * blocks, event slots, chunks, workspace bytes of pe_f0_dio_events}.
 *
 * tables (device, consts10[6] floats): exp(-2 pi i m / C), m < C = N / 2; exp(-2 pi i k / N), k <= C; per band the
 * spectrum (C + 1 complex bins, divided by C) of the low-cut filter convolved with the band's Nuttall low-pass, delayed
 * to the longest band's delay.  stats: pe_row_stats' output for this plan (the row mean).
 * pe_f0_dio_bands: band_signals[b][sample prefix + i], bands x totals6[1] floats.
 * pe_f0_dio_events: per (row, band, kind; kind 0 .. 3 = signal, negation, first difference, negated difference) the
 * fine edges in order as e_idx (integer part, i + 1) and e_frac (fraction in (0, 1]) at slot
 * (event slot prefix x bands x 4) + (band x 4 + kind) x (n / 2 + 1); e_count[row][band][kind] edges.
 * pe_f0_dio_candidates: cand / score [band][frame] (0 / 100000 = rejected), best[frame] and best_band[frame] of the
 * lowest score (first band on a tie).  pe_f0_dio_fix: steps4[s][frame] = the contour after FixF0Contour's step
 * s + 1; all zero for a row of at most voice_range_minimum frames.  pe_f0_stonemask: f0_out[frame] refined from
 * f0_in (0 stays 0; roots = the 128, 256, .. 4096-th roots of unity back to back, consts10[9] floats); every
 * f0_in > 0 must be >= f0_min, which bounds the transform (a smaller one yields 0). */
int pe_f0_dio_plan_fields(void);
int pe_f0_dio_plan(int n_rows, const long* n, const long* x_off, int sr, int hop, const double* config4,
                   long* consts10, long* half16, double* dconsts17, long* meta, long* totals6);
int pe_f0_dio_bands(const float* x, const long* meta, const long* host_meta, const float* stats,
                    const float* tables, long n_table, int n_rows, int sr, int hop, const double* config4,
                    float* band_signals, void* stream);
int pe_f0_dio_events(const float* band_signals, const long* meta, const long* host_meta, int n_rows, int sr,
                     int hop, const double* config4, int* e_idx, float* e_frac, int* e_count,
                     void* workspace, size_t workspace_bytes, void* stream);
int pe_f0_dio_candidates(const int* e_idx, const float* e_frac, const int* e_count, const long* meta,
                         const long* host_meta, int n_rows, int sr, int hop, const double* config4,
                         float* cand, float* score, float* best, int* best_band, void* stream);
int pe_f0_dio_fix(const float* best, const float* cand, const long* meta, const long* host_meta, int n_rows,
                  int sr, int hop, const double* config4, float* steps4, void* stream);
int pe_f0_stonemask(const float* x, const long* meta, const long* host_meta, const float* f0_in,
                    const float* roots, long n_roots, int n_rows, int sr, int hop, double f0_min,
                    float* f0_out, void* stream);

/* ---- Robustness stress conditions (reference Utils/room_and_microphone_stress.ipynb, amplitude_pathologies.ipynb)
 * and the notebooks' melody metrics, ragged batches ------------------------------------------------------------------
 * pe_stress_plan (host only): row r has n[r] samples at x + x_off[r] and is written to y + y_off[r].  consts4 =
 * {block step S = 2048, table floats, samples per biquad / AGC piece, samples per histogram chunk}; meta (n_rows x
 * pe_stress_plan_fields() int64, to be copied to the device) = per row {sample offset, samples, output offset, sample
 * prefix, blocks = ceil(n / S), block prefix}; totals2 = {samples, blocks}.  Every entry point below checks its
 * arguments and host_meta (the host copy of meta) before any device call: PE_E_ARG for a null pointer, a plan that is
 * not pe_stress_plan's or a value out of range, PE_E_WORKSPACE for a workspace that is missing or too small.  Rows of
 * length 0 are valid.  A row's output depends on the row alone, not on the batch or the layout around it.
 *
 * tables (device, consts4[1] floats): exp(-2 pi i m / C), m < C = 2048; exp(-2 pi i k / 2C), k <= C.
 * pe_stress_spectra: spectra (blocks x C complex) of every block of every row, one launch.  partition = 0: block b is
 * the real 2S-point transform of samples [(b - 1) S, (b + 1) S), zero outside the row; partition = 1: of samples
 * [b S, (b + 1) S) followed by S zeros, divided by C (a filter's partitions).  Bin 0 holds {X[0], X[C]}.
 * pe_stress_rir: y[n] = sum_k h[k] x[n - k] for n < len(x), h = RIR rir_index[r] of a set of n_rirs ragged RIRs (each
 * of length >= 1) given by their plan (rir_meta on the device, host_rir_meta) and their partition spectra
 * (pe_stress_spectra, partition = 1); then with p = max |y| of the row, y /= p + 1e-6 if p > 0.99 (float32).  Uniformly
 * partitioned overlap-save, three launches.  workspace: pe_stress_rir_workspace_bytes(totals2[1]).  PE_E_ARG also for an
 * index outside the set.
 * pe_stress_biquad: a cascade of n_stages <= 8 biquads, coeffs (host) = per stage {b0, b1, b2, a1, a2} with a0 = 1:
 * v[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 v[n-1] - a2 v[n-2] in double, the stage's output float32(v) clamped to
 * [-1, 1] (the clamp is never fed back).  PE_E_UNSUPPORTED for a stage with a pole on or outside the unit circle.
 * pe_stress_clip: copy != 0: y = x.  Else thr (thresholds[r], nullable) = numpy's linear quantile of |x| at q, in the
 * float32 arithmetic numpy 2 uses for a float32 array and a Python float q; y = clip(x, -thr, thr), or x if thr <= 0.
 * pe_stress_agc: params4 = {attack coefficient, release coefficient, target_rms, max_gain (< 256)}: the envelope
 * follower in double, gain = float32(clip(target_rms / (env + 1e-6), 1 / max_gain, max_gain)), for smoothing > 1
 * np.convolve(gain, ones / smoothing, "same") with exact window sums rounded once to float32, y = clip(float32(x gain),
 * -1, 1).  PE_E_ARG also for a row shorter than smoothing > 1.  workspace: pe_stress_agc_workspace_bytes(totals2[0]).
 *
 * pe_melody_metrics (the notebooks' compute_metrics, in double): tracks (n_rows x pe_melody_metrics_fields() int64;
 * host_tracks its host copy) = per row {offset in f0_pred, frames n, offset in f0_ref, offset in f0_base, frames
 * compared with the baseline}.  out7[r] = {RPA, RCA, VUV accuracy, OctaveError, VUV_flips, voiced frames, frames}:
 * voiced = f0_ref > 0, predicted voiced = f0_pred > voicing_threshold_hz, cents re 55 Hz with the prediction clipped
 * below at 1e-5, a hit within 50 cents (RCA: on the circular distance), an octave error = a miss within 50 cents of a
 * non-zero multiple of 1200 (round half even).  RPA, RCA and OctaveError are NaN when no frame is voiced; VUV_flips =
 * share of frames whose voicing differs from f0_base's, NaN without a baseline (f0_base NULL) or frames to compare. */
int pe_stress_plan_fields(void);
int pe_stress_plan(int n_rows, const long* n, const long* x_off, const long* y_off, long* consts4, long* meta,
                   long* totals2);
size_t pe_stress_rir_workspace_bytes(long blocks);
int pe_stress_spectra(const float* x, const long* meta, const long* host_meta, int n_rows, int partition,
                      const float* tables, long n_table, float* spectra, void* stream);
int pe_stress_rir(const float* x, const long* meta, const long* host_meta, int n_rows, const float* rir_spectra,
                  const long* rir_meta, const long* host_rir_meta, int n_rirs, const int* rir_index,
                  const int* host_rir_index, const float* tables, long n_table, float* y, void* workspace,
                  size_t workspace_bytes, void* stream);
int pe_stress_biquad(const float* x, const long* meta, const long* host_meta, int n_rows, const double* coeffs,
                     int n_stages, float* y, void* stream);
int pe_stress_clip(const float* x, const long* meta, const long* host_meta, int n_rows, double q, int copy, float* y,
                   float* thresholds, void* stream);
int pe_stress_clip_rows(const float* x, const long* meta, const long* host_meta, int n_rows, const double* q,
                        const double* host_q, const int* copy, const int* host_copy, float* y, float* thresholds,
                        void* stream);
size_t pe_stress_agc_workspace_bytes(long samples);
int pe_stress_agc(const float* x, const long* meta, const long* host_meta, int n_rows, const double* params4,
                  int smoothing, float* y, void* workspace, size_t workspace_bytes, void* stream);
int pe_melody_metrics_fields(void);
int pe_melody_metrics(const float* f0_pred, const float* f0_ref, const float* f0_base, const long* tracks,
                      const long* host_tracks, int n_rows, double voicing_threshold_hz, double* out7, void* stream);

/* ---- Synthesized evaluation stimuli (reference Utils/dynamic_pitch_tools.py, dynamic_pitch_behavior.ipynb,
 * pitch_range_and_timbre_coverage.ipynb) and the dynamic metrics, ragged batches -------------------------------------
 * pe_stim_plan (host only): row r has n[r] >= 1 samples written at y + y_off[r]; kind[r] = 0 a given F0 curve
 * (curve_len[r] float32 values at curves + curve_off[r]; curve_len 1 is a constant tone, else n[r]), 1 a linear
 * glide, 2 a vibrato, 3 a harmonic tone.  raw6[r] = {amplitude, a, b, c, duration in seconds, snr_db}: glide a =
 * start Hz, b = end Hz; vibrato a = base Hz, b = depth in cents, c = rate Hz; tone a = frequency.  partials[r] = 16 x
 * {harmonic, amplitude} of which the first n_partials[r] (1 .. 16, tones only) are summed in order; noise_off[r] = the
 * row's offset in the noise tensor, -1 for none.  n is given by the caller (int(duration * sr)); fade =
 * (long)max(0.02 * sr, 0).  consts4 = {piece S = 2048, fade, 16, doubles per row of `stats`}; meta (n_rows x
 * pe_stim_plan_fields() int64, to be copied to the device) = per row {offset, samples, kind, sample prefix, pieces =
 * ceil(n / S), piece prefix, curve offset, curve length, partials, fade, noise offset}; params (n_rows x
 * pe_stim_param_fields() doubles, to be copied to the device) = every derived parameter, evaluated once in the
 * reference's order: {amplitude, a' , b', c', snr_db, sr, duration / n, 0, then per partial {amplitude, (2 pi f) h}},
 * glide: start, (end - start) / (n - 1), end; vibrato: base, depth / 1200, (2 pi) rate; totals2 = {samples, pieces}.
 * PE_E_ARG: n < 1, 0 < fade and n < fade, a non-finite or non-positive frequency, duration or sr, a non-finite
 * amplitude, more than 16 partials or none, a curve length other than 1 or n.
 *
 * Every entry point below checks its arguments and host_meta (the host copy of meta) before any device call, allocates
 * nothing, and launches the same number of kernels whatever the rows; pieces are counted from a row's own first sample
 * and reduced in a fixed order, so a row's output is bit-identical alone, packed at any offset or padded.  workspace:
 * pe_stim_workspace_bytes(totals2[1]) (PE_E_WORKSPACE when missing or too small).
 * pe_stim_phase: phase[sample prefix + i] = sum over j <= i of ((2 pi) curve[j]) / sr in double, for rows of kinds
 * 0 .. 2 (three launches: piece sums, per-row carries, the scan).  pe_stim_synth: y = float32(amplitude sin(phase)).
 * pe_stim_tone: rows of kind 3, y[i] = float32(sum_h a_h sin(((2 pi f) h) t[i])), t[i] = i (duration / n).
 * pe_stim_finish, in place on y: the raised-cosine fade float32(float64(y) window) (ramp[j] = 0.5 - 0.5 cos(j (pi /
 * (fade - 1))) over the head and mirrored over the tail, the tail overwriting an overlap); for rows with noise,
 * scale = float32((rms_s / 10^(snr_db / 20)) / rms_n) with both rms in double over the float32 samples, y = y +
 * float32(noise scale) in float32, skipped when either rms is 0; then with peak = max |y|, y = y / float32(peak + 1e-6)
 * if peak > 0.99.  stats[r] = {peak, rms_s, rms_n (0 without noise), scale (0: no mix)}.  Four launches: the mix of
 * pe_noise_mix below (one implementation, csrc/snr_mix.h), in place and under the fade.
 * pe_stim_reference: the reference's sample_reference_f0 without a per-sample curve: frame_table (n_rows x 2 int64,
 * host copy host_frame_table) = per row {frame prefix, frames}; frame_times (device doubles, made by the caller);
 * ref[f] = float32(np.interp(tau, float32(t), float32(curve))), a tone's curve being float32(frequency).
 *
 * pe_dynamic_metrics: tracks (n_rows x pe_dynamic_metrics_fields() int64; host_tracks its host copy) = per row
 * {offset in f0_pred, frames L, offset in f0_ref}.  out4[r] = {rms cents error (pe_pitch_metrics' expression), lag in
 * frames = argmax_k sum_n pred_c[n + k - (L - 1)] ref_c[n] - (L - 1) on the mean-centred tracks (first maximum;
 * positive when the prediction is late; NaN when every |centred| of either track is <= 1e-8), overshoot 1200
 * log2(max(pred) / ref[L - 1]) (NaN when either is <= 0), final error 1200 log2(max(pred[L - 1], 1e-5) /
 * max(ref[L - 1], 1e-5)) (NaN when ref[L - 1] <= 0)}; all NaN for L = 0.  One workgroup per row, O(L^2) for the lag. */
int pe_stim_plan_fields(void);
int pe_stim_param_fields(void);
int pe_stim_plan(int n_rows, const long* n, const long* y_off, const int* kind, const double* raw6,
                 const double* partials, const int* n_partials, const long* curve_off, const long* curve_len,
                 const long* noise_off, double sr, long* consts4, long* meta, double* params, long* totals2);
size_t pe_stim_workspace_bytes(long pieces);
int pe_stim_phase(const long* meta, const long* host_meta, const double* params, const float* curves, int n_rows,
                  double* phase, void* workspace, size_t workspace_bytes, void* stream);
int pe_stim_synth(const long* meta, const long* host_meta, const double* params, const double* phase, int n_rows,
                  float* y, void* stream);
int pe_stim_tone(const long* meta, const long* host_meta, const double* params, int n_rows, float* y, void* stream);
int pe_stim_finish(const long* meta, const long* host_meta, const double* params, const float* noise, int n_rows,
                   float* y, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int pe_stim_reference(const long* meta, const long* host_meta, const double* params, const float* curves,
                      const long* frame_table, const long* host_frame_table, const double* frame_times, int n_rows,
                      float* ref, void* stream);
int pe_dynamic_metrics_fields(void);
int pe_dynamic_metrics(const float* f0_pred, const float* f0_ref, const long* tracks, const long* host_tracks,
                       int n_rows, double* out4, void* stream);

/* ---- Additive noise at an SNR (what the reference's Utils/noise_robustness_evaluation.ipynb is meant to add), ragged
 * batches ------------------------------------------------------------------------------------------------------------
 * pe_noise_plan (host only): row r has n[r] >= 0 samples written at y + y_off[r], generated after warmup[r] >= 0
 * samples that are run and not written, from seeds[r]; white_off[r] = the offset of the row's warmup + n given white
 * samples in `white`, -1 for samples drawn in the kernel.  coeffs = {d0, d1, then (a, b) per section}, n_sections <= 8:
 * the colour y[j] = d0 w[j] + d1 w[j - 1] + sum_k s_k[j], s_k[j] = a_k s_k[j - 1] + b_k w[j], w[-1] = s_k[-1] = 0.
 * consts4 = {piece S = 2048, 8, doubles per row of `stats`, int64 per row of `beds`}; meta (n_rows x
 * pe_noise_plan_fields() int64, to be copied to the device) = per row {offset, samples, warm-up, generated = warm-up +
 * samples, pieces = ceil(generated / S) (0 for a row without samples), piece prefix, seed, white offset}; params
 * (pe_noise_param_fields() doubles, to be copied to the device) = {d0, d1, sections, 0, then per section {a, b,
 * a^(8 2^m) for m < 8, a^2048, 0}}, the powers by repeated multiplication and squaring in double; totals2 = {samples,
 * pieces}.  PE_E_ARG: more than 8 sections, a non-finite coefficient, |a| >= 1, a negative length, warm-up or offset.
 *
 * Every entry point below checks its arguments and host_meta (the host copy of meta) before any device call, allocates
 * nothing, and launches the same number of kernels whatever the rows; pieces are counted from a row's own first
 * generated sample and combined in a fixed order, so a row's output is bit-identical alone, packed at any offset or
 * padded.  Rows of length 0 are valid.  workspace: pe_noise_workspace_bytes(totals2[1]) (PE_E_WORKSPACE when missing
 * or too small).
 * pe_noise_white: y[i] = z(seed, warm-up + i), z(seed, j) the standard normal of pe_world_responses' drawn noise:
 * Philox4x32-10 with key {seed lo, seed hi} and counter {j lo, j hi, 0, 0}, u1 = ((w0 >> 8) + 0.5) 2^-24, u2 =
 * (w1 >> 8) 2^-24, sqrt(-2 ln u1) cos(2 pi u2) in float32.  One launch.
 * pe_noise_colour: the colour of `params` (host_params its host copy; PE_E_ARG unless it is pe_noise_plan's) over
 * w[j] = z(seed, j) or the given white[white offset + j] (n_white = floats in `white`), j < generated, in double,
 * rounded once to float32; y[i] = sample warm-up + i.  A parallel scan: piece end states from a zero state, per-row
 * carries in piece order, the pieces again from their carries.  Three launches.
 * pe_noise_bed: y[i] = bed[offset + (start + i) mod L] with beds (n_rows x 3 int64; host_beds its host copy) = per row
 * {offset in `bed`, L >= 1, 0 <= start < L}; n_bed = floats in `bed`.  PE_E_ARG for a bed outside it.  One launch.
 * pe_noise_mix: x, noise and y share the plan's offsets.  rms_s, rms_n in double over the float32 samples of the row,
 * scale = float32((rms_s / 10^(snr_db / 20)) / rms_n), y = x + float32(noise scale) in float32; y = x and scale = 0
 * when either rms is 0.  With peak = max |y|: y = y / float32(peak + 1e-6) if peak_normalize and peak > 0.99.
 * stats[r] = {peak, rms_s, rms_n, scale}, all 0 for a row of length 0.  snr_db: one double per row on the device,
 * host_snr_db its host copy, PE_E_ARG unless every one is finite.  Five launches (four without peak_normalize): the
 * mix that pe_stim_finish runs in place (one implementation, csrc/snr_mix.h), the row peaks in a launch of their own. */
int pe_noise_plan_fields(void);
int pe_noise_param_fields(void);
int pe_noise_plan(int n_rows, const long* n, const long* y_off, const long* warmup, const long* seeds,
                  const long* white_off, const double* coeffs, int n_sections, long* consts4, long* meta,
                  double* params, long* totals2);
size_t pe_noise_workspace_bytes(long pieces);
int pe_noise_white(const long* meta, const long* host_meta, int n_rows, float* y, void* stream);
int pe_noise_colour(const long* meta, const long* host_meta, const double* params, const double* host_params,
                    const float* white, long n_white, int n_rows, float* y, void* workspace, size_t workspace_bytes,
                    void* stream);
int pe_noise_bed(const long* meta, const long* host_meta, const float* bed, long n_bed, const long* beds,
                 const long* host_beds, int n_rows, float* y, void* stream);
int pe_noise_mix(const float* x, const float* noise, const long* meta, const long* host_meta, const double* snr_db,
                 const double* host_snr_db, int peak_normalize, int n_rows, float* y, double* stats, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- Room impulse responses by the image-source method and their decay time (the impulse-response files that the
 * reference's Utils/room_and_microphone_stress.ipynb reads and nobody ships), ragged batches --------------------------
 * One row is one response of a shoebox room.  params (n_rows x 19 doubles, made by the caller) = per row {Lx, Ly, Lz,
 * source x y z, microphone x y z, beta x0 x1 y0 y1 z0 z1 (wall at coordinate 0, wall at L), fs, c, N, max_order (-1:
 * none)}.  With R_a = (1 - 2 p_a) s_a + 2 n_a L_a - r_a over n in Z^3, p in {0, 1}^3, d = |R|, tau = d fs / c and
 * A = prod_a beta_a0^|n_a - p_a| beta_a1^|n_a| / (4 pi d) (0^0 = 1), an image with A != 0, tau < N + 41 and
 * sum_a |n_a - p_a| + |n_a| <= max_order adds v = A sinc(x) (1 + cos(pi x / 41)) / 2 at every 0 <= k < N with
 * x = k - tau, |x| < 41, and h[k] = float32(2^-44 sum rint(2^44 v)) with the sum in 64-bit integers: the result
 * depends on no order of addition.  d, tau, A and the taps are double.
 * pe_rir_plan (host only): consts4 = {tile length T = 256, 19, int64 per tile, doubles per row of pe_rir_decay's out};
 * meta (n_rows x pe_rir_plan_fields() int64, to be copied to the device) = per row {offset y_off[r], N, tiles =
 * ceil(N / T), tile prefix}; tiles (may be null: totals only; else tile_capacity >= totals2[1] entries of 2 int64, to
 * be copied to the device) = {row, first sample} of every tile, those with the most images first; totals2 = {samples,
 * tiles}.  PE_E_ARG: a non-finite value, a dimension, fs or c <= 0, a source or microphone not strictly inside the
 * room or less than 1 cm apart, a beta outside [0, 1], N < 1 or not an integer, max_order < -1 or not an integer, a
 * negative offset.  PE_E_UNSUPPORTED: N > 2^24; more than 2^20 tiles; a lattice index that could pass 2^30, (d_max + D)
 * / L_a + 8 >= 2^30 with D the room's diagonal and d_max = (N + 42) c / fs; or too little fixed-point headroom: the
 * bound 288 pi D^3 / V + (d_max + D)^2 / V on the sum of all image amplitudes must stay below 2^18 (the integer sum
 * holds |h| < 2^19).
 * pe_rir_synth: host_meta, host_params and host_tiles are the host copies; PE_E_ARG unless they are what pe_rir_plan
 * makes of host_params and the offsets, or if a row leaves the n_y floats of y.  One launch, one workgroup per tile,
 * whatever the rows; every sample of every row is written, nothing else is.  A row's samples are bit-identical alone,
 * in a batch in any order, at any offset or padded.
 * pe_rir_decay: Schroeder's backward integration of the rows of h (n_h floats) that meta describes (any row plan:
 * meta_fields int64 per row, opening with offset and length; host_meta its host copy).  E[k] = sum_{m >= k} h[m]^2 in
 * double, db[k] = 10 log10(E[k] / E[0]); k_lo, k_hi = the first k with db[k] < lo_db, hi_db (N when there is none);
 * the least-squares line of db over k / fs on k_lo <= k < k_hi.  out6 (n_rows x 6 doubles) = {T60 = -60 / slope,
 * slope in dB / s, intercept in dB, k_lo, k_hi, db[N - 1]}; T60, slope and intercept are NaN when hi_db is never
 * reached or k_hi - k_lo < 2.  curve (may be null): db[k] as float32 at the rows' offsets.  PE_E_ARG: fs <= 0, lo_db >
 * 0, hi_db >= lo_db, a row outside h.  One launch, one workgroup per row. */
int pe_rir_plan_fields(void);
int pe_rir_plan(int n_rows, const double* params, const long* y_off, long* consts4, long* meta, long* tiles,
                long tile_capacity, long* totals2);
int pe_rir_synth(const long* meta, const long* host_meta, const double* params, const double* host_params,
                 const long* tiles, const long* host_tiles, int n_rows, float* y, long n_y, void* stream);
int pe_rir_decay(const float* h, long n_h, const long* meta, const long* host_meta, int meta_fields, int n_rows,
                 double fs, double lo_db, double hi_db, double* out6, float* curve, void* stream);

/* ---- Training-time augmentation: per-row biquad cascades as a parallel scan, ragged batches -------------------------
 * pe_augment_biquad: row r (any row plan: meta_fields int64 per row, opening with offset and length; host_meta its host
 * copy) of x runs through its own cascade of n_stages[r] in 0 .. 8 biquads and is written to y at the same offset;
 * y == x (in place) is allowed.  sos (device, n_rows x 8 x 5 doubles; host_sos its host copy) = per row and stage
 * {b0, b1, b2, a1, a2} with a0 = 1; the stages past n_stages[r] are not read by the checks and not used.  The float32
 * input is widened to double, the stages are chained in double in transposed direct form II (y = b0 x + z1; z1 = b1 x
 * - a1 y + z2; z2 = b2 x - a2 y) from a zero state without a clamp or a rounding between them, and the result is
 * rounded once to float32: scipy.signal.sosfilt in float64 and a cast.  No stages is a copy.  One launch, one workgroup
 * per row, a parallel scan over pieces of the row (csrc/augment.hip); a row's output is bit-identical alone, packed at
 * any offset, padded, in place, and beside any other rows.  Checked before any device call, PE_E_ARG: a null pointer,
 * meta_fields < 2, a negative offset or length, n_stages outside 0 .. 8, a non-finite coefficient of a used stage, a
 * used stage whose poles lie outside the stability triangle (|a2| < 1, |a1| < 1 + a2) or whose pole radius exceeds
 * 1 - 2^-12 (what the error bound 2^-24 |y| + 2^-26 max |y| of the row stands on).  No workspace.
 * pe_augment_biquad_consts (host only): consts3 = {samples of a lane's piece, samples of a workgroup's block, 8}.
 * pe_augment_gain: y = float32(x gains[r]) over row r (gain and polarity in one multiply; y == x is allowed; gains on the
 * device, host_gains its host copy, PE_E_ARG unless every one is finite).  One launch. */
int pe_augment_biquad_consts(long* consts3);
int pe_augment_gain(const float* x, const long* meta, const long* host_meta, int meta_fields, int n_rows,
                    const float* gains, const float* host_gains, float* y, void* stream);
int pe_augment_biquad(const float* x, const long* meta, const long* host_meta, int meta_fields, int n_rows,
                      const double* sos, const double* host_sos, const int* n_stages, const int* host_n_stages,
                      float* y, void* stream);

/* ---- Codec stress conditions (reference Utils/codec_and_bandwidth_torture.ipynb): a build-defined MDCT transform
 * codec and G.711 mu-law on ragged batches (csrc/codec.hip; the specification is DESIGN.md section 28) --------------
 * frame = M in {256, 512, 1024} (anything else: PE_E_UNSUPPORTED).  A row of n >= 1 samples has ceil(n / M) + 1
 * frames, an empty row none; frame f reads the 2M samples from (f - 1) M on, zero outside the row.
 * pe_codec_plan (host only): row r has n[r] samples at x + x_off[r] and is written to y + y_off[r].  consts4 = {M,
 * floats of the table, bands, entries of a step table}; meta (n_rows x pe_codec_plan_fields() int64, to be copied to
 * the device) = per row {sample offset, samples, output offset, frames, frame prefix}; totals2 = {samples, frames}.
 * pe_codec_bands (host only): the band edges e_0 = 0, e_{b+1} = min(M, e_b + max(4, 4 (e_b / 32))) into edges (room
 * for at least 49 ints); returns the number of bands.
 * tables (n_table floats, device): exp(-2 pi i m / (M / 2)) for m < M / 2, exp(-i pi (8 n + 1) / 8M) for n < M / 2,
 * the window sin(pi (j + 0.5) / 2M) for j < 2M, T[i] = 2^((i - 224) / 4) and R[i] = 2^(-(i - 224) / 4) for i < 448,
 * all rounded from float64.
 * pe_codec_mdct: the rows' frames, in plan order, to coefs (frames x M).  One launch.
 * pe_codec_quantize: frames x M coefficients -> q (int32), the dequantised coefficients, and per frame the gain index
 * g and the bits of the cost model.  Bins >= k_c count as zero; 1 <= k_c <= M; budget >= 8 + the bands that begin
 * below k_c (else PE_E_ARG).  The arithmetic is exact, so the result is that of tests/codec_ref.py bit for bit.  One
 * launch.
 * pe_codec_imdct: coefs (frames x M, plan order) to the rows of y; workspace: pe_codec_workspace_bytes(M, frames), the
 * windowed frames, which a second launch gathers.  Two launches.
 * pe_codec_apply: mdct, quantize and imdct fused; the coefficients stay in LDS; the result is bit for bit that of the
 * three calls.  g and bits (one int32 per frame) may be null.  Two launches.
 * pe_codec_mulaw: G.711 mu-law encoded and decoded, y = decode(encode(x)), elementwise over the rows of any
 * pe_codec_plan (its frame only sets the work split).  One launch.
 * Every entry point checks its plan's host copy before any device call; a row's result is bit-identical alone, packed
 * at any offset, padded, and beside any other rows; the launch count does not depend on the rows. */
int pe_codec_plan_fields(void);
int pe_codec_plan(int n_rows, int frame, const long* n, const long* x_off, const long* y_off, long* consts4, long* meta,
                  long* totals2);
int pe_codec_bands(int frame, int* edges, int n_edges);
size_t pe_codec_workspace_bytes(int frame, long frames);
int pe_codec_mdct(const float* x, const long* meta, const long* host_meta, int n_rows, int frame, const float* tables,
                  long n_table, float* coefs, void* stream);
int pe_codec_quantize(const float* coefs, long frames, int frame, int k_c, int budget, const float* tables,
                      long n_table, int* q, int* g, int* bits, float* dequantised, void* stream);
int pe_codec_imdct(const float* coefs, const long* meta, const long* host_meta, int n_rows, int frame,
                   const float* tables, long n_table, float* y, void* workspace, size_t workspace_bytes, void* stream);
int pe_codec_apply(const float* x, const long* meta, const long* host_meta, int n_rows, int frame, int k_c, int budget,
                   const float* tables, long n_table, float* y, int* g, int* bits, void* workspace,
                   size_t workspace_bytes, void* stream);
int pe_codec_mulaw(const float* x, const long* meta, const long* host_meta, int n_rows, int frame, float* y,
                   void* stream);

/* ---- Pitch modulation of real audio: a per-sample time warp and its label pass, ragged batches (csrc/pitch_mod.hip;
 * the specification is DESIGN.md section 29) ---------------------------------------------------------------------
 * Row r of n[r] samples is warped over [t0[r], t1[r]] (samples; t1 - t0 a multiple of hop and >= hop, t1 <= n), the
 * span its kept label frames cover: y(t) = x(t0 + tau(t - t0)) with tau the closed-form map of mods[r] = {d[4],
 * rate_hz[4], phi[4], a} (up to 4 sinusoids, those with d = 0 absent, and one ramp), tau(0) = 0 and tau(T) = T pinned.
 * pe_pitch_mod_plan (host only, no device call): fills meta (n_rows x pe_pitch_mod_plan_fields() int64, opening with
 * offset and length), params (n_rows x 24 doubles: d, w = 2 pi rate / sr, phi, cos phi, a, mbar, T) and totals2 =
 * {tiles, rows that are warped}.  on[r] = 0, or a modulation that is all zero, makes row r a copy.  PE_E_ARG for a
 * selected row with a non-finite value, 2 sum|d| + |a| > 0.5, a rate below 0.05 Hz or a span as above it is not.
 * pe_pitch_mod_consts (host only): consts4 = {output samples of a tile, threads, staged source samples, 4}.
 * pe_pitch_mod_wave: one launch, one workgroup per (row, tile), out of place (x != y): y at y_off[r] gets row r of x
 * read through the filter of res_type (0 = kaiser_best, 1 = kaiser_fast; table = its zeros * 512 + 1 pairs {value,
 * forward difference}) with the cutoff scale = min(1, 1 / tau') per sample, float32 accumulation in a fixed tap order;
 * samples outside (t0, t1) and rows that are copies keep their bits.  table_in_lds = 1 reads the table from a copy in
 * LDS (kaiser_fast only, else PE_E_UNSUPPORTED); the result has the same bits.
 * pe_pitch_mod_labels: f0 and sil (n_rows x width float32, row r's kept frames first) to f0_out and sil_out: frame j
 * below the row's frame count (t1 - t0) / hop + 1 <= width reads position tau(j hop) / hop by the rule linear between
 * two voiced frames (f0 > 0 and flag 0), else the nearer frame (the earlier on a tie); a voiced result is multiplied by
 * tau' and gets flag 0, an unvoiced one copies f0 and flag; everything else is copied.  One launch.
 * Both check the plan's and the parameters' host copies before any device call; a row's result is bit-identical alone,
 * packed at any offset, padded, in any batch order and into any output stride. */
int pe_pitch_mod_consts(long* consts4);
int pe_pitch_mod_plan_fields(void);
int pe_pitch_mod_plan(int n_rows, const long* n, const long* x_off, const long* y_off, const long* t0, const long* t1,
                      const int* on, const double* mods, int sr, int hop, long* meta, double* params, long* totals2);
int pe_pitch_mod_wave(const float* x, const long* meta, const long* host_meta, const double* params,
                      const double* host_params, int n_rows, const float* table, int res_type, int table_in_lds,
                      float* y, void* stream);
int pe_pitch_mod_labels(const float* f0, const float* sil, const long* meta, const long* host_meta,
                        const double* params, const double* host_params, int n_rows, int hop, int width,
                        float* f0_out, float* sil_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PITCHEXTRACTOR_HIP_H */
