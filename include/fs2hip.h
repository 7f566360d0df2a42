/* fs2hip.h — C ABI of libfs2hip.so: hand-written gfx950 (CDNA4) kernels for the FastSpeech 2 hot path.
 *
 * The reference (ming024/FastSpeech2) has no FFI layer: its hot path is torch op call sites inside Python
 * nn.Modules.  Each entry point below replaces the torch ops at the cited reference location (paths relative
 * to the reference tree).  Host code above this ABI (fastspeech2_amd/*.py) mirrors the reference's Python
 * surface and binds these symbols with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller (incl. workspaces);
 *   - functions enqueue work on `stream` and return immediately: no allocation, no synchronisation,
 *     no global mutable state (re-entrant; safe from autograd / DDP hook threads);
 *   - return 0 on success; <0 on error (FS2_EINVAL -1 bad shape/null, FS2_EDTYPE -2, FS2_ELAUNCH -3),
 *     message via fs2_last_error() (thread-local);
 *   - dtype: 0 = float32, 1 = bfloat16 (storage of activations / packed weights; accumulation, statistics,
 *     parameters, gradients of parameters and optimiser state are always float32);
 *   - activations are time-major rows [B*S][C] with C contiguous (== the reference's (B, S, C) tensors);
 *   - `lens` (int32 per sequence) replaces the reference's bool masks: row t of sequence b is padding iff
 *     t >= lens[b] (utils/tools.py:91-99 get_mask_from_lengths).
 */
#ifndef FS2HIP_H
#define FS2HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* fs2_stream_t; /* == hipStream_t */

enum { FS2_F32 = 0, FS2_BF16 = 1 };
enum { FS2_ACT_NONE = 0, FS2_ACT_RELU = 1, FS2_ACT_TANH = 2, FS2_ACT_LRELU = 3,
       FS2_ACT_GATE = 4 /* Y = (R > 0) ? acc+bias : 0 : ReLU backward fused into the data-gradient GEMM */ };

int fs2_version(void);
const char* fs2_last_error(void);

/* ---- dense contractions (MFMA) -------------------------------------------------------------------- */
/* Y[m][n] = ((act(sum_{j<taps} sum_c X[m + j*dil - pad][c] * W[n][j][c] + bias[n])) + R[m][n]) * out_scale
 * (+= Y if accumulate); taps shifted outside their sequence [0,S) contribute 0; rows t >= lens[b] -> 0.
 * Replaces nn.Linear / nn.Conv1d forward AND data-gradient (with the tap-flipped pack):
 *   transformer/SubLayers.py:39-41,54 (w_qs/w_ks/w_vs/fc), :87-88 (w_1 k=9, w_2 k=1);
 *   model/modules.py:209-240,291-296 (VariancePredictor Conv k=3); model/fastspeech2.py:95 (mel_linear);
 *   transformer/Layers.py:129-137 (PostNet k=5); hifigan/models.py:96-103,150-163; audio/stft.py:66-72. */
int fs2_conv_gemm(const void* X, long ldx, const void* Wpacked, const float* bias, const void* R, long ldr, void* Y,
                  long ldy, const int32_t* lens, const int32_t* tile_map, int M, int N, int Cin, int S, int taps, int dil,
                  int pad, int act, float slope, int in_act, float in_slope, int accumulate, float out_scale, int dtype,
                  fs2_stream_t stream);
/* tile_map (optional, from fs2_tile_map with rows = 256 for the same lens / S / M): lets the persistent kernel deal only
 * the M-tiles that hold valid rows to its workgroups.  With lens != NULL and tile_map == NULL the non-persistent kernels
 * run (same results).
 * fs2_tile_map: out[0] = number of REAL `rows`-row M-tiles of the [B*S] row space, out[1..] = their indices (ascending)
 * followed by the fully padded ones (all rows in one sequence's tail t >= lens[b]); out holds 1 + ceil(B*S/rows) ints. */
int fs2_tile_map(const int32_t* lens, int B, int S, int rows, int32_t* out, fs2_stream_t stream);
/* Everything a step derives from a lengths vector (int64, as the reference's batches carry them) in one launch:
 * lens32[b] = min(len[b], S); mask[b][t] = (t >= len[b]) as bytes (the bool masks FastSpeech2.forward returns, True = padding,
 * reference utils/tools.py:91-99); count[0] = sum_b lens32[b] (FastSpeech2Loss's valid-position count); tile_map as fs2_tile_map
 * (optional). */
int fs2_lens_prep(const int64_t* lens, int B, int S, int rows, int32_t* lens32, void* mask, float* count, int32_t* tile_map,
                  fs2_stream_t stream);
/* fs2_conv_gemm with scratch for the persistent kernel's TAIL SPLIT: when the output tiles do not fill a whole number of rounds
 * over the CUs, the last partial round is K-split (2 / 4 / 8 ways) so that it costs a fraction of a round instead of a whole
 * one; the parts store f32 partial tiles into tail_ws and one more launch sums them and applies the epilogue.  tail_ws:
 * fs2_conv_gemm_tail_ws_bytes() bytes, 16-byte aligned, any contents, not shared by launches that may run concurrently; NULL =
 * fs2_conv_gemm.  Launches the persistent kernel does not take ignore it. */
int fs2_conv_gemm_tail_ws_bytes(void);   /* a size, not a status */
int fs2_conv_gemm_tail(const void* X, long ldx, const void* Wpacked, const float* bias, const void* R, long ldr, void* Y,
                       long ldy, const int32_t* lens, const int32_t* tile_map, float* tail_ws, int M, int N, int Cin, int S,
                       int taps, int dil, int pad, int act, float slope, int in_act, float in_slope, int accumulate,
                       float out_scale, int dtype, fs2_stream_t stream);
/* K-split form for few-tile, long-reduction contractions: `ksplit` workgroups per output tile store partial tiles into ws
 * (f32 scratch, ksplit x M x N, any contents), one more launch sums them and finalises (bias, activation, residual, bf16).
 * bf16 only, Cin % (64 ksplit) == 0; FS2_EINVAL for unsupported shapes (fall back to fs2_conv_gemm). */
int fs2_conv_gemm_splitk(const void* X, long ldx, const void* Wpacked, const float* bias, const void* R, long ldr, void* Y,
                         long ldy, const int32_t* lens, const int32_t* tile_map, float* ws, int ksplit, int M, int N, int Cin,
                         int S, int taps, int dil, int pad, int act, float slope, float out_scale, int dtype,
                         fs2_stream_t stream);
/* fs2_conv_gemm_tail for HiFi-GAN's pre-activation chains when the activations are STORED leaky-ReLU'd (hifigan/models.py:96-103:
 * every convolution's input is leaky_relu(x), the residual is the raw x): the producer stores lrelu(value) (post_slope = slope,
 * applied last: after residual, out_scale and accumulate), the next convolution reads it with no prologue, and a residual operand
 * stored that way is undone on the fly (res_unlrelu = 1 / slope: r > 0 ? r : r * res_unlrelu).  0 switches either off. */
int fs2_conv_gemm_lrelu_io(const void* X, long ldx, const void* Wpacked, const float* bias, const void* R, long ldr, void* Y,
                           long ldy, float* tail_ws, int M, int N, int Cin, int S, int taps, int dil, int pad, int act, float slope,
                           int accumulate, float out_scale, float res_unlrelu, float post_slope, int dtype, fs2_stream_t stream);
/* Measurement aid: a back-to-back v_mfma_f32_32x32x16_bf16 stream on every SIMD of the chip (one 256-thread workgroup per CU,
 * iters x 8 MFMAs per wave); *flops receives the FLOPs of the launch.  bench.py times it to report what the matrix pipes SUSTAIN
 * under the chip's power management beside the nominal peak.  sink: one float of device memory (never written in practice). */
int fs2_mfma_calibrate(int iters, float* sink, double* flops, fs2_stream_t stream);
/* The memory-side calibrations reported beside it (roofline.hbm_copy / roofline.l2_to_lds): a 16-byte-per-lane copy of `bytes`
 * (src -> dst), and an LDS-DMA stream of an L2-resident window on every CU (8 waves x 4 KiB in flight; *bytes = bytes moved). */
int fs2_hbm_calibrate(const void* src, void* dst, size_t bytes, fs2_stream_t stream);
int fs2_ldsdma_calibrate(const void* src, size_t src_bytes, int iters, float* sink, double* bytes, fs2_stream_t stream);
/* Which kernel fs2_conv_gemm dispatches a launch description to: a pure function (no state) - a measurement aid that
 * lets bench.py attribute HIP-event durations to the kernel names rocprofv3 reports.  has_lens / has_map: whether
 * lens / tile_map would be non-NULL; ldr = 0 without a residual operand. */
#define FS2_GEMM_PLAIN 1   /* conv_gemm_kernel: 128x128 register-staged */
#define FS2_GEMM_DMA 2     /* conv_gemm_dma_kernel: 128x128 LDS-DMA, halo reuse (incl. in-workgroup split-K) */
#define FS2_GEMM_RING 3    /* conv_gemm_ring_kernel: 256x128 wave-specialised (shapes the persistent kernel declines; lrelu_io launches with a residual) */
#define FS2_GEMM_SKINNY 4  /* conv_skinny_kernel: C = 32 / 64 */
#define FS2_GEMM_PERSIST 5 /* conv_gemm_p_kernel<false>: persistent 256x128 convolution (taps >= 3), MFMA-bound */
#define FS2_GEMM_PERSIST_1TAP 6 /* conv_gemm_p_kernel<true>: the same kernel for taps == 1 (Linear / k=1 conv): HBM-bound at K <= 1024 */
#define FS2_GEMM_WIDE_1TAP 7 /* conv_gemm_w_kernel: persistent 256x256 tiles, every wave loads and multiplies (taps == 1, N % 256 == 0) */
/* (8 was round 4's 512x128 tall-tile kernel: measured slower at every shape of the model and removed from the library in round 5;
 *  git history: fastspeech2_amd/csrc/fs2_gemm_t.hip at ff5fda0) */
#define FS2_GEMM_STREAM_K256 9 /* conv_gemm_s_kernel: one tap, K = 256, N % 256 == 0 - weights in registers, X streamed through LDS (HBM-bound) */
int fs2_conv_gemm_variant(long ldx, long ldy, long ldr, int has_lens, int has_map, int M, int N, int Cin, int S, int taps,
                          int dil, int in_act, float in_slope, int dtype);
/* ... and of a fs2_conv_gemm_lrelu_io launch (its dispatch also looks at the epilogue operands: residual / accumulate launches with
 * a short reduction go to the ring kernel's LDS-staged epilogue) */
int fs2_conv_gemm_lrelu_io_variant(long ldx, long ldy, long ldr, int accumulate, int M, int N, int Cin, int S, int taps, int dil,
                                   int act, float res_unlrelu, float post_slope, int dtype);
/* Master conv weights are stored tap-major W[n][j][c] f32 (the (Cout,Cin,k) nn.Parameter is a permuted view of it):
 * -> Wf[n][j][c] (forward: dtype cast) and/or Wd[c][j][n] = W[n][k-1-j][c] (data gradient: tap flip + transpose). */
int fs2_pack_weight(const float* w, void* wf, void* wd, int Cout, int Cin, int k, int dtype, fs2_stream_t stream);
/* All data-gradient packs of a model in ONE launch.  table (device, int64 [n_entries][6]) = {src element offset into
 * flat, dst element offset into wd_base, Cout, Cin, k, first 64x64 tile index}; total_tiles = sum over entries of
 * ceil(Cout/64)*ceil(Cin/64)*k.  Each entry is packed as fs2_pack_weight's Wd (tap flip + transpose, LDS-tiled). */
int fs2_pack_dgrad_multi(const float* flat, void* wd_base, const int64_t* table, int n_entries, int total_tiles, int dtype,
                         fs2_stream_t stream);
/* dW[n][j][c] += sum_m dY[m][n] * X[m + j*dil - pad][c]   (tap-major master layout, f32, atomic accumulate);
 * dbias (optional): dbias[n] += sum_m dY[m][n], fused into the same pass over dY (the conv/linear bias gradient).
 * lens (optional): the caller guarantees dY rows t >= lens[b] are zero, so their K-tiles are skipped. */
int fs2_conv_wgrad(const void* dY, long lddy, const void* X, long ldx, float* dW, float* dbias, const int32_t* lens, int M,
                   int N, int Cin, int S, int taps, int dil, int pad, int dtype, fs2_stream_t stream);
/* The same with a split-K workspace (round 3): every split stores its partial tile into its own f32 copy of dW inside `ws`
 * (plain stores) and one more launch sums the splits into dW / dbias in index order - no atomics, bit-reproducible gradients,
 * and (dil == 1) tap groups of up to 5 taps that share one set of X fragment reads.  ws: fs2_conv_wgrad_ws_bytes(...) bytes for
 * the same shape, 16-byte aligned, any contents, not shared by launches that may run concurrently; NULL or too small = the
 * atomic path of fs2_conv_wgrad.  bf16 only (fp32 ignores ws).  fs2_conv_wgrad_ws_bytes returns a size, not a status. */
int fs2_conv_wgrad_ws_bytes(int M, int N, int Cin, int S, int taps, int dil, int has_lens, int dtype);
int fs2_conv_wgrad_ws_cap(void);     /* upper bound of fs2_conv_wgrad_ws_bytes over all shapes that get a workspace at all (a size, not a status) */
int fs2_conv_wgrad_ws(const void* dY, long lddy, const void* X, long ldx, float* dW, float* dbias, const int32_t* lens, int M,
                      int N, int Cin, int S, int taps, int dil, int pad, int dtype, float* ws, long ws_bytes, fs2_stream_t stream);
/* out[n] += sum_m x[m][n]  (bias gradients) */
int fs2_colsum(const void* x, long ldx, float* out, int M, int N, int dtype, fs2_stream_t stream);

/* ---- attention: transformer/Modules.py:14-25 + head split/merge SubLayers.py:39-52 ----------------- */
/* qkv [B*S][3*H*128] = (q|k|v); ctx [B*S][H*128]; lse [B][H][S] f32 (saved for backward). */
int fs2_attn_fwd(const void* qkv, void* ctx, float* lse, const int32_t* lens, int B, int S, int H, int dk, float scale,
                 int dtype, fs2_stream_t stream);
/* delta [B][H][S] f32 workspace; dqkv [B*S][3*H*128] receives (dq|dk|dv). */
int fs2_attn_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* delta, void* dqkv,
                 const int32_t* lens, int B, int S, int H, int dk, float scale, int dtype, fs2_stream_t stream);

/* ---- LayerNorm family: SubLayers.py:54-55,90-91 + Layers.py:25,28; model/modules.py:222-240 -------- */
/* z = drop_pre(y) + res (written back into y); out = mask(drop_post(LN(z)*gamma+beta)); saves mean/rstd. */
int fs2_ln_fwd(void* y, const void* res, const float* gamma, const float* beta, const int32_t* lens, void* out,
               float* mean, float* rstd, int B, int S, int C, float eps, float p_pre, uint64_t seed_pre, float p_post,
               uint64_t seed_post, const uint64_t* seed_dev, int dtype, fs2_stream_t stream);
/* gemm_res_ln: the N = 256 projection of a transformer sub-layer AND its LayerNorm in one launch (SubLayers.py:54-55, 90-93 +
 * Layers.py:25,28): Z = dropout_pre(X W^T + bias) + R (bf16, saved for backward: what fs2_ln_fwd leaves in y),
 * out = mask(LN(Z) * gamma + beta), mean / rstd saved.  Same dropout stream and statistics as fs2_conv_gemm + fs2_ln_fwd; the
 * projection's output is never stored (one bf16 rounding less).  bf16, N == 256, Cin % 32 == 0; fs2_gemm_res_ln_supported
 * returns 1 / 0 (a flag, not a status) - otherwise call the two entry points. */
int fs2_gemm_res_ln_supported(int M, int N, int Cin, int S, int dtype);
/* 1 when the shape runs on the streaming K = 256 kernel (weights in registers, 64-row tiles: every CU busy at the decoder's M) */
int fs2_gemm_res_ln_streams(int M, int N, int Cin, int S, int dtype);
int fs2_gemm_res_ln_fwd(const void* X, long ldx, const void* Wpacked, const float* bias, const void* R, long ldr, void* Z, long ldz,
                        void* out, long ldo, const float* gamma, const float* beta, float* mean, float* rstd, const int32_t* lens,
                        const int32_t* tile_map, int M, int N, int Cin, int S, float eps, float p_pre, uint64_t seed_pre,
                        const uint64_t* seed_dev, int dtype, fs2_stream_t stream);
/* d1 = dz (+ d1_add), d2 = dz * dropmask_pre * (relu_bwd ? z>0 : 1); dgamma/dbeta += column sums.
 * partial_ws: caller workspace of per-block partial sums, reduced by a 2nd launch: FS2_LN_BWD_GRID*2*C floats when dgamma /
 * dbeta are given (nothing is written beyond that).  dgamma = dbeta = NULL DEFERS the reduction: the workspace must then hold
 * FS2_LN_BWD_GRID*2*C + 4 floats (the block count is stored behind the partials) and the caller runs
 * fs2_ln_bwd_reduce(partial_ws, ...) later, on any stream ordered after this call, before partial_ws is reused. */
#define FS2_LN_BWD_GRID 1024
int fs2_ln_bwd(const void* z, const void* dout, const float* gamma, const int32_t* lens, const float* mean,
               const float* rstd, const void* d1_add, void* d1, void* d2, float* dgamma, float* dbeta,
               float* partial_ws, int B, int S, int C, float p_pre, uint64_t seed_pre, float p_post, uint64_t seed_post, const uint64_t* seed_dev,
               int relu_bwd, int dtype, fs2_stream_t stream);
int fs2_ln_bwd_reduce(const float* partial_ws, int C, float* dgamma /*+=*/, float* dbeta /*+=*/, fs2_stream_t stream);
/* fs2_ln_bwd with the upstream gradient given as a SUM of two tensors, dout + dout2 (dout2 may be NULL = fs2_ln_bwd): the residual
 * branch's gradient reaches the LayerNorm below a sub-layer as "data gradient of the sub-layer + gradient that bypassed it"
 * (autograd of `output + residual`, transformer/SubLayers.py:55,91).  Rounds 1-5 added the bypass term in the epilogue of the
 * contraction that produced the first (16 dependent residual loads behind the tile's own stores: 25-45 us per launch); here it is one
 * more coalesced row read of an HBM-bound kernel. */
int fs2_ln_bwd_sum(const void* z, const void* dout, const void* dout2, const float* gamma, const int32_t* lens, const float* mean,
                   const float* rstd, const void* d1_add, void* d1, void* d2, float* dgamma, float* dbeta,
                   float* partial_ws, int B, int S, int C, float p_pre, uint64_t seed_pre, float p_post, uint64_t seed_post, const uint64_t* seed_dev,
                   int relu_bwd, int dtype, fs2_stream_t stream);

/* ---- BatchNorm1d (+tanh, +dropout) of PostNet: transformer/Layers.py:129-137 ------------------------ */
/* Column sums are bit-reproducible: every reducing launch stores per-workgroup partial sums in a workspace and a second tiny
 * launch adds them in index order (no float atomics, no device-scope fences).  A BN workspace holds fs2_bn_ws_floats(C)
 * floats (any contents); its first 2C floats receive the sums.  Every reducing entry point takes the workspace's size in floats
 * (`ws_floats`) right behind the pointer and refuses one smaller than fs2_bn_ws_floats(C) - rounds 1-3 needed 2C floats, so a caller
 * built against the old prototype now fails at the call instead of being written out of bounds. */
int fs2_bn_ws_floats(int C);
int fs2_bn_stats(const void* x, float* stats /*workspace; [0,2C) = sum | sum of squared deviations*/, long ws_floats, int M, int C,
                 int dtype, fs2_stream_t stream);
/* train-mode statistics without housekeeping launches; also updates the running statistics and increments
 * num_batches_tracked (int64, optional) - nn.BatchNorm1d's buffers. */
int fs2_bn_train_stats(const void* x, float* stats_ws, long ws_floats, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, float* mean_rstd, int M, int C, float eps, float momentum, int dtype,
                       fs2_stream_t stream);
int fs2_bn_finalize(const float* stats, float* running_mean, float* running_var, float* mean_rstd /*2C*/, int M, int C,
                    float eps, float momentum, fs2_stream_t stream);
/* out = drop(act(BN(x))) + res ; seed_dev (optional, device) is added to every dropout seed so that a replayed
 * hipGraph draws a fresh mask each step. */
int fs2_bn_apply(const void* x, const float* mean_rstd, const float* gamma, const float* beta, const void* res, void* out,
                 int M, int C, int act, float p, uint64_t seed, const uint64_t* seed_dev, int dtype, fs2_stream_t stream);
/* fs2_bn_apply that also writes fp32 images: out32 [M][C] = the result as stored in `dtype`, widened (bit for bit what fs2_cast
 * makes of `out`); res32 (optional, needs res) = the residual operand widened.  out may be NULL (only the fp32 image wanted). */
int fs2_bn_apply_out32(const void* x, const float* mean_rstd, const float* gamma, const float* beta, const void* res, void* out,
                       float* out32, float* res32, int M, int C, int act, float p, uint64_t seed, const uint64_t* seed_dev,
                       int dtype, fs2_stream_t stream);
int fs2_bn_bwd(const void* x, const void* dout, const float* mean_rstd, const float* gamma, const float* beta,
               float* sums /*workspace; [0,2C) = dbeta|dgamma*/, long ws_floats, void* dx, int M, int C, int act, float p,
               uint64_t seed, const uint64_t* seed_dev, int dtype, fs2_stream_t stream);
/* the same with dgamma_acc / dbeta_acc (parameter-gradient buffers) += the reduced sums; successive calls on one stream may
 * share one workspace. */
int fs2_bn_bwd_acc(const void* x, const void* dout, const float* mean_rstd, const float* gamma, const float* beta, float* sums,
                   long ws_floats, void* dx, float* dgamma_acc, float* dbeta_acc, int M, int C, int act, float p, uint64_t seed,
                   const uint64_t* seed_dev, int dtype, fs2_stream_t stream);

/* ---- gathers / index kernels ----------------------------------------------------------------------- */
/* transformer/Models.py:89-91: out = src_word_emb[tok] + position_enc[t] */
int fs2_embed_pe_fwd(const int64_t* tokens, const float* emb, const float* pe, void* out, int B, int L, int C, int V,
                     int dtype, fs2_stream_t stream);
int fs2_embed_bwd(const int64_t* tokens, const void* dy, float* demb, int rows, int C, int V, int pad_idx, int dtype,
                  fs2_stream_t stream);
/* model/fastspeech2.py:68-71: x[b,t,:] += speaker_emb[speakers[b]] */
int fs2_add_rowvec(void* x, const float* table, const int64_t* idx, int B, int S, int C, int V, int dtype,
                   fs2_stream_t stream);
int fs2_rowvec_bwd(const void* dy, float* dtable, const int64_t* idx, int B, int S, int C, int V, int dtype,
                   fs2_stream_t stream);
/* model/modules.py:80-100,121,126: out = x + emb[bucketize(vals*scale, bins)] ; idx_out saved for backward */
int fs2_bucket_embed_add_fwd(const void* x, const float* vals, float scale, const float* bins, int nbins,
                             const float* emb, void* out, int32_t* idx_out, int rows, int C, int dtype,
                             fs2_stream_t stream);
/* demb[n_bins][C] (fp32) += rows of dy grouped by bucket index (gather-reduce per bin, one atomic per channel and row split) */
int fs2_bucket_embed_bwd(const int32_t* idx, const void* dy, float* demb, int rows, int n_bins, int C, int dtype,
                         fs2_stream_t stream);
/* model/modules.py:167-194 LengthRegulator (+ utils/tools.py:299-317 pad): integer index map, bit-exact.
 * cum [B][L+1] int32 exclusive prefix sums of max((int)d,0); idx [B][T] frame->phoneme (-1 = padding);
 * mel_len [B] int64 = un-cropped total (Appendix A #4). */
int fs2_lr_index(const void* durations, int dur_is_float, int B, int L, int T, int32_t* cum, int32_t* idx,
                 int64_t* mel_len, fs2_stream_t stream);
/* out[b,t,:] = x[b,idx[b,t],:] (0 if idx<0) + (pe ? pe[t,:] : 0)  — pe fuses Decoder's position_enc add
 * (transformer/Models.py:154-162). */
int fs2_lr_gather_fwd(const void* x, const int32_t* idx, const float* pe, void* out, int B, int L, int T, int C,
                      int dtype, fs2_stream_t stream);
int fs2_lr_gather_bwd(const void* dy, const int32_t* cum, void* dx, int B, int L, int T, int C, int accumulate,
                      int dtype, fs2_stream_t stream);
/* fs2_lr_gather_bwd and the residual adds behind it in one launch: dx0 = segment sums, dx1 = dx0 + add1, dx2 = dx1 + add2
 * (add2 / dx2 optional), every stage rounded to `dtype` before the next add - bit for bit fs2_lr_gather_bwd + fs2_add + fs2_add. */
int fs2_lr_gather_bwd_add(const void* dy, const int32_t* cum, const void* add1, const void* add2, void* dx0, void* dx1, void* dx2,
                          int B, int L, int T, int C, int dtype, fs2_stream_t stream);
/* model/modules.py:132-135: clamp(round_half_even(exp(log_d)-1) * d_control, min=0) */
int fs2_duration_round(const float* logd, float d_control, float* out, int n, fs2_stream_t stream);
/* model/modules.py:243-249: out[r] = mask(dot(x[r,:], w) + b) */
int fs2_rowdot_fwd(const void* x, const float* w, const float* bias, const int32_t* lens, float* out, int B, int S, int C,
                   int dtype, fs2_stream_t stream);
int fs2_rowdot_bwd(const void* x, const float* w, const float* g, const int32_t* lens, void* dx, float* dw, float* db,
                   int B, int S, int C, int dtype, fs2_stream_t stream);
/* transformer/Layers.py:25,28 masked_fill(mask, 0) in place */
int fs2_mask_rows(void* x, const int32_t* lens, int B, int S, int C, int dtype, fs2_stream_t stream);
int fs2_cast(const void* in, int in_dtype, void* out, int out_dtype, size_t n, fs2_stream_t stream);
int fs2_add(const void* a, const void* b, void* out, size_t n, int dtype, fs2_stream_t stream);
/* transformer/Models.py:154-162 (frame-level variance configs): x[b,t,:] += position_enc[t,:] */
int fs2_add_pe(void* x, const float* pe, int B, int S, int C, int dtype, fs2_stream_t stream);
int fs2_bump_counter(uint64_t* ctr, uint64_t inc, fs2_stream_t stream);

/* ---- vocoder (hifigan/models.py:113-174, utils/model.py:74-92) and mel extraction (audio/stft.py) ---- */
/* The dense layers run in fs2_conv_gemm:
 *   conv_pre / ResBlock convs   taps=k, dil, in_act = leaky_relu(0.1), residual / accumulate / out_scale=1/3 epilogue
 *                               (models.py:96-103,150,155-160);
 *   ConvTranspose1d(k=2u, stride u, pad u/2) as its polyphase form: a 3-tap conv with N = u*Cout whose output rows
 *                               [B*T][u*Cout] ARE the up-sampled time-major rows [B*T*u][Cout] (models.py:124-135,152-153);
 *   framed DFT                  X = reflect-padded wav viewed as rows [B*rows][hop], taps = filter/hop (stft.py:66-72).
 * (B, C, T) float32 -> rows [B*T][C] in `dtype` (vocoder_infer receives mels channel-major, utils/model.py:74-80). */
int fs2_chan_to_rows(const float* in, void* out, int B, int C, int T, int dtype, fs2_stream_t stream);
/* models.py:161-163 + utils/model.py:82-85: y = tanh(conv(leaky_relu(x, in_slope), w[taps][C]) + bias);
 * wav[m] = y (optional), pcm[m] = (int16)(y * max_wav_value) with numpy's astype semantics (optional). */
int fs2_conv_post_pcm(const void* x, long ldx, const float* w, const float* bias, float in_slope, float* wav,
                      int16_t* pcm, float max_wav_value, int M, int S, int C, int taps, int pad, int dtype,
                      fs2_stream_t stream);
/* hifigan/models.py:96-103 + 155-160: a whole ResBlock1 of the narrow stages (C = 32 / 64, bf16) in ONE launch -
 *   y = x; for m in 0..2: t = lrelu(conv1_m(lrelu(y), dilation d_m)); y = conv2_m(t) + y;  xs = (accumulate ? xs : 0) + out_scale * y
 * x / xs: rows [B*S][C] (time-major); w1 / w2: [3][C][k][C] (convs1 / convs2 of the block, cout-major, tap, cin), b1 / b2: [3][C] f32.
 * The running sum stays in fp32 registers, the convolutions' operands in LDS: x is read once, xs read + written once.
 * post_slope > 0: the xs written is leaky_relu(xs, post_slope) (the next up-sampling convolution then needs no prologue).
 * fs2_resblock_supported: 1 when a (C, k, dilations, dtype) combination has an instantiation (else run the convolutions one by one). */
int fs2_resblock_supported(int C, int k, int d0, int d1, int d2, int dtype);
int fs2_resblock_fwd(const void* x, long ldx, const void* w1, const void* w2, const float* b1, const float* b2, void* xs,
                     long ldxs, int accumulate, float out_scale, float slope, float post_slope, int B, int S, int C, int k, int d0,
                     int d1, int d2, int dtype, fs2_stream_t stream);
/* models.py:155-160 for a whole up-sampling stage: the three residual blocks (kernel sizes ka / kb / kc, same dilations) of one x
 * in ONE launch - xs = out_scale * (block_a(x) + block_b(x) + block_c(x)), the running xs rounded to the storage dtype after
 * every block (as the per-block launches stored it): x is read once from HBM (twice more from L2), xs written once. */
int fs2_resstage_fwd(const void* x, long ldx, const void* w1a, const void* w2a, const float* b1a, const float* b2a, int ka,
                     const void* w1b, const void* w2b, const float* b1b, const float* b2b, int kb, const void* w1c,
                     const void* w2c, const float* b1c, const float* b2c, int kc, void* xs, long ldxs, float out_scale,
                     float slope, float post_slope, int B, int S, int C, int d0, int d1, int d2, int dtype, fs2_stream_t stream);
/* ---- MelGAN generator (fastspeech2_amd/melgan.py states the network) ----
 * Guard rows for reflection-padded convolutions on the zero-padding contraction kernels: dst holds [B][G + S + G] rows of C channels
 * (row stride ld_dst, item stride dst_bstride, both in elements); row G + t of item b is src row t (src: row stride ld_src, item
 * stride src_bstride, pointing at row 0 of item 0).  Guard rows t in [-G, 0) and [S, S + G) <- src row reflect(t) = -t resp.
 * 2 (S - 1) - t (reflect = 1, needs S > G: F.pad(mode="reflect")) or zeros (reflect = 0: in front of a transposed convolution).
 * interior = 1 copies rows [0, S) too (src and dst are different buffers); interior = 0 writes the 2G guard rows only (in place:
 * src = dst + G * ld_dst). */
int fs2_melgan_guard_rows(const void* src, long ld_src, long src_bstride, void* dst, long ld_dst, long dst_bstride, int B, int S,
                          int G, int C, int reflect, int interior, int dtype, fs2_stream_t stream);
/* The three ResnetBlocks of a narrow up-sampling stage (C = 32 / 64, bf16) in ONE launch:
 *   for d in (d0, d1, d2):  x = shortcut(x) + conv4(lrelu(conv3(reflect_pad_d(lrelu(x)), dilation d)))       (k = 3, 1, 1; lrelu slope)
 * x / y: row t of item b at base + b * bstride + t * ld (elements); reflection at the ends of [0, S) of every item.
 * w: [3][5C][C] (per block: conv3 tap 0, 1, 2 as [cout][cin], shortcut, conv4), bias: [3][2][C] f32 (conv3's; shortcut's + conv4's).
 * y = leaky_relu(result, out_slope) when out_slope > 0.  x is read once, y written once; S >= 32, dilations <= 9.
 * fs2_melgan_stage_supported: 1 when (C, dtype) has an instantiation (a flag, not a status) - otherwise run the convolutions one by one. */
int fs2_melgan_stage_supported(int C, int dtype);
int fs2_melgan_stage_fwd(const void* x, long ldx, long x_bstride, const void* w, const float* bias, void* y, long ldy, long y_bstride,
                         float slope, float out_slope, int B, int S, int C, int d0, int d1, int d2, int dtype, fs2_stream_t stream);
/* stft.py:60-66: xp[b][i] = y[b][reflect(i - P)], i < N + 2P; zero-filled up to row_len. */
int fs2_reflect_pad(const float* y, float* xp, int B, int N, int P, long row_len, fs2_stream_t stream);
/* The same for a ragged batch (preprocessor/preprocessor.py:194 over a corpus): row b holds lens[b] samples (row stride ldy,
 * lens[b] > P else the row is zero-filled) and is reflected at its own end. */
int fs2_reflect_pad_ragged(const float* y, long ldy, const int32_t* lens, float* xp, int B, int P, long row_len,
                           fs2_stream_t stream);
/* stft.py:74-78,174-176 + audio_processing.py:91: ft rows [B*S][2*NF] (Re|Im) -> mel (B, n_mel, frames) =
 * log(clamp(mel_basis[n_mel][NF] . |ft|, clamp_min)), energy (B, frames) = ||ft|||_2; span[n_mel][2] = non-zero
 * band [lo, hi) of each filter. */
int fs2_stft_mel_epilogue(const float* ft, long ldft, const float* mel_basis, const int32_t* span, float* mel,
                          float* energy, int B, int S, int frames, int NF, int n_mel, float clamp_min,
                          fs2_stream_t stream);

/* ---- Griffin-Lim mel inversion (audio/stft.py:52-122, audio/audio_processing.py:7-82, audio/tools.py:18-34) ----
 * Frame-major rows: utterance b owns rows [b*Fmax, (b+1)*Fmax) of which frames[b] are frames (frames == NULL: all Fmax);
 * G rows are [m cos(phi) (NF) | m sin(phi) (NF) | 0 up to ldg], the inverse GEMM's input.  Every padding entry (rows
 * f >= frames[b], columns >= 2 NF) is written as 0.  Strided operands: element (b, f, k) at b*sb + f*sf + k*sk.
 * fs2_gl_mel_to_mag: log-mel (element (b, j, t) at b*sb + j*sj + t*st) -> mag[b][f][k] (row stride ldm) =
 * 1000 * exp(mel[b][:, f]) . mel_basis[:, k] over the filters' bands, f < mel_lens[b] - 1 (the last frame dropped), 0 beyond. */
int fs2_gl_mel_to_mag(const float* mel, long sb, long sj, long st, const int32_t* mel_lens, const float* mel_basis,
                      const int32_t* span, float* mag, long ldm, int B, int Fmax, int n_mel, int NF, fs2_stream_t stream);
/* stft.py:84-86: G = [mag cos(phase) ; mag sin(phase)] */
int fs2_gl_recombine(const float* mag, long msb, long msf, long msk, const float* phase, long psb, long psf, long psk,
                     const int32_t* frames, float* G, long ldg, int B, int Fmax, int NF, fs2_stream_t stream);
/* audio_processing.py:77-79: forward-DFT rows ft[b*S + f] (Re | Im) -> G = [mag cos(atan2(Im, Re)) ; mag sin(atan2(Im, Re))] */
int fs2_gl_project(const float* ft, long ldft, int S, const float* mag, long msb, long msf, long msk, const int32_t* frames,
                   float* G, long ldg, int B, int Fmax, int NF, fs2_stream_t stream);
/* stft.py:88-120: overlap-add of the inverse GEMM's per-frame segments seg[b*Fmax + f][0, filter) in increasing f, divided by
 * window_sumsquare (win_sq: the squared, centre-padded window, filter_length doubles) where it exceeds tiny(float32), times
 * filter/hop, trimmed by filter/2 at both ends: N_b = hop (frames[b] - 1) samples.  xp (optional): the reflect-padded rows the
 * next forward DFT reads (row_len >= hop (Fmax - 1) + filter; reflected at each utterance's own end, zero beyond);
 * y (optional): the signal rows (ldy >= hop (Fmax - 1); zero beyond N_b). */
int fs2_gl_ola(const float* seg, long lds, const int32_t* frames, const double* win_sq, float* xp, long row_len, float* y,
               long ldy, int B, int Fmax, int filter_length, int hop_length, fs2_stream_t stream);
/* stft.py:74-81: ft rows -> magnitude, phase = atan2(Im, Re), each (B, NF, F) */
int fs2_gl_mag_phase(const float* ft, long ldft, int S, float* mag, float* phase, int B, int F, int NF, fs2_stream_t stream);

/* ---- sample-rate conversion and peak normalisation (reference preprocessor/ljspeech.py:28-34: librosa.load(path, sr), then
 * wav / max|wav| * max_wav_value as int16; specification: fastspeech2_amd/resample.py) ----
 * fs2_resample_poly: rational polyphase resampler over a ragged float32 batch.  Row b of x (row stride ldx) holds in_len[b]
 * samples that start at absolute input index in_begin[b] of its utterance (in_begin == NULL: 0); every other input index counts as
 * zero and nothing beyond in_len[b] is read.  Outputs j in [out_begin[b], out_begin[b] + out_len[b]) (out_begin == NULL: 0) go to
 * y[b][j - out_begin[b]] (row stride ldy), and clamped to [-1, 1] to yc (optional, same stride):
 *     y[j] = sum_{s < T} tab[p][s] * x[q - T + 1 + s],   p = (j down + half) mod up,   q = (j down + half) div up,
 * tab [up][T] the fp64 taps phase-major in ascending input index (T even, 16-byte aligned; fastspeech2_amd.resample.phase_table).
 * fp64 fma in ascending s, one rounding to float32; no atomics; a row's result does not depend on its batch. */
int fs2_resample_poly(const float* x, long ldx, const int32_t* in_begin, const int32_t* in_len, const double* tab, int up,
                      int down, int half, int T, const int32_t* out_begin, const int32_t* out_len, float* y, float* yc, long ldy,
                      int B, int Nin, int Nout, fs2_stream_t stream);
/* peak[b] = max |y[b][0, lens[b])| (0 for an empty row; exact in any order, NaN propagates) */
int fs2_peak_abs(const float* y, long ldy, const int32_t* lens, float* peak, int B, int Nmax, fs2_stream_t stream);
/* pcm[b][n] = (int16)(y[b][n] / peak[b] * max_wav_value): float32 division then product, numpy's astype semantics (truncate toward
 * zero to int32, low 16 bits: a positive peak sample times 32768 becomes -32768, as in the reference).  peak[b] == 0: zeros;
 * [lens[b], Nmax) of a row is zero-filled. */
int fs2_peaknorm_pcm(const float* y, long ldy, const int32_t* lens, const float* peak, float max_wav_value, int16_t* pcm, long ldp,
                     int B, int Nmax, fs2_stream_t stream);

/* ---- programme loudness, ITU-R BS.1770-4 (csrc/fs2_loudness.hip; specification: fastspeech2_amd/loudness.py) ----
 * Ragged float32 rows (B, ldx) with device lens, fp64 after the load, no floating-point atomics: the same input gives the same
 * bytes.  Nothing at or beyond lens[b] is read.
 * fs2_kweight_energy: z[b][i] = mean square of the K-weighted row over block [i h, i h + n), i < n_blocks[b] = (len - n) / h + 1
 * (0 when len < n; z of such a row is not touched).  coef: HOST memory, b0 b1 b2 a1 a2 of the shelf then of the high-pass (a0 = 1).
 * pw: device memory, 8 row-major 4 x 4 matrices, pw[d] = A^(L 2^d) of the cascade's state recursion in transposed direct form II
 * (fastspeech2_amd.loudness.chunk_tables), d = 0 .. 7.  L must equal fs2_kweight_chunk(); L <= h <= L * fs2_kweight_chunks_per_tile(),
 * h <= n.  ws: fs2_kweight_energy_ws(B, Nmax, h) doubles of device workspace (-1: the batch is too large for one call). */
int fs2_kweight_chunk(void);
int fs2_kweight_chunks_per_tile(void);
int fs2_kweight_energy_ws(int B, int Nmax, int h);
int fs2_kweight_energy(const float* x, long ldx, const int32_t* lens, const double* coef, const double* pw, int L, int n, int h,
                       double* z, long ldz, int32_t* n_blocks, double* ws, long ws_doubles, int B, int Nmax, fs2_stream_t stream);
/* out[b][5] = integrated loudness (LKFS), max momentary loudness, n_blocks, blocks above the absolute gate (l_i > -70, l_i = -0.691 +
 * 10 log10 z_i), blocks above both gates (relative: 10 LU below the loudness of the mean of the absolutely gated blocks).  No block:
 * NaN, NaN, 0, 0, 0.  No block above -70: loudness -inf. */
int fs2_gated_loudness(const double* z, long ldz, const int32_t* n_blocks, double* out, int B, int max_blocks, fs2_stream_t stream);
/* g[b] = min(10^((target - loud[b ld_loud]) / 20), 10^(ceiling_db / 20) / peak[b]); flags[b] bit 0: the ceiling bound the gain; bit 1:
 * NaN or infinite loudness, g = 10^(ceiling_db / 20) / peak[b].  peak[b] == 0: g = 0.  target in [-70, 0], ceiling_db <= 0. */
int fs2_loudness_gain(const double* loud, long ld_loud, const float* peak, double target, double ceiling_db, double* g, int32_t* flags,
                      int B, fs2_stream_t stream);
/* pcm[b][k] = (int16)clamp(rint(x[b][k] * g[b] * 32768), -32768, 32767), fp64, round-half-even; saturated[b] = samples the clamp
 * changed; [lens[b], Nmax) of a row is zero-filled. */
int fs2_gain_pcm(const float* x, long ldx, const int32_t* lens, const double* g, int16_t* pcm, long ldp, int32_t* saturated, int B,
                 int Nmax, fs2_stream_t stream);

/* ---- F0: DIO + StoneMask (reference preprocessor/preprocessor.py:182-187; specification: fastspeech2_amd/pitch.py) ----
 * fp64 throughout; rows x[b][0, lens[b]) of a float32 batch (row stride ldx), nothing beyond lens[b] is read; fixed-order reductions,
 * no atomics: a row's F0 does not depend on the rest of its batch.  Frame-major outputs [B][Fmax], frames[b] valid per row.
 * fs2_f0_dc: stats[b] = {mean over N+1 samples (x[N] := 0), event threshold 1e-9 max|x - mean|}. */
int fs2_f0_dc(const float* x, long ldx, const int32_t* lens, double* stats, int B, int Nmax, fs2_stream_t stream);
/* zero-phase 50 Hz low-cut of the DC-free row: lc[b][m + H] for m in [-H, N + H], taps[2R + 1] (ldl >= Nmax + 2H + 1) */
int fs2_f0_lowcut(const float* x, long ldx, const int32_t* lens, const double* stats, const double* taps, int R, double* lc,
                  long ldl, int H, int B, int Nmax, fs2_stream_t stream);
/* per band (nuttall: the nb bands' 4 band_h[j] low-pass taps back to back): band signal -> negative-going, positive-going, peak and
 * dip events.  emit = 0: counts[B][nb][4][ceil(Nmax / 256)] per tile; emit = 1: positions at offs into events[B][nb][4][cap]. */
int fs2_f0_events(const double* lc, long ldl, int H, const int32_t* lens, const double* stats, const double* nuttall,
                  const int32_t* band_h, int nb, int max_h, int32_t* counts, const int32_t* offs, double* events, long cap, int B,
                  int Nmax, int emit, fs2_stream_t stream);
/* exclusive prefix of the tile counts per (row, band, stream) -> offs, totals[B][nb][4] */
int fs2_f0_scan(const int32_t* counts, int32_t* offs, int32_t* totals, int B, int nb, int Nmax, fs2_stream_t stream);
/* per (frame, band): candidate F0 and normalised score cand / score [B][nb][Fmax] from the four event lists */
int fs2_f0_candidates(const double* events, long cap, const int32_t* totals, const int32_t* frames, const double* band_f0,
                      int nb, double fs, double frame_period, double f0_floor, double f0_ceil, double* cand, double* score,
                      int B, int Fmax, fs2_stream_t stream);
/* best band per frame and contour fixing steps 1-4 (vrm: voice range minimum in frames; tmp [B][2][Fmax]) -> f0 [B][Fmax] */
int fs2_f0_fix(const double* cand, const double* score, const int32_t* frames, int nb, int vrm, double allowed_range,
               double* tmp, double* f0, int B, int Fmax, fs2_stream_t stream);
/* StoneMask refinement of f0 [B][Fmax] at t = f frame_period / 1000 from the DC-intact rows -> out (may alias f0) */
int fs2_f0_stonemask(const float* x, long ldx, const int32_t* lens, const double* f0, const int32_t* frames, double fs,
                     double frame_period, double* out, int B, int Fmax, int Nmax, fs2_stream_t stream);

/* ---- F0: probabilistic YIN (Mauch & Dixon 2014; specification: fastspeech2_amd/pyin.py) ----
 * fp64 throughout, the same ragged float32 rows as above; three stages, each taking the previous one's output, fixed-order sums,
 * no atomics.  Frame f of row b is centred at sample f hop and spans frame_length samples (zero outside [0, lens[b])); every output
 * row at f >= frames[b] is written as 0.
 * fs2_pyin_cmnd: cumulative-mean-normalised difference d'[B][Fmax][tmax + 1], integration window frame_length / 2, direct form
 * (tmax <= frame_length / 2 - 1). */
int fs2_pyin_cmnd(const float* x, long ldx, const int32_t* lens, const int32_t* frames, int hop, int frame_length, int tmax,
                  double* dprime, int B, int Fmax, int Nmax, fs2_stream_t stream);
/* troughs of d' on [tmin, tmax], the nthr threshold weights beta[k] (threshold (k + 1) / nthr) -> obs[B][Fmax][2 nb]: nb voiced pitch
 * bins (bin = round(bins_per_octave log2(f / fmin))), then nb equal unvoiced entries (1 - pv) / nb; pv[B][Fmax] = min(sum, 1) */
int fs2_pyin_observe(const double* dprime, const int32_t* frames, int tmin, int tmax, const double* beta, int nthr,
                     double no_trough_prob, double fs, double fmin, int bins_per_octave, int nb, double* obs, double* pv,
                     int B, int Fmax, fs2_stream_t stream);
/* Viterbi over the 2 nb states (state = v nb + bin, v = 0 voiced): logw[2 half_width + 1] the band's log weights, logz[nb] the log of
 * each source bin's in-range weight sum; backptr [B][Fmax][2 nb] bytes of workspace ((offset, flip) in one byte: 2 (2 half_width + 1)
 * above 255 is FS2_EINVAL) -> states[B][Fmax], f0[B][Fmax] = fmin 2^(bin / bins_per_octave) or 0 */
int fs2_pyin_viterbi(const double* obs, const int32_t* frames, int nb, int half_width, const double* logw, const double* logz,
                     double switch_prob, double fmin, int bins_per_octave, uint8_t* backptr, int32_t* states, double* f0,
                     int B, int Fmax, fs2_stream_t stream);

/* ---- forced alignment: monophone HMM, Baum-Welch + Viterbi (specification: fastspeech2_amd/align.py) ----
 * fp64 throughout, ragged batches: utterance b has lens[b] frames and jlens[b] states (both int32, device); buffers are
 * [B][Tmax][Jmax] with explicit batch / frame strides in elements, graph rows sid / skip / block are [B][Jmax] int32 with row stride
 * ldg.  Nothing at t >= lens[b] or j >= jlens[b] is read or written.  alt[b] = {alternative start state or -1, alternative end state
 * or -1}: a path starts in state 0 or alt[b][0] and ends in state jlens[b] - 1 or alt[b][1].  No atomics: results do not depend on
 * the rest of the batch or on the run.  Jmax above fs2_align_max_states() is FS2_EINVAL. */
int fs2_align_max_states(void);
/* log-mel [B][n_mel][frames] f32 (strides ldm_b, ldm_c) -> x [B][Tmax][2 n_mel]: per-utterance mean removed, then the central
 * differences (x[t+1] - x[t-1]) / 2 with edge replication appended; mean [B][n_mel] is workspace */
int fs2_align_feats(const float* mel, long ldm_b, long ldm_c, const int32_t* lens, double* mean, double* x, long ldx_b, long ldx_t,
                    int B, int n_mel, int Tmax, fs2_stream_t stream);
/* E[b][t][j] = -1/2 sum_d ((x_d - mu_d)^2 / var_d + log(2 pi var_d)) for class sid[b][j] of the [n_classes][D] tables mu, var */
int fs2_align_emit(const double* x, long ldx_b, long ldx_t, const int32_t* lens, const int32_t* jlens, const int32_t* sid, long ldg,
                   const double* mu, const double* var, int n_classes, int D, double* E, long lde_b, long lde_t, int B, int Tmax,
                   int Jmax, fs2_stream_t stream);
/* Mixture emissions: component m of class c is row c * M + m of w [n_classes * M], mu and var [n_classes * M][D], 1 <= M <=
 * fs2_align_max_mixtures() (8; more is FS2_EINVAL before any launch).  N_m = log w_m - 1/2 sum_d (...), log 0 = -inf;
 * E[b][t][j] = mx + log(sum_m exp(N_m - mx)), mx = max_m N_m, over ascending m; resp[b][t][j][m] = exp(N_m - E) (strides ldr_b,
 * ldr_t, ldr_j, m contiguous) unless resp is NULL.  With M = 1 and w = 1, E has the bits fs2_align_emit writes. */
int fs2_align_max_mixtures(void);
int fs2_align_emit_gmm(const double* x, long ldx_b, long ldx_t, const int32_t* lens, const int32_t* jlens, const int32_t* sid, long ldg,
                       const double* w, const double* mu, const double* var, int n_classes, int M, int D, double* E, long lde_b,
                       long lde_t, double* resp, long ldr_b, long ldr_t, long ldr_j, int B, int Tmax, int Jmax, fs2_stream_t stream);
/* log-domain forward recursion over the arcs self, next (j - 1) and skip[b][j] -> alpha, loglik[b] over the end states */
int fs2_align_forward(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                      long ldg, const int32_t* alt, double* alpha, long lda_b, long lda_t, double* loglik, int B, int Tmax, int Jmax,
                      fs2_stream_t stream);
/* backward recursion (beta stays on the chip) -> gamma = exp(alpha + beta - loglik); gamma may be alpha itself (equal strides) */
int fs2_align_backward(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                       long ldg, const int32_t* alt, const double* alpha, long lda_b, long lda_t, const double* loglik, double* gamma,
                       long ldo_b, long ldo_t, int B, int Tmax, int Jmax, fs2_stream_t stream);
/* partials[b][j] = sum_t gamma[b][t][j] * {1, x[b][t][0..D), x[b][t][0..D)^2} (1 + 2 D columns, strides ldp_b, ldp_j), ascending t */
int fs2_align_stats(const double* gamma, long ldo_b, long ldo_t, const double* x, long ldx_b, long ldx_t, const int32_t* lens,
                    const int32_t* jlens, int D, double* partials, long ldp_b, long ldp_j, int B, int Tmax, int Jmax,
                    fs2_stream_t stream);
/* partials[b][j * M + m] = sum_t gamma[b][t][j] * resp[b][t][j][m] * {1, x, x^2} (row stride ldp_r), ascending t; the product of
 * gamma and resp is formed on the chip.  Jmax * M may reach 8192. */
int fs2_align_stats_gmm(const double* gamma, long ldo_b, long ldo_t, const double* resp, long ldr_b, long ldr_t, long ldr_j,
                        const double* x, long ldx_b, long ldx_t, const int32_t* lens, const int32_t* jlens, int M, int D,
                        double* partials, long ldp_b, long ldp_r, int B, int Tmax, int Jmax, fs2_stream_t stream);
/* sums[c][0..cols) = (accumulate ? sums[c] : 0) + the rows items[offs[c] .. offs[c + 1]) of partials (as [n_rows][ldp_j]), in list order */
int fs2_align_reduce(const double* partials, long ldp_j, long n_rows, const int32_t* offs, const int32_t* items, int n_classes,
                     int cols, double* sums, int accumulate, fs2_stream_t stream);
/* Viterbi: bp[b][t][j] = 0 self / 1 next / 2 skip (lowest code on ties, row 0 is 0), end[b] = best end state (lower index on ties),
 * score[b] its log-probability */
int fs2_align_viterbi(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                      long ldg, const int32_t* alt, uint8_t* bp, long ldp_b, long ldp_t, int32_t* end, double* score, int B, int Tmax,
                      int Jmax, fs2_stream_t stream);
/* The three scans with a cost on every arc (the "Transitions" paragraph of fastspeech2_amd/align.py).  w [B][3][ldw], ldw >= Jmax:
 * w[b][0][j] the self arc of state j, w[b][1][j] the arc j - 1 -> j, w[b][2][j] the arc skip[b][j] -> j; edge [B][4]: start in state 0,
 * start in alt[b][0], end in state jlens[b] - 1, end in alt[b][1].  All costs are finite log-probabilities; nothing of w at
 * j >= jlens[b] is read.  A null w or edge and ldw < Jmax are FS2_EINVAL before any launch; every other argument is checked as in the
 * scan without costs.  With all costs 0 each returns the bits of that scan.  Nothing of this has been timed.
 *   forward:   alpha[0][j] = edge + E[0][j] at the start states; alpha[t][j] = E[t][j] + lse(alpha[t-1][j] + w[0][j],
 *              alpha[t-1][j-1] + w[1][j], alpha[t-1][skip j] + w[2][j]); loglik = lse over the end states e of alpha[T-1][e] + edge(e)
 *   backward:  beta[T-1][e] = edge(e), every successor arc adds its cost; gamma as fs2_align_backward (it may be alpha itself);
 *              xi [B][Jmax][5] (strides ldx_b >= Jmax ldx_j, ldx_j >= 5): xi[b][j][a] = sum over t = T-1 .. 1, in that order, of
 *              exp(alpha[t-1][pred_a(j)] + w[a][j] + E[t][j] + beta[t][j] - loglik) for a = 0 self, 1 next, 2 skip;
 *              xi[b][j][3] = gamma[0][j], xi[b][j][4] = gamma[T-1][j]; nothing at j >= jlens[b] is written
 *   viterbi:   the same costs inside the max, the same tie rules; score includes the end edge */
int fs2_align_forward_arcs(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                           long ldg, const int32_t* alt, const double* w, long ldw, const double* edge, double* alpha, long lda_b,
                           long lda_t, double* loglik, int B, int Tmax, int Jmax, fs2_stream_t stream);
int fs2_align_backward_arcs(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                            long ldg, const int32_t* alt, const double* w, long ldw, const double* edge, const double* alpha,
                            long lda_b, long lda_t, const double* loglik, double* gamma, long ldo_b, long ldo_t, double* xi,
                            long ldx_b, long ldx_j, int B, int Tmax, int Jmax, fs2_stream_t stream);
int fs2_align_viterbi_arcs(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                           long ldg, const int32_t* alt, const double* w, long ldw, const double* edge, uint8_t* bp, long ldp_b,
                           long ldp_t, int32_t* end, double* score, int B, int Tmax, int Jmax, fs2_stream_t stream);
/* frames[b][k] = frames the best path spends in block k (block[b][j] = block of state j), zero-filled up to nbmax */
int fs2_align_backtrack(const uint8_t* bp, long ldp_b, long ldp_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                        const int32_t* block, long ldg, const int32_t* end, int32_t* frames, int nbmax, int B, int Tmax, int Jmax,
                        fs2_stream_t stream);
/* Alignment confidence (csrc/fs2_align_score.hip; specification: the "Confidence" paragraph of fastspeech2_amd/align.py).  No atomics.
 * The walk of fs2_align_backtrack kept per frame: state[b][t] = the state of the best path at frame t, cls[b][t] = sid[b][state]
 * (int32 [B][Tmax], batch strides lds_b, ldc_b >= Tmax).  A chain that leaves [0, jlens[b]) stops: the frames before it get -1 in
 * both.  Nothing at t >= lens[b] is written. */
int fs2_align_path(const uint8_t* bp, long ldp_b, long ldp_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                   const int32_t* sid, long ldg, const int32_t* end, int32_t* state, long lds_b, int32_t* cls, long ldc_b, int B,
                   int Tmax, int Jmax, fs2_stream_t stream);
/* doubles of workspace fs2_align_frame_scores needs: n_classes M (D + 1) (0 for tables outside its limits) */
int fs2_align_frame_scores_ws(int n_classes, int M, int D);
/* Every frame of f [B][Tmax][D] (strides ldf_b >= Tmax ldf_t, ldf_t >= D) against every class of the tables w [n_classes * M], mu,
 * var [n_classes * M][D] (fs2_align_emit_gmm's layout; with M = 1 the caller passes w = 1):  F[t][c] = mx + log(sum_m exp(N_m - mx)),
 * N_m = log w_m - 1/2 sum_d ((f_d - mu_d)^2 (1 / var_d) + log(2 pi var_d)), d and m ascending, the frame-independent terms taken
 * once per call into ws.  own[b][t] = F[t][cls[b][t]] (NaN when cls[b][t] is outside [0, n_classes); nothing outside the tables is
 * read), best[b][t] = max_c F[t][c], arg[b][t] = the lowest c that attains it; own <= best, and own == best bit for bit where
 * arg == cls.  own, best (double) and arg, cls (int32) are [B][Tmax] with their own batch strides >= Tmax.  Nothing at t >=
 * lens[b] is read or written.  FS2_EINVAL before any launch: M outside 1..fs2_align_max_mixtures(), D <= 0, n_classes <= 0,
 * n_classes M (D + 1) >= 2^31, B > 65535, a bad stride, ws_doubles below fs2_align_frame_scores_ws(). */
int fs2_align_frame_scores(const double* f, long ldf_b, long ldf_t, const int32_t* lens, const int32_t* cls, long ldc_b,
                           const double* w, const double* mu, const double* var, int n_classes, int M, int D, double* ws,
                           long ws_doubles, double* own, long ldo_b, double* best, long ldb_b, int32_t* arg, long lda_b, int B,
                           int Tmax, fs2_stream_t stream);
/* Segmental scores (csrc/fs2_align_seg.hip; specification: the "Segmental scores" paragraph of fastspeech2_amd/align.py).  No atomics.
 * The largest number of candidate phones P (256), and the doubles of workspace fs2_align_segment_scores needs: n_classes M (D + 1)
 * (0 for tables outside the limits of fs2_align_frame_scores). */
int fs2_align_max_seg_phones(void);
int fs2_align_segment_scores_ws(int n_classes, int M, int D);
/* For every block k < Kmax of every utterance: seg[b][k] = (start, frames) (int32, batch stride lds_b >= 2 Kmax) is a run of frames
 * of f (as for fs2_align_frame_scores), cand[b][k][q S + s] (int32, strides ldc_b >= Kmax ldc_k, ldc_k >= P S) the class of state s
 * of candidate phone q < P, arc[c] = (ws, wn) the log-probabilities of staying in and of leaving class c ([n_classes][2]).  With
 * F[t][c] of fs2_align_frame_scores (the same preparation into ws, the same statements per frame, class and component):
 * v_0(start) = F[start][c_0], v_s(start) = -inf for s > 0; v_s(t) = F[t][c_s] + max(v_s(t-1) + ws[c_s], v_{s-1}(t-1) + wn[c_{s-1}]);
 * V[b][k][q] = v_{S-1}(start + frames - 1) + wn[c_{S-1}], -inf when frames < S (double, strides ldv_b >= Kmax ldv_k, ldv_k >= P).
 * Two phones with identical table rows get identical bits.  A block with frames <= 0, start < 0, start + frames > lens[b] or a
 * negative entry among its P S candidates is absent: its V row is not written and nothing is read for it.  A candidate class
 * >= n_classes scores -inf and the tables are not read for it.  FS2_EINVAL before any launch: P outside
 * 1..fs2_align_max_seg_phones(), S outside 1..3, M outside 1..fs2_align_max_mixtures(), D <= 0, n_classes <= 0, n_classes M (D + 1) >=
 * 2^31, B > 65535, a bad stride, a null pointer, ws_doubles below fs2_align_segment_scores_ws(). */
int fs2_align_segment_scores(const double* f, long ldf_b, long ldf_t, const int32_t* lens, const int32_t* seg, long lds_b,
                             const int32_t* cand, long ldc_b, long ldc_k, const double* w, const double* mu, const double* var,
                             int n_classes, int M, int D, const double* arc, double* ws, long ws_doubles, double* V, long ldv_b,
                             long ldv_k, int B, int Tmax, int Kmax, int P, int S, fs2_stream_t stream);
/* Phone-loop recognition (csrc/fs2_align_loop.hip; specification: fastspeech2_amd/recognize.py).  No atomics.  P phones of S states,
 * state j = p S + s is emission class j, C = P S; E [B][Tmax][>= C] from fs2_align_emit / fs2_align_emit_gmm with sid = 0 .. C - 1.
 * Costs, fp64, finite or -inf: self_[C]; next_[C], the arc s - 1 -> s (unused at s = 0); link[p][q] (row stride ldl >= P), leave the
 * last state of p and enter the first state of q; init[P]; final_[P].  The largest P (253: the backpointer is one byte). */
int fs2_align_max_loop_phones(void);
/* d[0][q S] = init[q] + E[0][q S], every other state -inf;  d[t][j] = E[t][j] + the maximum over, in code order, 0: d[t-1][j] +
 * self_[j]; for s > 0, 1: d[t-1][j-1] + next_[j]; for s = 0, 2 + p: d[t-1][p S + S - 1] + link[p][q], p ascending; a later candidate
 * replaces an earlier one only when strictly larger.  bp[b][t][j] (bytes, strides ldp_b >= Tmax ldp_t, ldp_t >= C) is the winning
 * code, row 0 is 0.  end[b] = the state p S + S - 1 of the largest d[T-1][p S + S - 1] + final_[p], p ascending, strictly larger
 * replaces; score[b] that value; end = -1 and score = -inf when it is -inf or lens[b] = 0.  Only adds and compares: exact.
 * Nothing at t >= lens[b] is read or written.  FS2_EINVAL before any launch: P outside 1..fs2_align_max_loop_phones(), S outside
 * 1..3, P S above fs2_align_max_states(), a bad stride, a null pointer. */
int fs2_align_loop_viterbi(const double* E, long lde_b, long lde_t, const int32_t* lens, const double* self_, const double* next_,
                           const double* link, long ldl, const double* init, const double* final_, uint8_t* bp, long ldp_b,
                           long ldp_t, int32_t* end, double* score, int B, int Tmax, int P, int S, fs2_stream_t stream);
/* The segments of the best path in time order: seg_phone[b][k] the phone, seg_start[b][k] the first frame (int32, row stride lds_b >=
 * Tmax), n_seg[b] <= lens[b] of them; 0 when end[b] < 0 or lens[b] = 0.  A chain that leaves the table stops: n_seg = -1 and no
 * segment is written.  Nothing at k >= n_seg[b] is written. */
int fs2_align_loop_backtrack(const uint8_t* bp, long ldp_b, long ldp_t, const int32_t* lens, const int32_t* end, int32_t* seg_phone,
                             int32_t* seg_start, long lds_b, int32_t* n_seg, int B, int Tmax, int P, int S, fs2_stream_t stream);
/* The LDA stage (csrc/fs2_align_lda.hip).  Spliced frames y [B][Tmax][D_s], D_s = n_mel (2 c + 1), strides ldy_b >= Tmax ldy_t,
 * ldy_t >= D_s, in elements.  Limits, all FS2_EINVAL before any launch: 0 <= c <= 4, 1 <= k <= D_s <= fs2_align_max_splice_dim() (720).
 * Nothing at t >= lens[b] is read or written.  No atomics. */
int fs2_align_max_splice_dim(void);
/* y[b][t][(p + c) n_mel + m] = x[b][min(max(t + p, 0), lens[b] - 1)][m], p = -c..c, m < n_mel: the first n_mel columns of x
 * (ldx_t >= n_mel, ldx_b >= Tmax ldx_t), clamped at the utterance's own ends */
int fs2_align_splice(const double* x, long ldx_b, long ldx_t, const int32_t* lens, int n_mel, int c, double* y, long ldy_b, long ldy_t,
                     int B, int Tmax, fs2_stream_t stream);
/* doubles of workspace fs2_align_scatter needs for a batch of this shape (0 for an empty batch or Ds outside 1..720); at most
 * 32 (78 * 4096 + 768) */
int fs2_align_scatter_ws(int B, int Tmax, int Ds);
/* s[0..Ds) += sum y, S[Ds][Ds] (row stride lds >= Ds) += sum y y^T over the valid frames of the batch; the caller zeroes both before
 * the first batch.  The padded rows b Tmax + t are cut into at most 32 chunks whose length depends on (B, Tmax) only; the lower
 * triangle's 64 x 64 tiles are summed per chunk with v_mfma_f64_16x16x4_f64 in ascending t into ws, added in ascending chunk order,
 * added to S and mirrored: S[i][j] and S[j][i] hold the same bits.  ws_doubles below fs2_align_scatter_ws() is FS2_EINVAL. */
int fs2_align_scatter(const double* y, long ldy_b, long ldy_t, const int32_t* lens, int Ds, double* s, double* S, long lds, double* ws,
                      long ws_doubles, int B, int Tmax, fs2_stream_t stream);
/* z[b][t][q] = sum_d P[q][d] y[b][t][d] - o[q], q < K: P [K][Ds] contiguous, o [K], z strides ldz_b >= Tmax ldz_t, ldz_t >= K; the
 * sum ascends in d (v_mfma_f64_16x16x4_f64, four d per step) */
int fs2_align_project(const double* y, long ldy_b, long ldy_t, const int32_t* lens, const double* P, const double* o, int K, int Ds,
                      double* z, long ldz_b, long ldz_t, int B, int Tmax, fs2_stream_t stream);
/* Speaker adaptation, constrained MLLR (csrc/fs2_align_fmllr.hip; specification: the "fMLLR" paragraph of fastspeech2_amd/align.py).
 * f, c, h, out [B][Tmax][D] with strides ld*_b >= Tmax ld*_t, ld*_t >= D, in elements; xi = (f, 1) has D + 1 entries.  Limit,
 * FS2_EINVAL before any launch: 1 <= D <= fs2_align_max_fmllr_dim() (64).  Nothing at t >= lens[b] or j >= jlens[b] is read or
 * written.  No atomics.  Nothing of this has been timed. */
int fs2_align_max_fmllr_dim(void);
/* c[b][t][i] = sum_j gamma[b][t][j] / var[sid[b][j]][i], h[b][t][i] = sum_j gamma[b][t][j] mu[sid[b][j]][i] / var[sid[b][j]][i], j
 * ascending; gamma [B][Tmax][Jmax] (ldg_t >= Jmax), sid [B][ldsid] as for fs2_align_emit, mu and var [n_classes][D] contiguous;
 * c and h share their strides */
int fs2_align_fmllr_weights(const double* gamma, long ldg_b, long ldg_t, const int32_t* lens, const int32_t* jlens, const int32_t* sid,
                            long ldsid, const double* mu, const double* var, int n_classes, int D, double* c, double* h, long ldc_b,
                            long ldc_t, int B, int Tmax, int Jmax, fs2_stream_t stream);
/* doubles of workspace fs2_align_fmllr_accum needs for a batch of this shape (0 for an empty batch or D outside 1..64):
 * 64 D (D + 1)(D + 2) for the partial tables and 2 B + 130 for the list of chunks */
int fs2_align_fmllr_accum_ws(int B, int Tmax, int D);
/* For every speaker s with rows in the CSR (offs [n_spk + 1], rows [offs[n_spk]], int32 on the device: the utterances b of speaker
 * s are rows[offs[s] .. offs[s + 1]), every b at most once):  beta[s] += frames,  G[s][i] += sum_t c[b][t][i] xi xi^T
 * ([n_spk][D][D + 1][D + 1] contiguous),  k[s][i] += sum_t h[b][t][i] xi ([n_spk][D][D + 1]), over the speaker's utterances in list
 * order, t ascending; the caller zeroes the tables before the first batch, the tables of a speaker without rows are not touched.
 * The speaker's padded rows are cut into chunks whose length depends on (B, Tmax) only; the lower triangle's 16 x 16 tiles are summed
 * per chunk with v_mfma_f64_16x16x4_f64 in ascending t, the chunks are added in ascending order, the total is added to G and
 * mirrored: G[s][i][p][q] and G[s][i][q][p] hold the same bits.  ws_doubles below fs2_align_fmllr_accum_ws() is FS2_EINVAL. */
int fs2_align_fmllr_accum(const double* f, long ldf_b, long ldf_t, const double* c, const double* h, long ldc_b, long ldc_t,
                          const int32_t* lens, const int32_t* offs, const int32_t* rows, int n_spk, int D, double* beta, double* G,
                          double* k, double* ws, long ws_doubles, int B, int Tmax, fs2_stream_t stream);
/* out[b][t][r] = sum_p W[spk[b]][r][p] f[b][t][p] + W[spk[b]][r][D], p ascending: W [n_spk][D][D + 1] contiguous, spk [B] int32 on
 * the device, every entry in [0, n_spk) (an utterance whose entry is not is left unwritten) */
int fs2_align_fmllr_apply(const double* f, long ldf_b, long ldf_t, const int32_t* lens, const double* W, const int32_t* spk, int n_spk,
                          int D, double* out, long ldo_b, long ldo_t, int B, int Tmax, fs2_stream_t stream);
/* The triphone tree (csrc/fs2_align_tree.hip; specification: the "Triphones" paragraph of fastspeech2_amd/align.py).  The item table
 * sums [n_items][lds >= 1 + 2 D] holds {n, a[0..D), q[0..D)} per row, left / right [n_items] int32 the context symbols, member
 * [n_sets][n_symbols] uint8 the question sets: question qi < n_sets asks whether left[item] is in set qi, question n_sets + qi
 * whether right[item] is.  Limits, FS2_EINVAL before any launch: 1 <= n_sets <= fs2_align_max_tree_sets() (1024), min_occ >= 1.
 * No atomics.  Nothing of this has been timed. */
int fs2_align_max_tree_sets(void);
/* For node m < n_nodes, the items items[offs[m] .. offs[m + 1]) of the list of n_list entries (an entry outside [0, n_items) is
 * skipped, a symbol outside [0, n_symbols) answers no; rows of the table that are not listed are not read): per question the pooled
 * sums of the items that answer yes and of those that answer no, both accumulated with v_mfma_f64_16x16x4_f64 (the item is the k
 * index, ascending in steps of four), the likelihoods L = -n / 2 sum_d (log(2 pi max(q_d / n - (a_d / n)^2, floor[d])) + 1), d
 * ascending, and gain = (L(yes) + L(no)) - L(node), -inf unless both sides have n >= min_occ.  best_q[m] = the question of the
 * largest gain (the lowest on ties, -1 when none is eligible), best_gain[m] that gain.  gains and n_yes, each [n_nodes][ldq >=
 * 2 n_sets] or NULL, receive the whole tables.  Every sum's order depends on the node's item count and D alone. */
int fs2_align_tree_gains(const double* sums, long lds, int n_items, const int32_t* left, const int32_t* right, const int32_t* offs,
                         const int32_t* items, int n_list, int n_nodes, const uint8_t* member, int n_sets, int n_symbols,
                         const double* floor, int D, double min_occ, int32_t* best_q, double* best_gain, double* gains, double* n_yes,
                         long ldq, fs2_stream_t stream);

/* ---- objective scoring: cepstra, dynamic time warping, F0 along the path (specification: fastspeech2_amd/metrics.py) ----
 * fp64 throughout, ragged batches of pairs: pair p has alens[p] reference frames (index i) and blens[p] synthesized frames (index j),
 * int32 on the device, both at most fs2_dtw_max_frames() (T1max / T2max above it are FS2_EINVAL).  Cepstra are [B][Tmax][K] with
 * batch / frame strides in elements.  Local costs (f64) and backpointers (bytes) of a pair are stored skewed: cell (i, j) is at row
 * (i + j) mod blens[p], column i of a [T2max][>= T1max] matrix (row stride ld*_s >= T1max, pair stride ld*_b >= T2max ld*_s), so an
 * anti-diagonal is contiguous in i.  Nothing at i >= alens[p] or a row >= blens[p] is read or written.  No atomics. */
int fs2_dtw_max_frames(void);
/* log-mel [B][n_mel][frames] f32 (strides ldm_b, ldm_c) -> c[b][t][k] = sum_m mel[b][m][t] table[k][m] in ascending m, k < K <= 40;
 * table [K][n_mel] f64 (n_mel <= 128) is the caller's DCT rows: no cosine is evaluated on the device */
int fs2_mcep(const float* mel, long ldm_b, long ldm_c, const int32_t* lens, const double* table, int K, double* c, long ldc_b,
             long ldc_t, int B, int n_mel, int Tmax, fs2_stream_t stream);
/* d(i, j) = sqrt(sum_k (a[p][i][k] - b[p][j][k])^2), k ascending, unfused, correctly rounded root; skewed */
int fs2_dtw_cost(const double* a, long lda_b, long lda_t, const int32_t* alens, const double* b, long ldb_b, long ldb_t,
                 const int32_t* blens, int K, double* cost, long ldd_b, long ldd_s, int B, int T1max, int T2max, fs2_stream_t stream);
/* D(0,0) = d(0,0), D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)); bp = 0 / 1 / 2 in that order, lowest code on ties, skewed
 * like cost; total[p] = D(alens[p] - 1, blens[p] - 1).  D itself is never stored. */
int fs2_dtw_scan(const double* cost, long ldd_b, long ldd_s, const int32_t* alens, const int32_t* blens, uint8_t* bp, long ldp_b,
                 long ldp_s, double* total, int B, int T1max, int T2max, fs2_stream_t stream);
/* the path from (0, 0) to (alens[p] - 1, blens[p] - 1): pi / pj [B][ldq] int32 (ldq >= T1max + T2max - 1), plen[p] = P cells;
 * entries [P, alens[p] + blens[p] - 1) are set to -1, later ones are left alone */
int fs2_dtw_backtrack(const uint8_t* bp, long ldp_b, long ldp_s, const int32_t* alens, const int32_t* blens, int32_t* pi, int32_t* pj,
                      long ldq, int32_t* plen, int B, int T1max, int T2max, fs2_stream_t stream);
/* sums[p][0..3) = {cells where exactly one of r = f0_ref[p][pi], s = f0_syn[p][pj] is 0, cells with r > 0 and s > 0, the sum over
 * those of (1200 log2(s / r))^2}, in a fixed order of additions */
int fs2_dtw_f0(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* f0_ref, long ldr,
               const double* f0_syn, long lds, const int32_t* alens, const int32_t* blens, double* sums, long ldo, int B, int T1max,
               int T2max, fs2_stream_t stream);
/* prosody along the path, with e_ref / e_syn [B][lde*] the float32 frame energies and V the cells with r > 0 and s > 0:
 * sums[p][0..8) = {cells of V with fabs(s - r) > 0.2 r, |V|, cells where exactly one of r, s is 0, Sxx, Syy, Sxy of x = ln r and
 * y = ln s over V about their means (mean first, then a second pass), sum |e_ref - e_syn|, sum e_ref}; ldo >= 8 */
int fs2_dtw_prosody(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* f0_ref, long ldr,
                    const double* f0_syn, long lds, const float* e_ref, long lder, const float* e_syn, long ldes, const int32_t* alens,
                    const int32_t* blens, double* sums, long ldo, int B, int T1max, int T2max, fs2_stream_t stream);
/* the voiced frames (f0 > 0) among the first lens[b] <= Tmax <= fs2_dtw_max_frames() of row b, in order, to out[b][0 .. nv[b]) (the
 * rest of the row is left alone; out must not be f0), and stats[b][0..5) = {nv, mean, M2, M3, M4}, the central sums of those values
 * about their mean in a second pass; all zero when nv[b] = 0.  Strides in elements: ldf, ldo >= Tmax, lds >= 5 */
int fs2_prosody_voiced(const double* f0, long ldf, const int32_t* lens, double* out, long ldo, int32_t* nv, double* stats, long lds,
                       int B, int Tmax, fs2_stream_t stream);

/* ---- over-smoothing: global variance and modulation spectrum (csrc/fs2_modspec.hip; specification: fastspeech2_amd/modspec.py) ----
 * Trajectories c [B][Tmax][K] f64 with batch / frame strides in elements (ldc_t >= K, ldc_b >= Tmax ldc_t) and unit stride in k; row
 * b has lens[b] frames (int32, device), 1 <= Tmax <= fs2_dtw_max_frames(), 1 <= K <= 128.  Nothing at a frame >= lens[b] is read; a
 * row with lens[b] < 1 is left alone.  fp64, no atomics; every sum runs in ascending order in one thread with its rounding errors
 * carried in a second word: the same input gives the same bytes.
 * fs2_modspec_nfft: the transform length N = 4096, twice the frame bound. */
int fs2_modspec_nfft(void);
/* mom[b][k][0..2) = {mean = (sum_t c) / T, M2 = sum_t (c - mean)^2 in a second pass}; strides ldm_k >= 2, ldm_b >= K ldm_k */
int fs2_traj_moments(const double* c, long ldc_b, long ldc_t, const int32_t* lens, double* mom, long ldm_b, long ldm_k, int B, int Tmax,
                     int K, fs2_stream_t stream);
/* With x[t] = c[b][t][k] - mean[b][k] (mean: any strides ldm_b, ldm_k, so the mom of fs2_traj_moments serves), X[f] = sum_t x[t]
 * (cos - i sin)(2 pi ((f t) mod N) / N) against twiddle [N][2] = {cos, sin}(2 pi j / N), the caller's device table (no sine is
 * evaluated here), and ms[f] = ln(|X[f]|^2 / T + floor), f = 0 .. N / 2: bands[b][k][j] = (10 / ln 10) times the mean of ms over the
 * bins [bins[2 j], bins[2 j + 1]), j < n_bands (strides ldo_k >= n_bands, ldo_b >= K ldo_k), and, when logms is not NULL,
 * logms[b][k][f] = ms[f] (strides ldl_k >= N / 2 + 1, ldl_b >= K ldl_k).  bins: HOST memory, 1 <= n_bands <= 16 non-empty, ascending,
 * disjoint ranges within [0, N / 2 + 1); floor > 0; B <= 65535.  Nothing beyond those counts is written. */
int fs2_modspec(const double* c, long ldc_b, long ldc_t, const int32_t* lens, const double* mean, long ldm_b, long ldm_k,
                const double* twiddle, const int32_t* bins, int n_bands, double floor_, double* bands, long ldo_b, long ldo_k,
                double* logms, long ldl_b, long ldl_k, int B, int Tmax, int K, fs2_stream_t stream);

/* ---- modulation-spectrum postfilter (csrc/fs2_msfilter.hip; specification: fastspeech2_amd/postfilter.py) ----
 * fs2_ms_stats_update: folds the rows b = 0 .. B - 1 of logms [B][K][N / 2 + 1] (what fs2_modspec writes; strides ldl_k >= N / 2 + 1,
 * ldl_b >= K ldl_k) whose keep[b] (int32, device) is not 0 into state[k][f][0..2) = {mean, M2} (stride lds_k >= 2 (N / 2 + 1)), in
 * ascending b with Welford's update; n_before is the number of rows folded into state so far (0: state is not read).  One thread per
 * (k, f), no atomics: the same input gives the same bytes. */
int fs2_ms_stats_update(const double* logms, long ldl_b, long ldl_k, const int32_t* keep, double* state, long lds_k, long n_before,
                        int B, int K, fs2_stream_t stream);
/* The postfilter on trajectories c [B][Tmax][K], float32 (is_f64 = 0) or float64 (is_f64 = 1), strides in elements as fs2_modspec
 * takes them, into y of the same type (ldy_t >= K, ldy_b >= Tmax ldy_t; y must not overlap c).  With x = c - mean, X and ms[f] as
 * fs2_modspec defines them and the rows k of the tables mu_n, sd_n, mu_g, sd_g [K][N / 2 + 1] f64 (stride lds_k >= N / 2 + 1):
 * r = sd_n / sd_g (1 where sd_g is not above 0), ln g[f] = 0.5 k_emph (r (ms - mu_g) + mu_n - ms) clamped to +- max_gain_db
 * (ln 10) / 20, g[0] = 1, y[t] = mean + (1 / N)(X[0] + 2 sum_{0 < f < N / 2} Re(g X e^{+2 pi i f t / N}) + g X[N / 2] (-1)^t), t < lens[b].
 * fp64 arithmetic whatever the type.  A row with lens[b] < min_frames is copied to y; a row with lens[b] < 1 is left alone; nothing
 * at a frame >= lens[b] or a coefficient >= K is read or written.  0 <= k_emph <= 1, floor > 0, 0 <= max_gain_db <= 200,
 * min_frames >= 1, 1 <= Tmax <= fs2_dtw_max_frames(), 1 <= K <= 128, B <= 65535. */
int fs2_ms_filter(const void* c, long ldc_b, long ldc_t, const int32_t* lens, const double* mean, long ldm_b, long ldm_k,
                  const double* twiddle, const double* mu_n, const double* sd_n, const double* mu_g, const double* sd_g, long lds_k,
                  double k_emph, double floor_, double max_gain_db, int min_frames, void* y, long ldy_b, long ldy_t, int is_f64, int B,
                  int Tmax, int K, fs2_stream_t stream);

/* ---- wavelet prosody scores (csrc/fs2_cwt.hip; specification: fastspeech2_amd/cwt.py) ----
 * Ragged batches of f64 rows; row b has lens[b] frames (int32, device), 1 <= Tmax <= fs2_dtw_max_frames().  Nothing at a frame >=
 * lens[b] is read or written; a row with lens[b] < 1 is left alone.  No atomics; every sum carries its rounding errors in a second
 * word, per lane in ascending order and then by a fixed tree: the same input gives the same bytes, whatever rows are beside it.
 * fs2_cwt_scales: the number of scales, 10. */
int fs2_cwt_scales(void);
/* The normalised continuous ln F0 of the tracks f0 [B][ldf] in Hz (a frame is voiced where f0 > 0): x = ln f0 at a voiced frame,
 * x[t0] + (x[t1] - x[t0]) * ((t - t0) / (t1 - t0)) between the nearest voiced frames t0 < t < t1, the first / last voiced value
 * before / after them; m = (sum x) / T, sd = sqrt(sum (x - m)^2 / T) in a second pass, z[b][t] = (x[t] - m) / sd, and
 * stats[b][0..4) = {voiced frames, m, sd, flat}; flat = 1 without a voiced frame (then m = sd = 0) or with sd <= 1e-12, and z is
 * then 0 over [0, T).  Strides ldf, ldz >= Tmax, lds >= 4; z must not be f0. */
int fs2_cwt_contour(const double* f0, long ldf, const int32_t* lens, double* z, long ldz, double* stats, long lds, int B, int Tmax,
                    fs2_stream_t stream);
/* w[b][i][t] = sum over u in [0, lens[b]), ascending, of z[b][u] tab[i][|u - t|], i < 10, with tab [10][ldt] the caller's device
 * tables, of which support[i] entries count (HOST memory; 1 <= support[i] <= min(ldt, 2048)) and the rest is taken as 0, and
 * power[b][i] = sum_t w[b][i][t]^2.  Strides ldz, ldw_i >= Tmax, ldw_b >= 10 ldw_i, ldp >= 10; B <= 65535. */
int fs2_cwt_transform(const double* z, long ldz, const int32_t* lens, const double* tab, long ldt, const int32_t* support, double* w,
                      long ldw_b, long ldw_i, double* power, long ldp, int B, int Tmax, fs2_stream_t stream);
/* Along the path (pi, pj, plen as fs2_dtw_backtrack writes them), for the 15 components c of w_ref / w_syn (as fs2_cwt_transform
 * writes them): c < 10 the scale c, c = 10 + j the level w[2 j] + w[2 j + 1], with x = the component of w_ref at pi[k] and y that of
 * w_syn at pj[k]: sums[p][c][0..4) = {Sxx, Syy, Sxy about the two means of a first pass, Sd2 = sum (x - y)^2}; all 0 for a pair
 * without a path cell.  Strides ldr_i >= T1max, ldr_b >= 10 ldr_i (w_syn alike), ldo_c >= 4, ldo_b >= 15 ldo_c; B <= 65535. */
int fs2_cwt_on_path(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* w_ref, long ldr_b, long ldr_i,
                    const double* w_syn, long lds_b, long lds_i, const int32_t* alens, const int32_t* blens, double* sums, long ldo_b,
                    long ldo_c, int B, int T1max, int T2max, fs2_stream_t stream);

/* ---- harmonics-to-noise ratio (csrc/fs2_hnr.hip; specification: fastspeech2_amd/hnr.py) ----
 * Ragged batches: row b of the float32 audio y [B][ldy] has lens[b] samples and frames[b] frames (int32, device), 1 <= Tmax <=
 * fs2_dtw_max_frames().  fp64 after the load; no atomics, every sum carries its rounding errors in a second word and has one order:
 * the same input gives the same bytes, whatever rows are beside it.  Nothing at a frame >= frames[b] is read or written, no sample
 * >= lens[b] is read.
 * fs2_hnr_max_window: the longest window N = 2 h + 1 in samples, 8191. */
int fs2_hnr_max_window(void);
/* Frame t < frames[b] of row b: x[k] = y[b][t hop - h + k], k < N = 2 h + 1, 0 outside [0, lens[b]); mu = (sum x) / N, a[k] = (x[k] -
 * mu) w[k], r0 = sum a^2, with w [N] and rw [lmax + 1] the caller's device tables (the window and its normalised autocorrelation).
 * With f = f0[b][t] (f0 [B][ldf] f64, Hz): the frame is invalid, out[b][t][0..3) = 0 and lag[b][t] = 0, when f is not above 0, r0 <=
 * 1e-20 N, or l1 < l0 for tau0 = fs / f, l0 = max(2, ceil(tau0 / 1.2)), l1 = min(lmax - 1, floor(tau0 * 1.2)).  Otherwise r'(tau) =
 * (sum_{k < N - tau} a[k] a[k + tau]) / (r0 rw[tau]) for tau in [l0 - 1, l1 + 1], lag[b][t] = the first tau in [l0, l1] that
 * maximises it, the peak of the parabola through its two neighbours (r' itself when the second difference d is not below 0: r' -
 * (r'(tau + 1) - r'(tau - 1))^2 / (8 d)), r = that clipped to [1e-3, 1 - 1e-6], and out[b][t] = {r, 10 log10(r / (1 - r)), 1}.
 * 3 <= N <= fs2_hnr_max_window(), 3 <= lmax < N, hop >= 1; strides ldf, ldl >= Tmax, ldo_t >= 3, ldo_b >= Tmax ldo_t; B <= 65535. */
int fs2_hnr_frames(const float* y, long ldy, const int32_t* lens, const double* f0, long ldf, const int32_t* frames, const double* w,
                   const double* rw, double fs, int hop, int h, int lmax, double* out, long ldo_b, long ldo_t, int32_t* lag, long ldl, int B,
                   int Tmax, fs2_stream_t stream);
/* stats[b][0..3) = {n, mean, M2}: the number of frames t < frames[b] of fr (as fs2_hnr_frames writes it) with fr[b][t][2] != 0, the
 * mean of their fr[b][t][1] and, in a second pass, the sum of the squared differences from it; all 0 without such a frame.  lds >= 3. */
int fs2_hnr_side(const double* fr, long ldf_b, long ldf_t, const int32_t* frames, double* stats, long lds, int B, int Tmax,
                 fs2_stream_t stream);
/* Along the path (pi, pj, plen as fs2_dtw_backtrack writes them), over the cells whose frames pi[k] of fr_ref and pj[k] of fr_syn
 * (both as fs2_hnr_frames writes them) are both valid, with x, y their two hnr values: sums[p][0..7) = {cells, mean x, mean y, Sxx,
 * Syy, Sxy about those means of a first pass, Sd2 = sum (x - y)^2}; all 0 for a pair without such a cell.  ldo >= 7. */
int fs2_hnr_on_path(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* fr_ref, long lda_b, long lda_t,
                    const double* fr_syn, long ldb_b, long ldb_t, const int32_t* alens, const int32_t* blens, double* sums, long ldo, int B,
                    int T1max, int T2max, fs2_stream_t stream);

/* ---- time-aligned intelligibility: STOI and ESTOI (csrc/fs2_stoi.hip; specification: fastspeech2_amd/stoi.py) ----
 * Ragged batches of time-aligned pairs at 10 kHz: float32 rows x (clean) and y (B, ldx) sharing one device lens, fp64 after the load,
 * no atomics, fixed-order sums: the same input gives the same bytes.  Nothing at or beyond lens[b] is read.  Frames of 256 samples at
 * hop 128 start at s = 0, 128, .. with s < len - 256: F(len) = ceil((len - 256) / 128) for len > 256, else 0; Fmax = F(Nmax).  w [256]
 * is the caller's window.  Buffers of Fmax = 0 frames may be NULL.
 * fs2_stoi_frame_energy: e[b][j] = sum_n (x[b][128 j + n] w[n])^2, j < F(lens[b]). */
int fs2_stoi_frame_energy(const float* x, long ldx, const int32_t* lens, const double* w, double* e, long lde, int B, int Nmax,
                          fs2_stream_t stream);
/* mask[b][j] = (max_j e > 0 and e[b][j] > 1e-4 max_j e), j < F(lens[b]); map[b][i] = the i-th frame with mask 1, i < n_kept[b]
 * (int32 rows of stride ldm >= Fmax; nothing beyond those counts is written) */
int fs2_stoi_keep(const double* e, long lde, const int32_t* lens, int32_t* mask, int32_t* map, long ldm, int32_t* n_kept, int B,
                  int Nmax, fs2_stream_t stream);
/* xo[b][128 i + n] = sum over the kept frames i that cover the sample, ascending, of x[b][128 map[b][i] + n] w[n], and yo of y the
 * same: (n_kept[b] - 1) 128 + 256 samples per row (none when n_kept[b] = 0), ldo >= (Fmax - 1) 128 + 256; a gather, nothing is
 * scattered.  A map entry outside [0, F) is clamped into it. */
int fs2_stoi_ola(const float* x, const float* y, long ldx, const int32_t* lens, const double* w, const int32_t* map, long ldm,
                 const int32_t* n_kept, double* xo, double* yo, long ldo, int B, int Nmax, fs2_stream_t stream);
/* X[b][k][m] = sqrt(sum of |DFT_512(xo[b][128 m .. 128 m + 256) w)|^2 over the bins [edges[k], edges[k + 1])), k < 15, m < n_kept[b] - 1
 * (strides ldx_b >= 15 ldx_k, ldx_k >= Fmax - 1).  twiddle [512][2] = {cos, sin}(2 pi j / 512) is the caller's device table: no sine
 * is evaluated here.  edges: HOST memory, 16 ascending bins within [0, 257] spanning at most 256. */
int fs2_stoi_bands(const double* xo, long ldo, const int32_t* n_kept, const double* w, const double* twiddle, const int32_t* edges,
                   double* X, long ldx_b, long ldx_k, int B, int Fmax, fs2_stream_t stream);
/* Per segment s < n_kept[b] - 30 of 30 frames of X and Y (both as fs2_stoi_bands writes them): seg[b][0][s] = the mean over the 15
 * bands of the STOI correlation (clip = 1 + 10^(15 / 20) bounds alpha Y by clip X), seg[b][1][s] = the ESTOI score (rows, then
 * columns normalised; sum / 30); strides lds_b >= 2 lds_k, lds_k >= Fmax - 30 */
int fs2_stoi_segments(const double* X, const double* Y, long ld_b, long ld_k, const int32_t* n_kept, double clip, double* seg,
                      long lds_b, long lds_k, int B, int Fmax, fs2_stream_t stream);
/* out[b][6] = {STOI, ESTOI (the means of the row's S = max(n_kept[b] - 30, 0) segment scores in a fixed order; NaN when S = 0),
 * F(lens[b]), n_kept[b], S, S == 0} */
int fs2_stoi_mean(const double* seg, long lds_b, long lds_k, const int32_t* lens, const int32_t* n_kept, double* out, int B, int Nmax,
                  fs2_stream_t stream);

/* ---- speaker similarity: GMM-UBM (csrc/fs2_spk.hip; specification: fastspeech2_amd/speaker.py) ----
 * fp64 throughout, no atomics, fixed-order sums: the same input gives the same bytes.  Frames are PACKED: utterance u owns the rows
 * offs[u] .. offs[u] + n_kept[u] of a [N][D] matrix (offs, n_kept: int32 on the device).  A mixture is given expanded: a[m][d] =
 * mu / var, b[m][d] = -1 / (2 var) (rows of stride ldt >= D), c[m] = log w - 1/2 sum_d (log(2 pi var) + mu^2 / var), -inf allowed;
 * L[n][m] = c[m] + sum_d (x[n][d] a[m][d] + x[n][d]^2 b[m][d]).  Limits, all FS2_EINVAL before any launch: 1 <= D <=
 * fs2_spk_max_dim() (64), 1 <= M <= fs2_spk_max_components() (2048), G M < 2^31, N < 2^31 (an int).  Nothing beyond a row's D columns
 * or at a row >= N is read or written. */
int fs2_spk_max_dim(void);
int fs2_spk_max_components(void);
/* cep [B][Tmax][n_cep + 1] (strides ldc_b >= Tmax ldc_t, ldc_t >= n_cep + 1; column 0 is c0), 1 <= n_cep <= 32, D = 2 n_cep.  Feature j
 * of frame t: cepstrum j + 1 for j < n_cep, else (d1 + 2 d2) / 10 with dk = c[min(t + k, T - 1)] - c[max(t - k, 0)] of cepstrum
 * j - n_cep + 1.  A frame passes when c0[t] >= max_t c0 - energy_floor (>= 0).  With n >= 2 frames passing: mean[b][j] = their sum in
 * ascending t over n, var[b][j] = the sum of the squared differences from that mean over n (rows of stride ldm >= D); when every var is
 * > 0, n_kept[b] = n and feat[offs[b] + i][j] = (f - mean) / sqrt(var) for the i-th passing frame (row stride ldf >= D), else n_kept[b]
 * = 0 and no row is written.  With n < 2: n_kept[b] = 0, mean and var NaN, no row written.  Nothing at t >= lens[b] is read; rows
 * beyond n_kept[b] are not written.  One workgroup per utterance. */
int fs2_spk_feats(const double* cep, long ldc_b, long ldc_t, const int32_t* lens, const int32_t* offs, int n_cep, double energy_floor,
                  double* feat, long ldf, int32_t* n_kept, double* mean, double* var, long ldm, int B, int Tmax, fs2_stream_t stream);
/* lse[n][g] = log sum_m exp L[n][g M + m] for the G groups of M components in a, b [G M][ldt], c [G M] (row stride ldl >= G); -inf when
 * every c of the group is -inf.  post, NULL or for G = 1 only: post[n][m] = exp(L[n][m] - lse[n]) (row stride ldp >= M), 0 where lse
 * is -inf.  The contraction runs on v_mfma_f64_16x16x4_f64 over k = (x, x^2), four k per step ascending; a workgroup owns 64 frames
 * and walks the 64-component tiles of its groups, folding them into a running (max, sum) in a fixed order. */
int fs2_spk_loglik(const double* x, long ldx, const double* a, const double* b, long ldt, const double* c, double* lse, long ldl,
                   double* post, long ldp, int N, int D, int M, int G, fs2_stream_t stream);
/* doubles of workspace fs2_spk_accum needs (0 for N <= 0 or D, M outside their limits): chunks x ceil(M / 64) x ceil((1 + 2 D) / 64)
 * tiles of 4096, at most 32 x 32 x 3 of them */
int fs2_spk_accum_ws(int N, int D, int M);
/* stats[m][0 .. 1 + 2 D) += sum_n post[n][m] (1, x[n][0..D), x[n][0..D)^2) (row stride lds >= 1 + 2 D); the caller zeroes stats before
 * the first batch.  The N rows are cut into at most 32 chunks whose length (a multiple of 16) depends on N only; 64 x 64 tiles are
 * summed per chunk with v_mfma_f64_16x16x4_f64 in ascending n into ws and added in ascending chunk order.  ws_doubles below
 * fs2_spk_accum_ws() is FS2_EINVAL. */
int fs2_spk_accum(const double* post, long ldp, const double* x, long ldx, double* stats, long lds, double* ws, long ws_doubles, int N,
                  int D, int M, fs2_stream_t stream);
/* out[u][g] = (sum over r = offs[u] .. offs[u] + n_kept[u], ascending, of lse[r][g] - ubm[r]) / n_kept[u], g < G (row strides ldl,
 * ldo >= G); NaN when n_kept[u] <= 0.  IEEE arithmetic on -inf: a -inf in lse alone gives -inf, in both gives NaN. */
int fs2_spk_mean_rows(const double* lse, long ldl, const double* ubm, const int32_t* offs, const int32_t* n_kept, double* out, long ldo,
                      int U, int G, fs2_stream_t stream);

/* ---- spectral envelope (CheapTrick) and its mel-cepstrum (specification: fastspeech2_amd/envelope.py) ----
 * fp64 throughout, ragged: row b has lens[b] samples of the float32 batch x (row stride ldx) and frames[b] frames (int32, device);
 * f0 [B][ldf] f64, one value per frame; spectra [B][Fmax][N / 2 + 1] with batch / frame strides in elements, N a power of two in
 * [256, 2048]; twiddle [N / 2][2] = {cos, -sin}(2 pi k / N) is the caller's table: no sine is evaluated for a transform.  Nothing
 * at a frame >= frames[b] or a sample >= lens[b] is read or written.  No atomics, fixed-order sums.
 * fs2_env_spectrum: P[b][f] = DC-corrected power spectrum of the clamped, Hann-windowed, mean-removed frame at f frame_period ms. */
int fs2_env_spectrum(const float* x, long ldx, const int32_t* lens, const double* f0, long ldf, const int32_t* frames, double fs,
                     double frame_period, const double* twiddle, int N, double* P, long ldp_b, long ldp_t, int B, int Fmax, int Nmax,
                     fs2_stream_t stream);
/* in place, P -> envelope: linear smoothing of width 2 f0 / 3, + env_floor, then the sinc and recovery (q1) lifters on its cepstrum */
int fs2_env_smooth(const double* f0, long ldf, const int32_t* frames, double fs, const double* twiddle, int N, double q1,
                   double env_floor, double* P, long ldp_b, long ldp_t, int B, int Fmax, fs2_stream_t stream);
/* c[b][f][m - 1] = sum_q table[m - 1][q] c_q, m = 1 .. K <= 40, c_q the one-sided cepstrum of 0.5 ln env[b][f]; table [K][N / 2 + 1]
 * is the caller's freqt recursion applied to the unit vectors; c [B][Fmax][K] in the row layout fs2_dtw_cost reads */
int fs2_env_mcep(const double* env, long lde_b, long lde_t, const int32_t* frames, const double* twiddle, int N, const double* table,
                 int K, double* c, long ldc_b, long ldc_t, int B, int Fmax, fs2_stream_t stream);

/* ---- loss (model/loss.py:19-92): masked L1 (mel, post-net mel) + masked MSE (pitch, energy, log-duration) ----
 * mel / post: [B][T][n_mel] f32 predictions; mel_t: target with batch stride ld_t_b (its own padded length >= T);
 * lens int64 (valid = t < min(len, T)); p/e predictions [B][L] (phoneme level) or [B][T] (p_frame / e_frame = 1) with
 * target row strides ld_pt / ld_et; logd [B][L], dur int64 [B][L] (row stride ld_dur; target = log(dur + 1));
 * cnt (device) = {valid phonemes, valid frames} = the divisors of the means (data-parallel: global counts / world).
 * fwd: sums[5] workspace, losses[6] = {total, mel, postnet, pitch, energy, duration}.
 * bwd: g[6] (device) upstream gradients of the 6 outputs; writes dense gradients (exact zeros on padding). */
int fs2_loss_fwd(const float* mel, const float* post, const float* mel_t, long ld_t_b, const int64_t* mel_lens,
                 const int64_t* src_lens, const float* p_pred, const float* p_t, long ld_pt, const float* e_pred,
                 const float* e_t, long ld_et, const float* logd, const int64_t* dur, long ld_dur, const float* cnt,
                 int B, int T, int L, int n_mel, int p_frame, int e_frame, float* sums, float* losses, fs2_stream_t stream);
int fs2_loss_bwd(const float* mel, const float* post, const float* mel_t, long ld_t_b, const int64_t* mel_lens,
                 const int64_t* src_lens, const float* p_pred, const float* p_t, long ld_pt, const float* e_pred,
                 const float* e_t, long ld_et, const float* logd, const int64_t* dur, long ld_dur, const float* cnt,
                 const float* g, int B, int T, int L, int n_mel, int p_frame, int e_frame, float* dmel, float* dpost,
                 float* dp, float* de, float* dlogd, fs2_stream_t stream);
/* fs2_loss_fwd with a KEPT workspace: sums_ws (5 floats) is zero on entry (zeroed once by its owner) and zero again on return,
 * so no clear is launched in front; calls sharing one workspace must be ordered. */
int fs2_loss_fwd_ws(const float* mel, const float* post, const float* mel_t, long ld_t_b, const int64_t* mel_lens,
                    const int64_t* src_lens, const float* p_pred, const float* p_t, long ld_pt, const float* e_pred,
                    const float* e_t, long ld_et, const float* logd, const int64_t* dur, long ld_dur, const float* cnt,
                    int B, int T, int L, int n_mel, int p_frame, int e_frame, float* sums_ws, float* losses, fs2_stream_t stream);
/* fs2_loss_bwd with the upstream factors as six device scalars (NULL = 0: that term was not differentiated) and dmel / dpost
 * stored in grad_dtype (FS2_BF16: rounded to nearest even, bit for bit fs2_cast of the fp32 gradient), rows [B*T][n_mel]. */
int fs2_loss_bwd_lp(const float* mel, const float* post, const float* mel_t, long ld_t_b, const int64_t* mel_lens,
                    const int64_t* src_lens, const float* p_pred, const float* p_t, long ld_pt, const float* e_pred,
                    const float* e_t, long ld_et, const float* logd, const int64_t* dur, long ld_dur, const float* cnt,
                    const float* g_total, const float* g_mel, const float* g_post, const float* g_pitch, const float* g_energy,
                    const float* g_dur, int B, int T, int L, int n_mel, int p_frame, int e_frame, void* dmel, void* dpost,
                    int grad_dtype, float* dp, float* de, float* dlogd, fs2_stream_t stream);

/* ---- optimiser: train.py:93 clip_grad_norm_ + model/optimizer.py:10-51 Adam ------------------------- */
/* ws: FS2_SUMSQ_BLOCKS floats of workspace (two-stage reduction in a fixed order: bit-reproducible norm) */
#define FS2_SUMSQ_BLOCKS 1024
int fs2_sumsq(const float* x, size_t n, float* out /*+=*/, float* ws, fs2_stream_t stream);
int fs2_sumsq_set(const float* x, size_t n, float* out /*=: no clear needed in front*/, float* ws, fs2_stream_t stream);
/* hyper (device) = {lr, 1-beta1^t, 1-beta2^t}; clip = min(1, max_norm/(sqrt(*gnorm_sq)+1e-6)).
 * p_lowp (optional, bf16): compute-dtype copy of the updated parameters written in the same pass;
 * zero_grad: clear g as it is consumed (optimizer.zero_grad(), model/optimizer.py:30-31).  n % 4 == 0. */
int fs2_adam_step(float* p, float* g, float* m, float* v, size_t n, const float* gnorm_sq, float max_norm,
                  const float* hyper, float b1, float b2, float eps, float wd, void* p_lowp, int lowp_dtype, int zero_grad,
                  fs2_stream_t stream);
/* the same with lr / 1-beta1^t / 1-beta2^t as launch arguments (eager steps: no host-to-device copy in front of the optimiser) */
int fs2_adam_step_h(float* p, float* g, float* m, float* v, size_t n, const float* gnorm_sq, float max_norm, float lr, float bc1,
                    float bc2, float b1, float b2, float eps, float wd, void* p_lowp, int lowp_dtype, int zero_grad,
                    fs2_stream_t stream);

/* ---- grapheme-to-phoneme: graphone n-gram, many-to-many EM alignment and beam search (specification: fastspeech2_amd/g2p.py) ----
 * fp64 throughout, ragged batches of words: word w has glens[w] letters (index i) and plens[w] phones (index j), int32 on the
 * device, ids in int32 rows letters [W][ldl] and phones [W][ldp]; an id outside [0, A) / [0, P) makes every arc over it absent.
 * Arc code c consumes (letters, phones) = (1,0), (1,1), (1,2), (2,1).  logtheta is the dense table of A NQ + A A P doubles,
 * NQ = 1 + P + P P: codes 0..2 at a NQ + q (q = 0 | 1 + p | 1 + P + p0 P + p1), code 3 at A NQ + (a0 A + a1) P + p; n_table must be
 * exactly that and at most fs2_g2p_max_table_mib() MiB.  Limits, FS2_EINVAL before any launch: A <= fs2_g2p_max_letters() (64),
 * P <= fs2_g2p_max_phones() (128), Lgmax <= fs2_g2p_max_word_letters() (32), Lpmax <= fs2_g2p_max_word_phones() (48), beam K <=
 * fs2_g2p_max_beam() (256), order N <= fs2_g2p_max_order() (4).  Nothing at i >= glens[w] or j >= plens[w] of an id row is read,
 * nothing outside a word's own cells is written.  No atomics; every sum has one order.  Nothing of this has been timed. */
int fs2_g2p_max_letters(void);
int fs2_g2p_max_phones(void);
int fs2_g2p_max_word_letters(void);
int fs2_g2p_max_word_phones(void);
int fs2_g2p_max_beam(void);
int fs2_g2p_max_order(void);
int fs2_g2p_max_table_mib(void);
/* log-domain forward / backward over the (Lg + 1) x (Lp + 1) lattice, the log-sum-exp in arc-code order: loglik[w] (-inf without a
 * path) and post[w][i][j][c], i < Lg, j <= Lp (strides ldo_w >= Lgmax ldo_i, ldo_i >= 4 (Lpmax + 1)), the posterior of the arc of
 * code c that leaves cell (i, j): exactly 0 when the arc does not exist or lies on no path, never NaN */
int fs2_g2p_m2m_expect(const int32_t* letters, long ldl, const int32_t* phones, long ldp, const int32_t* glens, const int32_t* plens,
                       const double* logtheta, long n_table, int A, int P, double* loglik, double* post, long ldo_w, long ldo_i, int W,
                       int Lgmax, int Lpmax, fs2_stream_t stream);
/* the same lattice with max: score[w] the best path's log weight (-inf without one), bp[w][i][j], i <= Lg, j <= Lp (strides ldb_w >=
 * (Lgmax + 1) ldb_i, ldb_i >= Lpmax + 1), the code of the best arc into (i, j), the lowest on ties, 255 at (0, 0) and at a cell no
 * path reaches */
int fs2_g2p_m2m_viterbi(const int32_t* letters, long ldl, const int32_t* phones, long ldp, const int32_t* glens, const int32_t* plens,
                        const double* logtheta, long n_table, int A, int P, double* score, uint8_t* bp, long ldb_w, long ldb_i, int W,
                        int Lgmax, int Lpmax, fs2_stream_t stream);
/* The back-off n-gram: order n <= N holds the entries [order_offs[n - 1], order_offs[n]) of keys / logp / bow (n_keys in all), keys
 * ascending, a key packing n ids of 16 bits with the oldest in the highest place.  out[q] = log P(tok[q] | hist[q][0 .. N - 1)),
 * the history oldest first (ldh >= N - 1): found at order n -> its logp; else bow of the order's history (0 when that history has
 * no entry) + the score under the history without its oldest id; -inf when the token has no unigram.  The weights are added from
 * the longest history down, the log-probability last. */
int fs2_g2p_ngram_score(const int32_t* hist, long ldh, const int32_t* tok, const uint64_t* keys, const double* logp, const double* bow,
                        const int32_t* order_offs, int n_keys, int N, double* out, int n, fs2_stream_t stream);
/* Beam search, one workgroup per word, synchronous in the letter position, no recombination.  Graphone types are 0 .. T - 1 (T <
 * 65534), <s> = T, </s> = T + 1; type_phones [T][2] their phones (-1 = none); spell_offs [A + A A + 1] / spell_types [n_spell] list
 * per letter chunk (a | A + a0 A + a1) the ascending types that spell it, a row cut at max_fan1 (one letter) / max_fan2 (two).
 * Hypotheses at position i expand those at i - 1 by the types spelling letters[i-1:i], then those at i - 2 by the types spelling
 * letters[i-2:i]; candidates are numbered in that order, parent slot ascending, type ascending; the K best are kept, ties to the
 * lower number, -inf dropped.  Caller's workspace, readable afterwards: beam_score / beam_hist / beam_bp [W][Lgmax + 1][K] (hist =
 * the last three ids packed like a key, bp = 2 (parent slot) + letters consumed - 1), beam_n [W][Lgmax + 1] the kept counts, cand
 * [W][ldc], ldc >= K (max_fan1 + max_fan2).  At the end log P(</s> | history) is added and the best (the lower slot on ties) is
 * walked back: out_phones[w][0 .. out_n[w]) (ldo >= 2 Lgmax), out_score[w]; out_n[w] = -1 and -inf when nothing reaches the end
 * (an unknown letter, an unseen spelling). */
int fs2_g2p_decode(const int32_t* letters, long ldl, const int32_t* glens, int A, const int32_t* spell_offs, const int32_t* spell_types,
                   int n_spell, int max_fan1, int max_fan2, const int32_t* type_phones, int T, const uint64_t* keys, const double* logp,
                   const double* bow, const int32_t* order_offs, int n_keys, int N, int K, double* beam_score, uint64_t* beam_hist,
                   int32_t* beam_bp, int32_t* beam_n, double* cand, long ldc, int32_t* out_phones, long ldo, int32_t* out_n,
                   double* out_score, int W, int Lgmax, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
