/*
 * salsa_nn.h -- C ABI of the layers of the SELD CRNN consumer that are hand-written for MI355X: average pools, fused
 * BatchNorm, and EVERY convolution of the training step on the matrix cores -- forward, data gradient and weight gradient of
 * the first layer (salsa_nn_conv3x3_stem*), the 64 -> 64 layers (salsa_nn_conv3x3_c64*), the 128 / 256 / 512-channel layers
 * (salsa_nn_conv3x3_wide*) and the 1x1 shortcuts (salsa_nn_conv1x1*); nothing of the step is left on MIOpen.  Tensors are channels-last ([N][H][W][C], C fastest), device pointers, caller-owned;
 * dtype: 0 = float32, 1 = bfloat16; asynchronous on the given HIP stream.
 *
 *   salsa_nn_avgpool2x2_{fwd,bwd}: F.avg_pool2d(x, 2) of the upstream model (models/model_utils.py:187-228 ConvBlock,
 *   the strided residual stages of the PANN ResNet22): y[n][h][w][c] = (x[2h][2w] + x[2h][2w+1] + x[2h+1][2w] +
 *   x[2h+1][2w+1]) / 4 accumulated in float32 in that order; odd trailing rows / columns are dropped (floor mode) and
 *   get zero gradient.  C must be a multiple of 8 (bf16) or 4 (float32).
 *
 *   salsa_nn_bn_*: nn.BatchNorm2d of the upstream blocks fused with what follows it there -- the residual add and the
 *   ReLU (models/model_utils.py:187-228, :312-367): y = [relu]( ((x - mean) * invstd) * gamma + beta [+ residual] ).
 *   x, y, residual, dy, dx: [M][C] (M = N*H*W) in `dtype`; gamma, beta, statistics: float32 [C].  Training statistics are
 *   accumulated per block in float32 and across blocks in float64 (sums_ws: salsa_nn_bn_workspace_bytes of scratch) and the running statistics are updated like torch does
 *   (momentum, unbiased variance).  Backward: with g = dy * (y > 0) (relu = 0: g = dy),
 *   dbeta = sum g, dgamma = sum g * xhat, dx = gamma * invstd * (g - dbeta/M - xhat * dgamma/M), and dres = g when the
 *   forward had a residual.  With relu != 0 and y_or_null = NULL (allowed when the forward had NO residual) the mask is
 *   recomputed from x, which saves reading y.  coef_ws: 7*C floats of scratch.  salsa_nn_bn_supported: C/L must be a power of two <= 256
 *   (L = 8 for bf16, 4 for float32).
 *
 *   salsa_nn_conv3x3_c64: the 3x3 / stride 1 / pad 1 convolution with 64 input and 64 output channels (the stem's second
 *   convolution and the four of the first residual stage: 42 % of the network's convolution FLOPs) on the matrix cores,
 *   bf16 in / float32 accumulate / bf16 out.  x, y: [N][H][W][64]; w: [64 co][3][3][64 ci] (a channels-last
 *   torch.nn.Conv2d weight).  The data gradient is the same call on dy with the filter flipped and transposed
 *   (w'[ci][r][s][co] = w[co][2-r][2-s][ci]).  salsa_amd/csrc/conv_mfma.hip describes the kernel.
 */
#ifndef SALSA_NN_H
#define SALSA_NN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int salsa_nn_avgpool2x2_fwd(const void *x, void *y, int dtype, int64_t N, int H, int W, int C, void *hip_stream);
int salsa_nn_avgpool2x2_bwd(const void *grad_y, void *grad_x, int dtype, int64_t N, int H, int W, int C, void *hip_stream);

int salsa_nn_conv3x3_c64(const void *x, const void *w, void *y, int64_t N, int H, int W, void *hip_stream);
/* inference: y = [relu](conv(x, w) + shift[co] [+ residual]) with the BatchNorm that follows folded in: w pre-scaled by
 * gamma / sqrt(var + eps) per output channel, shift = beta - mean * gamma / sqrt(var + eps) (float32 [64]); residual bf16 or NULL */
int salsa_nn_conv3x3_c64_bias_act(const void *x, const void *w, const float *shift, const void *residual, void *y, int relu,
                                  int64_t N, int H, int W, void *hip_stream);
/* the same followed by the 2x2 average pool of the upstream stem (taken in float32 before the single rounding):
 * y bf16 [N][H/2][W/2][64]; H and W even */
int salsa_nn_conv3x3_c64_bias_act_pool(const void *x, const void *w, const float *shift, const void *residual, void *y, int relu,
                                       int64_t N, int H, int W, void *hip_stream);
/* the network's first layer, Cin <= 16 -> 64 channels, on the extractor's output layout: x float32 planar [N][Cin][H][W] with
 * contiguous rows and the given batch / channel strides (elements; a time-cropped view needs no copy);
 * wq bf16, two layouts by Cin:
 *   Cin <= 8       (SALSA, 7 channels):          [64 co][10 taps][8 ci]  (taps row-major, tap 9 and ci >= Cin zero);
 *   9 <= Cin <= 16 (baseline GCC, 10 channels): [64 co][9 taps][16 ci]  (taps row-major, ci >= Cin zero);
 * y bf16 channels-last [N][H][W][64];
 * shift NULL: plain convolution, else y = [relu](conv + shift[co]) with the BatchNorm folded as above */
int salsa_nn_conv3x3_stem(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *wq, const float *shift,
                          void *y, int relu, int64_t N, int Cin, int H, int W, void *hip_stream);
/* the WIDE 3x3 / stride 1 / pad 1 convolutions (Cin a multiple of 32, Cout a multiple of 64: the 128 / 256 / 512-channel
 * residual stages, models/model_utils.py:312-367, :429-500): implicit GEMM over the flattened pixel axis, both operands staged
 * through LDS (salsa_amd/csrc/conv_wide.hip).  x [N][H][W][Cin], w [Cout][3][3][Cin], y [N][H][W][Cout], all bf16; float32
 * accumulation.  The data gradient is the same call on dy with w'[ci][r][s][co] = w[co][2-r][2-s][ci].
 * salsa_nn_conv3x3_wide_supported: 1 if the shape is taken (the padded input chunk of a 512-pixel tile must fit its LDS buffer). */
int salsa_nn_conv3x3_wide_supported(int64_t N, int H, int W, int Cin, int Cout);
int salsa_nn_conv3x3_wide(const void *x, const void *w, void *y, int64_t N, int H, int W, int Cin, int Cout, void *hip_stream);
/* the kernel instantiation the two calls above and salsa_nn_conv3x3_wide_stats / _bias_act launch for an output [N][H][W][Cout]:
 * returns the pixels per tile (512 | 256) and sets *tn to the output channels per tile (128 | 64); -1 for a NULL tn or a Cout
 * that is not a positive multiple of 64.  Host only (no device call): lets a test prove which instantiation a shape reaches. */
int salsa_nn_conv3x3_wide_config(int64_t N, int H, int W, int Cout, int *tn);
/* inference: y = [relu](conv(x, w) + shift[co] [+ residual]) with the BatchNorm that follows folded in (w pre-scaled per output
 * channel, shift float32 [Cout], residual bf16 like y or NULL), applied to the float32 sums before the single rounding */
int salsa_nn_conv3x3_wide_bias_act(const void *x, const void *w, const float *shift, const void *residual, void *y, int relu,
                                   int64_t N, int H, int W, int Cin, int Cout, void *hip_stream);
/* weight gradient of the wide layers (Cin a multiple of 32, Cout a multiple of 128): dw float32 [Cout][3][3][Cin] += sum_pixels
 * dy[p][co] * x[p+tap][ci] (zero it first), transposing LDS reads on the same flattened pixel axis.  The kernel walks many pixel
 * tiles per workgroup and takes its (n, h, w) arithmetic from two index tables of the map shape, built on the HOST by
 * salsa_nn_conv3x3_wide_tables (vpos: N*H*W ints, inv: salsa_nn_conv3x3_wide_table_len ints, tile_bounds: 2 *
 * salsa_nn_conv3x3_wide_tile_count ints) and uploaded once by the caller. */
int salsa_nn_conv3x3_wide_wrw_supported(int64_t N, int H, int W, int Cin, int Cout);
int64_t salsa_nn_conv3x3_wide_table_len(int64_t N, int H, int W);
int64_t salsa_nn_conv3x3_wide_tile_count(int64_t N, int H, int W);
int salsa_nn_conv3x3_wide_tables(int64_t N, int H, int W, int *vpos_host, int *inv_host, int *tile_bounds_host);
/* Training forward of the wide layers that also leaves the per-channel sum / sum of squares of its (bf16-rounded) output as
 * float64 partial rows stats_part[salsa_nn_conv3x3_wide_stats_blocks(...)][2][Cout] in its epilogue, like
 * salsa_nn_conv3x3_c64_stats: the BatchNorm that follows (salsa_nn_bn_train_fwd: stats_part, stats_blocks) makes no statistics
 * pass over y. */
int salsa_nn_conv3x3_wide_stats_blocks(int64_t N, int H, int W, int Cin, int Cout);
int salsa_nn_conv3x3_wide_stats(const void *x, const void *w, void *y, double *stats_part, int64_t N, int H, int W, int Cin, int Cout,
                                void *hip_stream);
int salsa_nn_conv3x3_wide_wrw(const void *x, const void *dy, float *dw, const int *d_vpos, const int *d_inv, const int *d_tile_bounds,
                              int64_t N, int H, int W, int Cin, int Cout, void *hip_stream);
/* Training forward of the 64 -> 64 layer that ALSO leaves the per-channel sum and sum of squares of its (bf16-rounded) output as
 * per-workgroup float64 rows stats_part[salsa_nn_conv3x3_c64_stats_blocks(N, H, W)][2][64], accumulated in its epilogue: the
 * BatchNorm that follows (salsa_nn_bn_train_fwd / _pool: stats_part, stats_blocks) then makes no statistics pass over y. */
int salsa_nn_conv3x3_c64_stats_blocks(int64_t N, int H, int W);
int salsa_nn_conv3x3_c64_stats(const void *x, const void *w, void *y, double *stats_part, int64_t N, int H, int W, void *hip_stream);
/* the geometry the 64 -> 64 forward (salsa_nn_conv3x3_c64, _stats, _xform_stats, _bias_act[_pool]) runs for [N][H][W][64], and the
 * weight gradient as well (its tiles are the same 4 x 32 pixels): returns the tile count and sets *transposed to 1 when the kernels
 * take the map with its axes swapped, else 0; -1 for a NULL transposed or a bad shape.  Host only (no device call): lets a test
 * prove which geometry a shape reaches. */
int salsa_nn_conv3x3_c64_config(int64_t N, int H, int W, int *transposed);
/* Training forward of the first layer from a persistent launch that also leaves the per-channel partial sums of its output
 * (see salsa_nn_conv3x3_c64_stats): stats_part[salsa_nn_conv3x3_stem_stats_blocks(N, H, W)][2][64] float64. */
int salsa_nn_conv3x3_stem_stats_blocks(int64_t N, int H, int W);
int salsa_nn_conv3x3_stem_stats(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *wq, void *y,
                                double *stats_part, int64_t N, int Cin, int H, int W, void *hip_stream);
/* weight gradient of the (Cin <= 14) -> 64 first layer: dw float32 [64 co][Cin][3][3] contiguous += sum_pixels dy[p][co] *
 * x[ci][p + tap] (zero it first); x float32 planar as in salsa_nn_conv3x3_stem, dy bf16 channels-last [N][H][W][64].
 * Cin <= 7 covers the Cin * 9 columns with one 64-column block, 8 <= Cin <= 14 with two (128 columns, the last one kept for
 * the ones plane of _bnf).  This and the two calls below return -1 for Cin > 14. */
int salsa_nn_conv3x3_stem_wrw(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *dy, float *dw, int64_t N,
                              int Cin, int H, int W, void *hip_stream);
/* The same with the BatchNorm (+ ReLU) behind the first layer differentiated on the fly: g = gradient of the BatchNorm's OUTPUT,
 * x1 = the BatchNorm's input (= the first layer's output), coef = the [7][64] table salsa_nn_bn_bwd leaves in coef_ws.  Call
 * salsa_nn_bn_bwd with dx = NULL (it then only produces dgamma, dbeta and coef_ws): dx's only reader is this weight gradient,
 * so the full-resolution dx is neither written nor read. */
int salsa_nn_conv3x3_stem_wrw_bn(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *g, const void *x1,
                                 const float *coef, int relu, float *dw, int64_t N, int Cin, int H, int W, void *hip_stream);

/* ... and with the BatchNorm backward's REDUCTION folded in as well (round 5): dx = a (g - b - xh k') is linear in the two totals
 * b = mean(g), k' = mean(g xh), so the pass over (g, x1, x) accumulates G = sum g (x) patch, Xh = sum xh (x) patch, S0 = sum patch,
 * dbeta = sum g, dgamma = sum g xh per workgroup, and a second small launch combines the slabs: dW = a (G - b S0 - k' Xh).  Replaces
 * salsa_nn_bn_bwd(dx = NULL) + salsa_nn_conv3x3_stem_wrw_bn (one pass over the 524-MB g and x1 instead of two).  mean / invstd: the
 * forward's saved statistics; ws: salsa_nn_conv3x3_stem_wrw_bnf_ws_bytes(N, H, W) bytes of device scratch (-5 when smaller); dw is
 * ADDED to, dgamma / dbeta are written.  Always bit-reproducible (slabs added in a fixed order, float64). */
size_t salsa_nn_conv3x3_stem_wrw_bnf_ws_bytes(int64_t N, int H, int W);
/* the workspace of salsa_nn_conv3x3_stem_wrw_bnf for 8 <= Cin <= 14 (128-column slabs and a grid of its own) */
size_t salsa_nn_conv3x3_stem16_wrw_bnf_ws_bytes(int64_t N, int H, int W);
int salsa_nn_conv3x3_stem_wrw_bnf(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *g, const void *x1,
                                  const float *mean, const float *invstd, const float *gamma, const float *beta, int relu, float *dw,
                                  float *dgamma, float *dbeta, void *ws, size_t ws_bytes, int64_t N, int Cin, int H, int W,
                                  void *hip_stream);
/* weight gradient of the same layer: dw float32 [64 co][3][3][64 ci] += sum_pixels dy[p][co] * x[p+tap][ci] (zero it first) */
int salsa_nn_conv3x3_c64_wrw(const void *x, const void *dy, float *dw, int64_t N, int H, int W, void *hip_stream);

/* Round 4: a conv -> BatchNorm -> ReLU (-> dropout) -> conv chain of the reference blocks (models/model_utils.py:213-228, :345-367)
 * without the normalised activation ever being stored.  The first convolution leaves its RAW output x1 and the per-workgroup
 * statistics (salsa_nn_conv3x3_*_stats); salsa_nn_bn_train_finalize turns those into mean / invstd (and updates the running
 * statistics) with no pass over x1; the SECOND convolution's forward (salsa_nn_conv3x3_c64_xform_stats: y = conv(a, w) + the
 * statistics epilogue for the BatchNorm that follows) and weight gradient (salsa_nn_conv3x3_c64_wrw_xform) form
 * a = dropout(relu(((x1 - mean) * invstd) * gamma + beta)) while they stage their operand -- as x1 * scale + shift with
 * scale = invstd * gamma, shift = beta - mean * scale in float32, rounded once to bf16; the dropout mask is the one
 * salsa_nn_bn_train_fwd would draw for (drop_p, drop_seed), so salsa_nn_bn_bwd regenerates the same.  The convolution's zero padding
 * applies to a, not to x1.  All four vectors: float32 [64]. */
int salsa_nn_bn_train_finalize(const double *stats_part, int stats_blocks, int64_t M, int C, float eps, float momentum,
                               float *running_mean, float *running_var, float *save_mean, float *save_invstd,
                               int64_t *batches_tracked, void *hip_stream);
int salsa_nn_conv3x3_c64_xform_stats(const void *x1, const void *w, void *y, double *stats_part, const float *mean,
                                     const float *invstd, const float *gamma, const float *beta, float drop_p, uint32_t drop_seed,
                                     int64_t N, int H, int W, void *hip_stream);
int salsa_nn_conv3x3_c64_wrw_xform(const void *x1, const void *dy, float *dw, const float *mean, const float *invstd,
                                   const float *gamma, const float *beta, float drop_p, uint32_t drop_seed, int64_t N, int H, int W,
                                   void *hip_stream);

/* drop_p > 0 fuses the dropout that follows the ReLU in the upstream residual block (models/resnet.py:78): an element is kept
 * when a counter-based hash of (its index, drop_seed) says so and scaled by 1/(1-p), p quantised to 1/65536; the backward takes
 * the same (drop_p, drop_seed) and regenerates the mask, so none is stored.  M*C must be below 2^32. */
int salsa_nn_bn_supported(int dtype, int64_t M, int C);
size_t salsa_nn_bn_workspace_bytes(int dtype, int64_t M, int C); /* size of sums_ws (8-byte aligned) */
int salsa_nn_bn_train_fwd(const void *x, void *y, const void *residual, int dtype, int64_t M, int C, const float *gamma,
                          const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                          float *save_mean, float *save_invstd, double *sums_ws, int relu, float drop_p, uint32_t drop_seed,
                          int64_t *batches_tracked /* nn.BatchNorm2d.num_batches_tracked (device), += 1; may be NULL */,
                          const double *stats_part, int stats_blocks /* per-workgroup [2][C] float64 sum / sum-of-squares rows left
                          by the convolution that produced x (salsa_nn_conv3x3_c64_stats): the statistics pass over x is
                          skipped; NULL / 0: the call computes them itself */,
                          void *hip_stream);
int salsa_nn_bn_eval_fwd(const void *x, void *y, const void *residual, int dtype, int64_t M, int C, const float *gamma,
                         const float *beta, const float *mean, const float *invstd, int relu, void *hip_stream);
int salsa_nn_bn_bwd(const void *dy, const void *y_or_null, const void *x, void *dx, void *dres_or_null, int dtype, int64_t M,
                    int C, const float *gamma, const float *beta, const float *save_mean, const float *save_invstd, int relu,
                    float *dgamma, float *dbeta, double *sums_ws, float *coef_ws, float drop_p, uint32_t drop_seed,
                    void *hip_stream);

/* BatchNorm (training statistics) [+ residual] + ReLU + the 2x2 average pool that follows them -- in the upstream stem
 * (models/model_utils.py:187-228) and, with the block's shortcut as `residual`, at the end of every residual block whose
 * successor starts with the stride-2 pool (:312-367) -- one pass over x: x [N][H][W][C] -> y [N][H/2][W/2][C] (normalise, add,
 * ReLU each of the four pixels, average in float32, one rounding); the full-resolution activation is never written.  Backward
 * from the POOLED gradient: dx, and dres (the residual's gradient) when there was one; the ReLU mask is recomputed from x (and
 * the residual), the same float32 operations in the same order as the forward. */
int salsa_nn_bn_train_fwd_pool(const void *x, void *y, const void *residual, int dtype, int64_t N, int H, int W, int C,
                               const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                               float *running_var, float *save_mean, float *save_invstd, double *sums_ws, int64_t *batches_tracked,
                               const double *stats_part, int stats_blocks, void *hip_stream);
int salsa_nn_bn_bwd_pool(const void *dy_pooled, const void *x, const void *residual, void *dx, void *dres, int dtype, int64_t N, int H,
                         int W, int C, const float *gamma, const float *beta, const float *save_mean, const float *save_invstd,
                         float *dgamma, float *dbeta, double *sums_ws, float *coef_ws, void *hip_stream);

/* The ReLU mask as a BIT PLANE (round 4).  Where something is added before the ReLU (the residual blocks' second BatchNorm) the
 * backward cannot recompute the mask from x alone: it read the stored output y (or, for the pooled variant, the residual) -- 16 bytes
 * per vector in each of its two passes -- only to test `> 0`.  The *_bits forward variants also leave live_bits: one BYTE per
 * 16-byte vector (M * C / 8 bytes for bf16, M * C / 4 for float32; bit k = "output element k of the vector is positive", after the
 * dropout if any), and the backward reads that instead: salsa_nn_bn_bwd with relu = 2 and live_bits in y's place,
 * salsa_nn_bn_bwd_pool_bits with live_bits in the residual's place (dres, or NULL, still receives the residual's gradient).
 * Same results bit for bit (the bits ARE the tests the backward made).  Measured: 0.18 ms of a 10.2-ms training step. */
int salsa_nn_bn_train_fwd_bits(const void *x, void *y, const void *residual, int dtype, int64_t M, int C, const float *gamma,
                               const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                               float *save_mean, float *save_invstd, double *sums_ws, int relu, float drop_p, uint32_t drop_seed,
                               int64_t *batches_tracked, const double *stats_part, int stats_blocks, void *live_bits, void *hip_stream);
int salsa_nn_bn_train_fwd_pool_bits(const void *x, void *y, const void *residual, int dtype, int64_t N, int H, int W, int C,
                                    const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                                    float *running_var, float *save_mean, float *save_invstd, double *sums_ws, int64_t *batches_tracked,
                                    const double *stats_part, int stats_blocks, void *live_bits, void *hip_stream);
int salsa_nn_bn_bwd_pool_bits(const void *dy_pooled, const void *x, const void *live_bits, void *dx, void *dres, int dtype, int64_t N,
                              int H, int W, int C, const float *gamma, const float *beta, const float *save_mean,
                              const float *save_invstd, float *dgamma, float *dbeta, double *sums_ws, float *coef_ws, void *hip_stream);

/* The 1x1 / stride 1 convolutions of the residual shortcuts (models/model_utils.py:340-349) over the flattened pixel axis
 * (salsa_amd/csrc/conv_1x1.hip): x bf16 [M][Cin] (channels-last pixels, M = N*H*W), w bf16 [Cout][Cin], y bf16 [M][Cout];
 * the data gradient is the same call on dy with the transposed filter [Cin][Cout]; the weight gradient is float32 [Cout][Cin],
 * ADDED to dw (zero it first).  *_supported: Cin % 16 == 0 and Cout % 64 == 0 (forward), Cin % 64 == 0 and Cout % 128 == 0 (wrw). */
int salsa_nn_conv1x1_supported(int64_t M, int Cin, int Cout);
int salsa_nn_conv1x1(const void *x, const void *w, void *y, int64_t M, int Cin, int Cout, void *hip_stream);
int salsa_nn_conv1x1_wrw_supported(int64_t M, int Cin, int Cout);
int salsa_nn_conv1x1_wrw(const void *x, const void *dy, float *dw, int64_t M, int Cin, int Cout, void *hip_stream);

/* The bf16 working copies of the float32 master filters (what autocast's per-layer casts + permutes + flips produce in the
 * reference's training step, models/seld_models.py:68-76 under torch.cuda.amp) for ALL layers in one launch: forward layout
 * [Cout][3][3][Cin] and, when the descriptor's bwd pointer is not 0, the data-gradient layout [Cin][3][3][Cout] with flipped taps.
 * desc (device memory): n_layers x 11 int64 = {src float32*, fwd bf16*, bwd bf16*, Cout, Cin, src element strides for
 * (co, ci, ky, kx), first block, taps (9: 3x3 filter, 1: 1x1 filter)}; layer l owns (Cout/32)*(Cin/32) consecutive blocks;
 * n_blocks = the total.  Cout, Cin % 32 == 0. */
int salsa_nn_conv_filter_bank(const void *desc, int n_layers, int n_blocks, void *hip_stream);

/* The SELD training loss and its gradients in one launch (reference models/interfaces.py:304-355, compute_loss: 0.3 x
 * BCE-with-logits of the event logits + 0.7 x the sum over x / y / z of the activity-masked mean absolute error): logit, sed_gt
 * [rows][nc], doa, doa_gt [rows][3 nc] (blocks x | y | z), float32 contiguous.  out3 = {loss, sed loss, doa loss};
 * g_logit = d sed / d logit, g_doa = d doa / d prediction, unweighted.  salsa_nn_seld_loss_bwd scales them by the incoming
 * gradients (device scalars, NULL = 0): out_a = a (g_loss w_sed + g_sed), out_b = b (g_loss w_doa + g_doa). */
#define SALSA_SELD_LOSS_WS 192 /* float64 values of scratch (partial_ws) salsa_nn_seld_loss needs: 64 workgroups x 3 partial sums */
int salsa_nn_seld_loss(const float *logit, const float *doa, const float *sed_gt, const float *doa_gt, int64_t rows, int nc,
                       float w_sed, float w_doa, float *out3, float *g_logit, float *g_doa, double *partial_ws, void *hip_stream);
int salsa_nn_seld_loss_bwd(const float *a, int64_t na, const float *b, int64_t nb, const float *g_loss, const float *g_sed,
                           const float *g_doa, float w_sed, float w_doa, float *out_a, float *out_b, void *hip_stream);

/* The ACCDOA training loss (output_format 'accdoa'; reference models/interfaces.py:273-302, compute_classwise_accdoa_loss) and
 * its gradient in one call: doa loss = sum over (row, class) of ((p_x - t_x)^2 + (p_y - t_y)^2 + (p_z - t_z)^2) sed_gt / rows;
 * sed_gt [rows][nc], doa, doa_gt [rows][3 nc] (blocks x | y | z), float32 contiguous.  out3 = {loss = doa loss, 0, doa loss} (the
 * reference discards its sed term); g_doa = 2 (p - t) sed_gt / rows; g_logit, when not NULL, [rows][nc] filled with zeros (the
 * event logits get an exact-zero gradient).  Float64 partial sums per workgroup added in a fixed order: bit-reproducible.  The
 * backward is salsa_nn_seld_loss_bwd with a = g_logit, b = g_doa, w_sed = 0, w_doa = 1. */
#define SALSA_ACCDOA_LOSS_WS 64 /* float64 values of scratch (partial_ws) salsa_nn_accdoa_loss needs: one per workgroup */
int salsa_nn_accdoa_loss(const float *doa, const float *sed_gt, const float *doa_gt, int64_t rows, int nc, float *out3, float *g_logit,
                         float *g_doa, double *partial_ws, void *hip_stream);
/* The SED decision of the ACCDOA output (reference models/interfaces.py:260-268): sed [rows][nc] = sqrt(x^2 + y^2 + z^2) of
 * xyz [rows][3 nc], float32, bit-equal to numpy's float32 expression (no fma, correctly rounded square root). */
int salsa_nn_accdoa_sed(const float *xyz, float *sed, int64_t rows, int nc, void *hip_stream);

/* The Multi-ACCDOA output format (output_format 'multi_accdoa'; salsa_amd/csrc/multi_accdoa.hip, statements in
 * multi_accdoa.h).  C = n_real_classes; three tracks (prediction) / slots (label) per class as pseudo-classes p = n C + c of the usual
 * layout: sed_gt [rows][3 C] in {0, 1}, doa and doa_gt [rows][9 C] (blocks x | y | z of 3 C columns), float32 contiguous.
 *
 * salsa_nn_adpit_loss: auxiliary duplicating permutation-invariant training.  Per item (row, c): the slots with sed_gt > 0.5 are
 * compacted in slot order into k sources; the candidate assignments (track 0, 1, 2 -> source) are, in index order, k = 0: the zero
 * target; k = 1: 000; k = 2: 001 010 011 100 101 110; k = 3: 012 021 102 120 201 210.  The cost of a candidate is the sum over
 * tracks (outer) and axes (inner) of (P - T)^2, one running float64 sum without fma; the chosen candidate is the lowest index of the
 * least cost (a later one wins only when strictly smaller, so a NaN cost never displaces an earlier candidate); the item loss is
 * cost / 9 and loss = sum of the items / (rows C), float64 partial sums per workgroup added in a fixed order: bit-reproducible.
 * out3 = {loss, 0, loss}; g_doa = (float)(2 (P - T_chosen) / (9 rows C)) in float64; g_logit, when not NULL, [rows][3 C] filled with
 * zeros; chosen, when not NULL, [rows][C] the candidate indices.  The backward is salsa_nn_seld_loss_bwd with w_sed = 0, w_doa = 1.
 * Returns 0; -1, before any device call, for a NULL required pointer, rows < 1, n_real_classes outside 1 .. 1024 or
 * rows * 9 C >= INT32_MAX; -6 when a launch fails. */
#define SALSA_ADPIT_LOSS_WS 64 /* float64 values of scratch (partial_ws) salsa_nn_adpit_loss needs: one per workgroup */
int salsa_nn_adpit_loss(const float *doa, const float *sed_gt, const float *doa_gt, int64_t rows, int n_real_classes, float *out3,
                        float *g_logit, float *g_doa, uint8_t *chosen, double *partial_ws, void *hip_stream);
/* salsa_nn_seld_decode_multi: file-level track activities act [n_files][n_in_frames][3 C] and vectors xyz [..][9 C] -> DCASE rows
 * with near-identical tracks of one class unified; only the first n_frames <= n_in_frames frames of a file are read.  Track n of
 * (frame, c) is active when act >= sed_threshold in float32 (NaN: inactive).  similar(i, j): both active and
 * dot > cos_unify sqrt(ni nj) with dot = (xi xj + yi yj) + zi zj and ni = (xi^2 + yi^2) + zi^2 in float64 without fma; cos_unify is
 * the cosine of the unification angle, computed by the caller.  With n_sim = sim01 + sim12 + sim20: 0 -- every active track emits
 * its own vector, in track order; 1 -- the similar pair emits (vi + vj) / 2.0f and the third track, if active, its own vector,
 * groups ordered by their lowest track; >= 2 -- one vector ((v0 + v1) + v2) / 3.0f (float32 per component, no fma).  rows
 * [n_files][3 n_frames C][4] int16 (8-byte aligned) receives (frame, real class, azimuth, elevation) -- the angles of
 * salsa_nn_seld_decode -- frame ascending, class ascending, then group order, in its first counts[f] rows per file; the rows behind
 * them are not written.  Bit-reproducible (no atomics).  Returns 0; -1, before any device call, for a NULL or misaligned pointer,
 * n_files < 1, n_frames or C outside 1 .. 32767, n_in_frames < n_frames, n_in_frames * 9 C > INT32_MAX / 4, or a cos_unify that is
 * NaN or outside [-1, 1]; -6 when the launch fails. */
int salsa_nn_seld_decode_multi(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames, int n_real_classes,
                               float sed_threshold, double cos_unify, int16_t *rows, int *counts, void *hip_stream);
/* salsa_nn_seld_decode_multi_thr: salsa_nn_seld_decode_multi with one threshold per REAL class, d_thresholds [n_real_classes] float32
 * on the device (4-byte aligned, not NULL), applied to the class's three tracks; a NaN threshold makes its class inactive.  The same
 * kernel code and checks; equal entries give salsa_nn_seld_decode_multi's rows and counts bit for bit. */
int salsa_nn_seld_decode_multi_thr(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames, int n_real_classes,
                                   const float *d_thresholds, double cos_unify, int16_t *rows, int *counts, void *hip_stream);

/* Test-time chunk combination and DCASE row decoding in one launch (reference models/interfaces.py:97-139 combine_chunks, then
 * :232-256 of write_classwise_output_to_file; salsa_amd/csrc/seld_decode.hip): sed [n_files][n_chunks][chunk_len][nc] ACTIVITIES (not
 * logits) and xyz [..][3 nc] (blocks x | y | z), float32 contiguous at the label rate; chunk_len and chunk_hop in label frames.
 * Chunk starts are arange(0, n_frames - chunk_len + 1, chunk_hop) plus the leftover start n_frames - chunk_len; chunk 0 is copied,
 * the first chunk_len - chunk_hop frames of every later chunk become (old + new) / 2 (combine 0) or sqrtf(old * new) (combine 1) and
 * its other frames overwrite -- the reference's running pairwise average, float32 without fma: bit-equal to numpy.  n_chunks == 1
 * is plain placement of a chunk of chunk_len >= n_frames frames, trimmed.  A pair (frame, class) is active when its combined sed
 * >= sed_threshold in float32 (NaN: inactive); rows [n_files][n_frames * nc][4] int16 (8-byte aligned) receives (frame, class,
 * azimuth, elevation) of file f's active pairs, frame ascending and class ascending within a frame, in its first counts[f] rows;
 * the rows behind them are not written.  The angles are round-half-even of atan2(y, x) and atan2(z, sqrt(x^2 + y^2)) in degrees,
 * computed in float64 from the combined xyz; azimuth 180 is written as -180.  file_sed [n_files][n_frames][nc] and file_xyz
 * [..][3 nc], when not NULL, receive the combined arrays.  Bit-reproducible (no atomics).  Returns 0; -1, before any device call,
 * for a NULL required pointer, n_frames or nc outside 1 .. 32767, chunk_len or chunk_hop < 1, n_chunks different from the number
 * of starts, chunk_hop > chunk_len or chunk_len > n_frames with more than one chunk, or combine not 0 / 1; -6 when the launch
 * fails. */
int salsa_nn_seld_decode(const float *sed, const float *xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop, int n_frames,
                         int nc, float sed_threshold, int combine, int16_t *rows, int *counts, float *file_sed, float *file_xyz,
                         void *hip_stream);
/* salsa_nn_seld_decode_thr: salsa_nn_seld_decode with one threshold per class, d_thresholds [nc] float32 on the device (4-byte
 * aligned, not NULL): pair (frame, c) is active when its combined activity >= d_thresholds[c] in float32 (NaN on either side:
 * inactive).  The same kernel code and checks; equal entries give salsa_nn_seld_decode's rows, counts and file outputs bit for bit. */
int salsa_nn_seld_decode_thr(const float *sed, const float *xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop, int n_frames,
                             int nc, const float *d_thresholds, int combine, int16_t *rows, int *counts, float *file_sed,
                             float *file_xyz, void *hip_stream);

/* DCASE rows against ground-truth rows: the SELD 2021 counters of crnn/metrics.py::SeldMetrics.update (reference metrics/
 * SELD2021_evaluation_metrics.py:81-195) per (file, segment), on the device (salsa_amd/csrc/seld_score.hip; statements in
 * seld_score.h).  pred_rows [n_files][pred_capacity][4] int16 (frame, class, azimuth, elevation in integer degrees; 8-byte aligned)
 * with pred_counts [n_files] -- what salsa_nn_seld_decode writes -- and gt_rows / gt_counts / gt_capacity in the same layout; rows
 * may come in any order.  n_seg = ceil(n_frames / label_rate) segments per file; record = file * n_seg + segment.  Outputs, every
 * element written: counters [records][10] int32 (TP FP FN S D I Nref DE_TP DE_FP DE_FN), total_de [records] float64, status
 * [records] int32: 0 scored; 1 doubt (in some frame another pairing costs within `margin` degrees of the best, or a slot average
 * lies within `margin` of doa_threshold -- the device's sin / cos / acos are not the host's bit for bit, so the host decides);
 * 2 refused (a (class, frame) cell with more than 4 DOAs on a side, or a count that is negative or above its capacity, in which
 * case no row of the file is read).  Records of status 1 and 2 carry zeros.  Distances are metrics.py::angular_distance_deg in
 * float64 without fma; the pairing is the minimum-total-cost injective map by brute force.  sum_counters [10] int64 and sum_de
 * [1] float64 (both or neither NULL) receive the status-0 records added up, total_de as one running sum in record order.
 * Bit-reproducible (no atomics).  Returns 0; -1, before any device call, for a NULL or misaligned pointer, n_files outside
 * 1 .. 65535, n_frames outside 1 .. 32767, a capacity < 1, label_rate or n_classes outside 1 .. 32, a NaN threshold or a margin that
 * is negative, NaN or infinite; -6 when a launch fails. */
int salsa_nn_seld_score(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows, const int *gt_counts,
                        int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes, double doa_threshold, double margin,
                        int *counters, double *total_de, int *status, int64_t *sum_counters, double *sum_de, void *hip_stream);
/* The same rows by the SELD 2020 metric: the counters of crnn/metrics.py::SeldMetrics2020.update (reference metrics/
 * SELD2020_evaluation_metrics.py:159-229, the scorer eval_version '2020' selects) per (file, segment).  Parameters, layouts, record
 * order, alignment rules, sums and return codes are salsa_nn_seld_score's; the same kernel bins the rows.  counters [records][10]
 * int32 are TP FP FN TN S D I Nref Nsys DE_TP (Nref / Nsys count the classes PRESENT in the segment), total_de [records] float64
 * the sum over the classes, in class order, of the mean cost of the class's common frames walked in ascending frame order; a
 * frame's cost is the least total distance over the injective maps of the smaller side into the larger, the best map's distances
 * added in reference-slot order.  status: 0 scored; 1 doubt -- some class average lies within `margin` of doa_threshold, the ONLY
 * doubt rule (a rival map of nearly equal cost is none: only the value of the minimum enters this metric); 2 refused as above.
 * Records of status 1 and 2 carry zeros; every output element is written.  Bit-reproducible (no atomics). */
int salsa_nn_seld_score2020(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows,
                            const int *gt_counts, int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes,
                            double doa_threshold, double margin, int *counters, double *total_de, int *status, int64_t *sum_counters,
                            double *sum_de, void *hip_stream);
/* The same rows by the class-wise SELD 2022 metric: the counters of crnn/metrics.py::SeldMetrics2022.update (the project's restatement
 * of the public DCASE 2022 metric) per (file, segment) AND per class.  The inputs, the record order, the
 * pairing, the doubt and refusal rules and the return codes are salsa_nn_seld_score's; the same kernel code bins the rows and books
 * the classes.  Outputs, every element written: class_counters [records][n_classes][5] int32 (TP Nref DE_TP DE_FP DE_FN; per class
 * FP == DE_FP, FN == DE_FN and FP_spatial == DE_TP - TP, so these five are all), class_de [records][n_classes] float64 (the class's
 * slot averages added from 0.0 in the order SeldMetrics2022 adds them; 8-byte aligned), sdi [records][3] int32 (S D I, formed per
 * segment over all classes), status [records] int32 as above.  Records of status 1 and 2 carry zeros.  file_counters
 * [n_files][n_classes][5] int64, file_de [n_files][n_classes] float64 and file_sdi [n_files][3] int64 (all three or none NULL;
 * 8-byte aligned) receive, per file, the file's status-0 records added up by a second kernel: every sum is one running sum in
 * segment order, and a file's sums depend on that file's records alone.  Bit-reproducible (no atomics). */
int salsa_nn_seld_score2022(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows,
                            const int *gt_counts, int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes,
                            double doa_threshold, double margin, int *class_counters, double *class_de, int *sdi, int *status,
                            int64_t *file_counters, double *file_de, int64_t *file_sdi, void *hip_stream);
/* salsa_nn_seld_score's distance statement alone: quads [n][4] int16 (azimuth1, elevation1, azimuth2, elevation2) -> out [n]
 * float64 degrees (tools/probe_score_distance.py measures its deviation from the host's, which sizes `margin`). */
int salsa_nn_seld_distance(const int16_t *quads, int64_t n, double *out, void *hip_stream);

/* The per-class SED threshold sweep (salsa_amd/csrc/seld_sweep.hip; statements in seld_sweep.h): the class-wise
 * SELD 2022 counters of K candidate thresholds per class, straight from the combined file outputs, in one launch.  act / xyz are
 * file-level float32 arrays on the device with n_in_frames >= n_frames frames per file, of which the first n_frames are decoded:
 * multi 0 -- act [n_files][n_in_frames][nc] activities and xyz [..][3 nc] (what salsa_nn_seld_decode writes to file_sed / file_xyz, or
 * a whole-clip forward); multi 1 -- act [..][3 C] track activities and xyz [..][9 C] (salsa_nn_chunk_merge_multi's or
 * salsa_nn_tta_merge_multi's outputs, or a forward), unified with cos_unify as salsa_nn_seld_decode_multi does.  thresholds [K][n_classes]
 * float32 on the device; gt_rows / gt_counts / gt_capacity as salsa_nn_seld_score2022 takes them.  record = file * n_seg + segment,
 * n_seg = ceil(n_frames / label_rate).
 *
 * For record r, candidate k and class c, class_counters [records][K][n_classes][5] int32 (TP Nref DE_TP DE_FP DE_FN) and class_de
 * [records][K][n_classes] float64 are the class-c entries of salsa_nn_seld_score2022's record for the rows salsa_nn_seld_decode_thr /
 * salsa_nn_seld_decode_multi_thr give at thresholds[k]: the same integer angles, distances, pairing and slot averages, class_de added
 * from 0.0 in the host's order.  status [records][K][n_classes] int32 is decided per (record, k, class), a class's counters depending
 * on its own rows alone: 1 doubt (in a common frame of the class another pairing costs within `margin` of the best, or a slot average
 * of the class lies within `margin` of doa_threshold), 2 refused (a reference cell of the class with more than 4 DOAs, or a gt count
 * that is negative or above gt_capacity, in which case no row of the file is read); such entries carry zeros and the host scores
 * them.  A cell is decoded and paired once per distinct predicted set (one for multi 0, at most seven for multi 1), never per
 * candidate.  file_counters [n_files][K][n_classes][5] int64 and file_de [n_files][K][n_classes] float64 (both or neither NULL)
 * receive each file's status-0 entries added up by a second kernel in segment order.  Every output element is written; no atomics:
 * bit-reproducible, and a file's entries do not depend on its batch.
 *
 * Returns 0; -1, before any device call and with the reason in salsa_last_error, for a NULL required pointer, a misaligned pointer (8
 * bytes for gt_rows and the 8-byte outputs, 4 otherwise), n_files outside 1 .. 65535, n_frames or n_in_frames outside 1 .. 32767,
 * n_in_frames < n_frames, gt_capacity < 1, n_classes or label_rate outside 1 .. 32, K outside 1 .. 64, multi not 0 / 1, with multi 1 a
 * cos_unify that is NaN or outside [-1, 1], a NaN doa_threshold, or a margin that is negative, NaN or infinite; -6 when a launch fails. */
int salsa_nn_seld_sweep(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames, int n_classes, int multi,
                        double cos_unify, const float *thresholds, int K, const int16_t *gt_rows, const int *gt_counts, int gt_capacity,
                        int label_rate, double doa_threshold, double margin, int *class_counters, double *class_de, int *status,
                        int64_t *file_counters, double *file_de, void *hip_stream);

/* Test-time augmentation and model ensembling around the forward (salsa_amd/csrc/tta.hip, statements in tta.h).
 * kind: 1 foa (V = 16 variants, 7 channels), 2 mic (V = 8, 7 channels), 3 gcc (V = 4, 10 channels) -- SALSA_BANK_FOA / _MIC / _GCC.
 * Variant v of foa / mic has the swap bits m[j] = (v >> j) & 1; of gcc: v = 0 no swap, v = 1, 2, 3 the one-hot m with bit v - 1 set.
 *
 * salsa_nn_tta_variant: d_out float32 dense [batch][C][n_frames][n_freq] = the channel swap of variant v applied to d_in, bit-equal
 * to the training augmentation's swap (salsa_augment_batch / salsa_augment_gcc_batch with no shift and no cutout: the same
 * per-element code).  d_in: float32 [batch][C][n_frames][n_freq] with dense (n_frames, n_freq) blocks and the given batch / channel
 * strides in elements (a time-cropped view needs no copy); not d_out.  16-byte accesses when n_frames * n_freq, both strides (and
 * for gcc n_freq) are multiples of four and both pointers are 16-byte aligned, 4-byte accesses otherwise.
 *
 * salsa_nn_tta_merge: the N = n_models * n_variants forward outputs in the slabs d_prob_slab [N][batch][label_frames][n_classes] and
 * d_xyz_slab [N][..][3 n_classes] (blocks x | y | z), slab n = model * n_variants + i holding the output for variant variant_ids[i]:
 * every xyz is rotated back by the inverse of the target swap of its variant (exact: selection and negation), then prob and xyz are
 * added in float32 in slab order starting from slab 0 and divided once by float(N), correctly rounded.  variant_ids is a HOST array
 * of n_variants <= 16 ids (any order, each in [0, V)); it is read during the call and travels in the kernel arguments.  Outputs
 * [batch][label_frames][n_classes] and [..][3 n_classes], every element written.  Bit-reproducible (no atomics).
 *
 * Both return 0; -1, before any device call and with the reason in salsa_last_error, for an unknown kind, a variant id outside
 * [0, V), N < 1, a NULL pointer, a non-positive or oversized shape, or input strides smaller than the block; -6 when the launch fails. */
int salsa_nn_tta_variant(const float *d_in, int64_t in_batch_stride, int64_t in_channel_stride, float *d_out, int batch, int n_frames,
                         int n_freq, int kind, int v, void *hip_stream);
int salsa_nn_tta_merge(const float *d_prob_slab, const float *d_xyz_slab, int n_models, const int *variant_ids, int n_variants, int kind,
                       int batch, int label_frames, int n_classes, float *d_prob_out, float *d_xyz_out, void *hip_stream);

/* Merging Multi-ACCDOA forwards of one clip after their tracks are aligned (track_merge 'align'; DESIGN.md section 9u;
 * salsa_amd/csrc/track_align.hip, statements in track_align.h).  C = n_real_classes, rows of 9 C vector columns (component (axis a,
 * track n, class c) at column (3 a + n) C + c) and 3 C activity columns (n C + c), float32 contiguous.  The tracks of a (row, class)
 * cell are an unordered set: an incoming cell V is permuted onto an anchor cell R by the candidate pi (012 021 102 120 201 210, the
 * k = 3 table of salsa_nn_adpit_loss) of least cost sum_n sum_a (R[n][a] - V[pi(n)][a])^2 -- one running float64 sum, tracks outer,
 * axes inner, no fma; a later candidate wins only when strictly smaller, so ties keep the lower index and a NaN cost keeps candidate 0.
 *
 * salsa_nn_tta_merge_multi: the N = n_models * n_variants slabs d_xyz_slab [N][batch][label_frames][9 C], ordered and un-swapped as
 * salsa_nn_tta_merge's (per column, so per track).  Slab 0 is the anchor; every later slab is aligned to slab 0 alone; the permuted
 * vectors are added in float32 in slab order starting from slab 0 and divided once by float(N), correctly rounded.  d_xyz_out
 * [batch][label_frames][9 C]; d_act_out [..][3 C] = the lengths of the merged vectors as salsa_nn_accdoa_sed forms them; d_perm_out,
 * when not NULL, [N][batch][label_frames][C] int32 receives the chosen candidates (0 for slab 0).  variant_ids is a HOST array.
 *
 * salsa_nn_chunk_merge_multi: chunk outputs d_act [n_files][n_chunks][chunk_len][3 C] and d_xyz [..][9 C] -> file outputs d_file_act
 * [n_files][n_frames][3 C] and d_file_xyz [..][9 C], what salsa_nn_seld_decode_multi takes.  The walk is salsa_nn_seld_decode's (same
 * starts, leftover chunk and trimming), per cell: chunk 0 and the frames of a chunk behind its first chunk_len - chunk_hop overwrite;
 * otherwise the fresh cell is aligned to the running one and v = (v + fresh[pi]) / 2.0f per component, the three activities with the
 * same pi.  With chunk_hop == chunk_len or one chunk no arithmetic is done: plain placement.
 *
 * One launch each, no atomics, no scratch: bit-reproducible, and a clip's result does not depend on its batch.  Both return 0; -1,
 * before any device call and with the reason in salsa_last_error, for a NULL required pointer, an unknown kind, a variant id outside
 * [0, V), N < 1 or more than 16 variant ids, a count below 1, a slab, chunk or output array beyond int32 indexing, n_chunks different
 * from the number of starts, or chunk_hop > chunk_len or chunk_len > n_frames with more than one chunk; -6 when the launch fails. */
int salsa_nn_tta_merge_multi(const float *d_xyz_slab, int n_models, const int *variant_ids, int n_variants, int kind, int batch,
                             int label_frames, int n_real_classes, float *d_xyz_out, float *d_act_out, int *d_perm_out, void *hip_stream);
int salsa_nn_chunk_merge_multi(const float *d_act, const float *d_xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop,
                               int n_frames, int n_real_classes, float *d_file_act, float *d_file_xyz, void *hip_stream);

/* The decoder's frequency mean (reference models/decoders.py: x.mean(dim=3) then (B, C, T) -> (B, T, C)) in one pass:
 * x bf16 channels-last [N][H][W][C] -> float32 y [H][N][C] (time_major != 0: the GRU scans' order) or [N][H][C]; C % 8 == 0.
 * _bwd: dx[n][h][w][c] = g[row(n, h)][c] / W, bf16 channels-last. */
int salsa_nn_freq_mean_fwd(const void *x, float *y, int64_t N, int H, int W, int C, int time_major, void *hip_stream);
int salsa_nn_freq_mean_bwd(const float *g, void *dx, int64_t N, int H, int W, int C, int time_major, void *hip_stream);

/* The decoder's freq_pool 'max' and 'avg_max' (reference models/decoders.py: torch.max(x, dim=3), and torch.mean + torch.max) in
 * one pass, next to the mean above: x bf16 channels-last [N][H][W][C] -> float32 y and uint8 argmax, both [H][N][C] (time_major
 * != 0) or [N][H][C]; C % 8 == 0, 1 <= W <= 255.  mode 1 (max): y = the maximum over w, exact (a bf16 value widened to float32).
 * mode 2 (avg_max): y = mean + max, the mean accumulated in float32 in w order as salsa_nn_freq_mean_fwd does.
 * Ties: argmax is the LOWEST w holding the maximum.  NaN: a NaN is greater than every number, so y is NaN and argmax the FIRST
 * NaN's w.  _bwd: dx[n][h][w][c] = g[row][c] / W (mode 2 only) + g[row][c] * (w == argmax[row][c]), written as bf16.
 * Both return 0, -1 for invalid arguments, -6 when the launch fails. */
int salsa_nn_freq_pool_fwd(const void *x, float *y, uint8_t *argmax, int64_t N, int H, int W, int C, int mode, int time_major,
                           void *hip_stream);
int salsa_nn_freq_pool_bwd(const float *g, const uint8_t *argmax, void *dx, int64_t N, int H, int W, int C, int mode, int time_major,
                           void *hip_stream);

/* Column sums of one or two float32 row-major [M][C] matrices, ADDED to out_a / out_b (zero them first; b may be NULL): the GRU's
 * bias gradients db_ih = sum_(t,b) dgi, db_hh = sum_(t,b) dgh in one launch (torch's reduction / a ones-vector GEMV: ~17 us each).
 * M <= 65535 * 64 (one workgroup row per 64 matrix rows); more is -1, before any launch. */
int salsa_nn_colsum2(const float *a, const float *b, float *out_a, float *out_b, int64_t M, int C, void *hip_stream);

/* Deterministic weight gradients (round 4).  Every weight-gradient kernel (salsa_nn_conv3x3_c64_wrw, _stem_wrw, _stem_wrw_bn,
 * _wide_wrw, salsa_nn_conv1x1_wrw) and salsa_nn_colsum2 is a reduction over pixels split across workgroups.  By default the
 * workgroups combine their float32 partial sums with atomic adds: the order of arrival decides the rounding, so two identical
 * training steps differ in the last bits.  salsa_nn_set_deterministic(ws, bytes) with a device workspace switches all of them to
 * partial SLABS (every workgroup stores its partial sums into its own slab of `ws`) followed by one reduction launch that adds the
 * slabs in slab order -- bit-identical results run to run, at the price of the slab traffic (<= 76 MB per call) and one more
 * launch per call.  The workspace is registered FOR THE DEVICE THAT IS CURRENT at the call (one per device; memory of another
 * device is refused with -1) and every launcher uses the workspace of the device current at ITS call -- a device without one keeps
 * the atomics.  ws = NULL switches every device back to atomics.  The calls return -5 when `bytes` is too small for a shape
 * (SALSA_NN_DET_WS_BYTES covers every layer of the SELD CRNN at the bench's sizes).  On one device the workspace is shared by all
 * calls: use one stream at a time, as the trainer does (two backward passes racing on two streams of one device need the atomics).
 * salsa_nn_get_deterministic: 1 when the current device has a workspace. */
#define SALSA_NN_DET_WS_BYTES ((size_t)160 << 20)
int salsa_nn_set_deterministic(void *ws, size_t bytes);
int salsa_nn_get_deterministic(void);

/* One Adam step over MANY parameter tensors in one launch (round 4) -- torch.optim.Adam's update rule (its fused CUDA kernel,
 * ADAM_MODE ORIGINAL, amsgrad off; the reference's optimiser, experiments/configs/seld.yml:37-52 through Lightning):
 *     g += weight_decay p;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *     p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * all float32.  torch's own fused path takes three multi_tensor_apply launches for this network's 143 tensors, two of them ~40
 * workgroups of tiny tensors (0.165 ms per step for 0.39 GB of traffic).
 *   table  device array [n_tensors] of {float *p, *m, *v; int64 n} (salsa_nn_adam_entry): stable from step to step;
 *   grads  HOST array [n_tensors] of device pointers to the gradients (they move from step to step: passed in the kernel arguments);
 *   chunks device array [n_chunks] of {int tensor, int first element / SALSA_NN_ADAM_CHUNK}: one workgroup each;
 * at most SALSA_NN_ADAM_MAX_TENSORS tensors per call.  Returns 0, -1 on bad arguments. */
#define SALSA_NN_ADAM_MAX_TENSORS 192
#define SALSA_NN_ADAM_CHUNK 8192
typedef struct { float *p, *m, *v; int64_t n; } salsa_nn_adam_entry;
int salsa_nn_adam_step(const salsa_nn_adam_entry *table, const float *const *grads, int n_tensors, const int *chunks, int n_chunks,
                       double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *hip_stream);

/* The decoder's optional self-attention stage (salsa_amd/csrc/attention.hip), all float32 with products exact in
 * float32.  Attention core of one multi-head self-attention:
 *     S_ij = q_i . k_j / sqrt(head_dim),  P = softmax_j(S),  o_i = sum_j P_ij v_j,  lse_i = ln sum_j exp(S_ij)
 *   qkv  (B, T, 3, n_heads, head_dim) contiguous: the in-projection's output as it is;   out  (B, T, n_heads * head_dim);
 *   lse  (B, n_heads, T);   d_qkv as qkv.  No mask, no dropout on P.
 * _bwd recomputes P from lse (no T x T plane is stored): with delta_i = d_o_i . o_i and dS = P o (d_o V^T - delta),
 *     dQ = dS K / sqrt(head_dim),  dK = dS^T Q / sqrt(head_dim),  dV = P^T d_o.
 * Every output element is summed by one workgroup in a fixed order (no atomics): both passes are bit-reproducible and a sample's
 * result does not depend on the rest of the batch.  Supported: head_dim 32 or 64, 1 <= n_heads <= 65535, 1 <= T <= 512, 1 <= B <=
 * 65535 (salsa_nn_attn_supported: 1 or 0).  The launchers return 0, -1 for an unsupported shape or a null pointer (before any
 * device call), -6 when the launch fails. */
int salsa_nn_attn_supported(int T, int n_heads, int head_dim);
int salsa_nn_attn_fwd(const float *qkv, float *out, float *lse, int B, int T, int n_heads, int head_dim, void *hip_stream);
int salsa_nn_attn_bwd(const float *qkv, const float *out, const float *lse, const float *d_out, float *d_qkv,
                      int B, int T, int n_heads, int head_dim, void *hip_stream);

/* y = LayerNorm(x + res) over the last axis of float32 [M][C] rows, C = 256 or 512: biased variance, eps inside the square root (as
 * torch), two-pass statistics; mean / rstd [M] are kept for the backward.  _bwd: dx [M][C] is the gradient of x AND of res (one
 * output serves both); dgamma / dbeta [C] are reduced in a fixed order (per-workgroup partial sums into `ws`, then one ordered pass):
 * bit-reproducible for a given M (not across a reordering of the rows).  ws: salsa_nn_add_layernorm_ws_bytes(M, C) bytes (0 for an
 * unsupported shape).  Return 0, -1 for bad arguments or a null pointer (before any device call), -5 when ws_bytes is too small,
 * -6 when the launch fails. */
size_t salsa_nn_add_layernorm_ws_bytes(int64_t M, int C);
int salsa_nn_add_layernorm_fwd(const float *x, const float *res, const float *gamma, const float *beta, float *y,
                               float *mean, float *rstd, int64_t M, int C, float eps, void *hip_stream);
int salsa_nn_add_layernorm_bwd(const float *dy, const float *x, const float *res, const float *gamma, const float *mean,
                               const float *rstd, float *dx, float *dgamma, float *dbeta, void *ws, size_t ws_bytes,
                               int64_t M, int C, void *hip_stream);

/* The decoder's optional Conformer blocks (salsa_amd/csrc/conformer.hip): everything of a block but its GEMMs and
 * the attention core above.  All float32; no atomics, every sum in a fixed order: bit-reproducible for a given shape, and a sample's
 * result does not depend on the rest of the batch, with one exception: a dropout mask depends on the element's flat index.
 * Dropout (drop_p, drop_seed) is the element-wise BatchNorm dropout's (salsa_nn_bn_train_fwd): p quantised to thresh = round(65536 p)
 * (at most 65535), one 32-bit hash of (flat index / 2, seed) serves two neighbouring elements -- the even one takes the low 16 bits --
 * an element is dropped when its 16 bits < thresh and kept ones are scaled by 65536 / (65536 - thresh); the flat index is the element's
 * in the tensor the mask applies to, which must have fewer than 2^32 elements.  No mask is stored: a backward regenerates it from the
 * same (drop_p, drop_seed).  0 <= drop_p < 1.  Every launcher returns 0, -1 for an unsupported shape, a bad argument or a missing
 * pointer (before any device call), -5 when ws_bytes is too small, -6 when a launch fails; every _ws_bytes is 0 for an unsupported
 * shape.
 *
 * Pre-norm residual step on [M][C] rows, C = 256 or 512, M >= 1, M C < 2^32 (salsa_nn_res_layernorm_supported):
 *     z = x + scale * drop(branch),   y = LayerNorm(z) * gamma + beta   (biased variance, eps inside the square root)
 *   branch NULL: z = x (drop_p and scale unused).  z_out NULL: z is not written.  y_out NULL: no LayerNorm (gamma, beta, mean, rstd
 *   unused and may be NULL); with y_out all four are required, and mean / rstd [M] are kept for the backward.  One of z_out / y_out
 *   is required.  Where the mask drops, z is x bit for bit.  With scale 1, drop_p 0 and a branch, y, mean and rstd are
 *   salsa_nn_add_layernorm_fwd's bits on the same operands (the same two-pass statistics).
 * _bwd: dy is the gradient of y (NULL when there was no y_out), dz_in the gradient that reaches z directly (NULL: none); one of them is
 *   required.  x, branch, scale, drop_p, drop_seed as in the forward (z is recomputed).
 *     dx = dz_in + LayerNorm_backward(dy),   dbranch = scale * mask * dropscale * dx   (dbranch NULL: not written),
 *   dgamma / dbeta [C] through per-workgroup slabs in ws and one ordered pass (with dy: gamma, mean, rstd, dgamma, dbeta and ws of
 *   salsa_nn_res_layernorm_ws_bytes(M, C) are required; without dy they are unused). */
int salsa_nn_res_layernorm_supported(int64_t M, int C);
size_t salsa_nn_res_layernorm_ws_bytes(int64_t M, int C);
int salsa_nn_res_layernorm_fwd(const float *x, const float *branch, float scale, float drop_p, uint32_t drop_seed,
                               const float *gamma, const float *beta, float *z_out, float *y_out, float *mean, float *rstd,
                               int64_t M, int C, float eps, void *hip_stream);
int salsa_nn_res_layernorm_bwd(const float *dy, const float *dz_in, const float *x, const float *branch, float scale, float drop_p,
                               uint32_t drop_seed, const float *gamma, const float *mean, const float *rstd, float *dx,
                               float *dbranch, float *dgamma, float *dbeta, void *ws, size_t ws_bytes, int64_t M, int C,
                               void *hip_stream);

/* The feed-forward epilogue on [M][C], C a multiple of 4 and <= 4096, M C < 2^32:  h = drop(swish(a + bias)),  swish(v) = v sigmoid(v).
 * THE BIAS ENTERS HERE: the caller's GEMM runs without one (F.linear(n, W1, None)) and this kernel adds W1's bias, so that the bias
 * gradient is this file's fixed-order column sum and no separate reduction over the rows is launched.  bias NULL: a already holds it.
 * _bwd: da = dh * mask * dropscale * swish'(a + bias), swish'(v) = s (1 + v (1 - s)), s = sigmoid(v) (recomputed from a);
 * dbias [C] = the column sum of da, through slabs in ws (salsa_nn_bias_swish_dropout_ws_bytes(M, C)) and one ordered pass; dbias NULL:
 * not produced and ws unused. */
int salsa_nn_bias_swish_dropout_supported(int64_t M, int C);
size_t salsa_nn_bias_swish_dropout_ws_bytes(int64_t M, int C);
int salsa_nn_bias_swish_dropout_fwd(const float *a, const float *bias, float *h, int64_t M, int C, float drop_p, uint32_t drop_seed,
                                    void *hip_stream);
int salsa_nn_bias_swish_dropout_bwd(const float *dh, const float *a, const float *bias, float *da, float *dbias, void *ws,
                                    size_t ws_bytes, int64_t M, int C, float drop_p, uint32_t drop_seed, void *hip_stream);

/* The convolution module between its two pointwise GEMMs:  u = swish(LayerNorm(DW(glu(a))) * gamma + beta)
 *   a (B, T, 2 d): glu(a) = first half * sigmoid(second half);  DW: depthwise convolution along T per sample, `kernel` taps, zero
 *   padding kernel / 2 at both ends, out[t][c] = dw_bias[c] + sum_k dw_weight[c][k] glu[t - kernel / 2 + k][c], dw_weight [d][kernel]
 *   (nn.Conv1d(d, d, kernel, groups=d)'s weight);  LayerNorm over the d channels;  u (B, T, d).
 * Supported: d = 256 or 512, 1 <= T <= 512, kernel odd in 3 .. 31, 1 <= B <= 65535 (salsa_nn_conv_module_supported).  One workgroup
 * owns SALSA_NN_CONV_MODULE_TILE time steps of one sample in the forward and in the data gradient.
 * _bwd recomputes the activations from a (nothing but a is kept): da (B, T, 2 d), d_dw_weight [d][kernel], d_dw_bias, dgamma, dbeta
 * [d]; the four parameter gradients through per-workgroup slabs and one ordered pass.  ws: salsa_nn_conv_module_ws_bytes(B, T, d,
 * kernel) bytes (the gradient at the depthwise output, (B, T, d), and the slabs).  Three launches. */
#define SALSA_NN_CONV_MODULE_TILE 16
int salsa_nn_conv_module_supported(int T, int d, int kernel);
size_t salsa_nn_conv_module_ws_bytes(int B, int T, int d, int kernel);
int salsa_nn_conv_module_fwd(const float *a, const float *dw_weight, const float *dw_bias, const float *gamma, const float *beta,
                             float *u, int B, int T, int d, int kernel, float eps, void *hip_stream);
int salsa_nn_conv_module_bwd(const float *du, const float *a, const float *dw_weight, const float *dw_bias, const float *gamma,
                             const float *beta, float *da, float *d_dw_weight, float *d_dw_bias, float *dgamma, float *dbeta,
                             void *ws, size_t ws_bytes, int B, int T, int d, int kernel, float eps, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
