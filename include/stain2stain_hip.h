/* stain2stain_hip.h -- C ABI of libstain2stain_hip.so (gfx950 / MI355X only).
 *
 * The reference (nirschl-lab/stain2stain) has no FFI: its hot path is stock torch.nn layers selected
 * through Hydra `_target_` strings (configs/model/*.yaml).  These entry points are therefore
 * build-defined; each one names the reference computation it replaces.  The Python classes in
 * stain2stain_amd/ (same constructor signatures and state_dict keys as the reference's
 * SharedEncoder / FlowMatchingDecoder / TimeEmbedding) bind them through ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success or a negative S2S_ERR_* code; nothing throws across the ABI
 *   - all pointers are DEVICE pointers unless stated otherwise; the caller owns every buffer,
 *     kernels never allocate; `stream` is a hipStream_t passed as void*
 *   - dtype: S2S_BF16 (0) = bf16 tensors, bf16 MFMA, fp32 accumulate;
 *            S2S_F32 (1)  = fp32 tensors; MFMA products formed from a 3-way bf16 split (6 MFMAs, fp32-grade)
 *   - activation tensors are NHWC "views": element (n,h,w,c) lives at base[((n*H+h)*W+w)*ld + c];
 *     ld (pixel stride, elements) lets a channel slice of a wider buffer be used in place.
 *     Channel counts and ld must be multiples of 8, base pointers 16-byte aligned.
 *   - the image tensors at the network boundary are NCHW contiguous fp32 (the reference's layout).
 */
#ifndef STAIN2STAIN_HIP_H
#define STAIN2STAIN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define S2S_OK 0
#define S2S_ERR_SHAPE (-1)
#define S2S_ERR_ALIGN (-2)
#define S2S_ERR_DTYPE (-3)
#define S2S_ERR_LAUNCH (-4)
#define S2S_ERR_NULL (-5)

#define S2S_BF16 0
#define S2S_F32 1

/* ---- 3x3 convolution, MFMA implicit GEMM (conv3x3_mfma.hip) -------------------------------------
 * nn.Conv2d(k=3, padding=1) of DoubleConv: src/models/components/shared_encoder.py:15,18,
 * task_decoders.py:15,18.  Input = channels [0,c0) of x0 followed by [0,c1) of x1 (x1 may be NULL with
 * c1 = 0): the torch.cat([skip, up], dim=1) of task_decoders.py:49 without the copy.
 * w_packed: s2s_pack_conv3x3 output (forward layout for the forward pass, dgrad layout + swapped channel
 * roles for the data gradient).  stat_part (optional): float[2][Cout][s2s_conv3x3_stat_blocks()] partial
 * (sum, sum of squares) of the stored values per output channel and producing workgroup, for BatchNorm
 * (channel-major, the layout s2s_bn_finalize reads).  ep_scale/ep_shift
 * (optional, both or neither) and relu: y = relu?((acc + bias) * scale + shift) -- eval-mode BatchNorm
 * folded into the epilogue.  relu without scale/shift: y = relu(acc + bias), in bf16 and in fp32 alike, with
 * statistics (of the values as stored) and with a split-K workspace too; such a bf16 launch runs on the per-tap
 * kernel (the plan of the same launch with a bias) and may store a zero as -0. */
int s2s_conv3x3_stat_blocks(int dtype, int B, int H, int W, int Cout);
int s2s_conv3x3_nhwc(int dtype, const void* x0, int ld0, int c0, const void* x1, int ld1, int c1,
                     const void* w_packed, const float* bias, void* y, int ldy, float* stat_part,
                     const float* ep_scale, const float* ep_shift, int relu, int B, int H, int W, int Cout,
                     void* stream);

/* Diagnostic: with S2S_CONV_DBG=64 in the environment the bf16 kernel's workgroups record the shader-clock counter and
 * the 100 MHz wall clock at entry and exit; this copies {clk0, clk1, wall0, wall1} of the first n <= 8192 workgroups of
 * the last launch into a HOST buffer (scripts/clk_probe.py turns them into the MHz the kernel ran at). */
/* The same with a split-K workspace (optional): kwork = float[s2s_conv3x3_ksplit()][B*H*W][Cout]; when the launch
 * carries no statistics and has few output tiles (sampling one tile at a time) the 32-channel chunks are shared by
 * several workgroups and a second launch folds the fp32 partial tiles (+ bias, folded affine, ReLU). */
int s2s_conv3x3_ksplit(int dtype, int B, int H, int W, int Cout, int cin);
int s2s_conv3x3_nhwc_k(int dtype, const void* x0, int ld0, int c0, const void* x1, int ld1, int c1,
                       const void* w_packed, const float* bias, void* y, int ldy, float* stat_part,
                       const float* ep_scale, const float* ep_shift, int relu, float* kwork, int B, int H, int W,
                       int Cout, void* stream);
/* Rows of BatchNorm partial sums a training-step launch of these operands writes (>= 1): s2s_conv3x3_stat_blocks() of
 * them, or one per (workgroup, wave row) when the launch runs on a persistent kernel that carries the sums over a
 * workgroup's tiles in registers (the staged kernel; the per-tap persistent kernel with a single channel tile).  Size
 * stat_part as float[2][Cout][rows] and hand `rows` to s2s_conv3x3_nhwc_s (stat_rows = 0: the per-tile count). */
int s2s_conv3x3_stat_rows(int dtype, int B, int H, int W, int Cout, int c0, int c1, int ld0, int ld1, int has_bias);
/* Which kernel family a bias-free training-step launch of these operands runs on: 0 = the per-tap kernels (one barrier
 * per filter tap), 1 = conv3x3_stage_kernel streaming its weights per 32-channel chunk, 2 = the same with the filter
 * resident in LDS (<= 64 input channels).  Diagnostic: tests and scripts assert the path they mean to measure. */
int s2s_conv3x3_staged(int dtype, int B, int H, int W, int Cout, int c0, int c1, int ld0, int ld1, int ldy, int stats);
/* Diagnostic: the kernel family the launch s2s_conv3x3_nhwc_s makes of these operands (stat_rows as passed to it; kwork
 * = a split-K workspace is offered, as s2s_conv3x3_nhwc_k with kwork): 0 = conv3x3_stage_kernel with the filter resident,
 * 1 = the same streaming the filter, 2 = the persistent per-tap kernel carrying statistics per workgroup, 3 = the same
 * with per-tile statistics or none, 4 = one tile per workgroup (split-K possible), 5 = the fp32 parity kernel; negative:
 * the launch is refused.  Tests pin the kernel a case was written for with it. */
int s2s_conv3x3_family(int dtype, int B, int H, int W, int Cout, int c0, int c1, int ld0, int ld1, int ldy, int has_bias,
                       int has_affine, int stats, int stat_rows, int kwork);
/* Diagnostic: the whole plan behind s2s_conv3x3_family, from the host code the launch itself dispatches on (nothing is
 * launched): out[9] = {family, cfg, gx, gy, grid, xsp, xsn, ksplit, stat_rows}.  cfg: the tile, bf16 0..7 = 8x32x128,
 * 8x32x64, 4x32x128, 4x32x64, 16x16x128, 16x16x64, 8x16x128, 8x16x64 (rows x columns x channels), fp32 0 = 4x32x64,
 * 1 = 8x16x64; the staged families tile 16x32x64 whatever cfg says.  gx x gy: pixel tiles x channel tiles of the
 * family's tile.  grid: workgroups of the staged and persistent families (0: the launch is gx x gy x ksplit).  xsp x xsn:
 * the XCD cut (0 x 1: plain order; the staged families report 8 x 1 or 0 x 1).  stat_rows: rows per channel of
 * stat_part.  Returns 0, or the negative status of a refused launch. */
int s2s_conv3x3_plan(int dtype, int B, int H, int W, int Cout, int c0, int c1, int ld0, int ld1, int ldy, int has_bias,
                     int has_affine, int stats, int stat_rows, int kwork, int* out);
int s2s_conv3x3_nhwc_s(int dtype, const void* x0, int ld0, int c0, const void* x1, int ld1, int c1, const void* w_packed,
                       const float* bias, void* y, int ldy, float* stat_part, int stat_rows, const float* ep_scale,
                       const float* ep_shift, int relu, float* kwork, int B, int H, int W, int Cout, void* stream);
int s2s_debug_conv_clock(long* out_host, int n);

/* ---- 3x3 convolution weight gradient (conv3x3_wgrad_mfma.hip) -----------------------------------
 * autograd's conv2d weight gradient for the same layers.  part: float[splits][9][Cout][c0+c1] scratch;
 * grad_oihw: float[Cout][c0+c1][3][3], overwritten or accumulated. */
int s2s_conv3x3_wgrad_splits(int dtype, int B, int H, int W, int Cin, int Cout);
/* diagnostic: the launch plan of s2s_conv3x3_wgrad_nhwc for this problem, from the launcher's own host code.
 * what: 0 = splits, 1 = 8x16 pixel tiles, 2 = XCD-aware workgroup order (0 / 1), 3 = waves per fold group (4 / 16),
 * 4 = kernel (0 = bf16 DMA, 1 = fp32 register-staged); a negative status for a shape / dtype the launch refuses. */
int s2s_conv3x3_wgrad_plan(int dtype, int B, int H, int W, int Cin, int Cout, int what);
int s2s_conv3x3_wgrad_nhwc(int dtype, const void* dy, int lddy, int Cout, const void* x0, int ld0, int c0,
                           const void* x1, int ld1, int c1, float* part, float* grad_oihw, int accumulate,
                           int B, int H, int W, void* stream);
/* the same in two launches: phases = 1 the split MFMA kernel (slabs into part), 2 the fold into grad_oihw, 3 both */
int s2s_conv3x3_wgrad_phase(int dtype, const void* dy, int lddy, int Cout, const void* x0, int ld0, int c0,
                            const void* x1, int ld1, int c1, float* part, float* grad_oihw, int accumulate,
                            int B, int H, int W, int phases, void* stream);
/* tests and A/B only: variant 0 = the product kernel, 1 = the bf16 loop it replaced (same bits) */
int s2s_conv3x3_wgrad_phase_variant(int dtype, const void* dy, int lddy, int Cout, const void* x0, int ld0, int c0,
                                    const void* x1, int ld1, int c1, float* part, float* grad_oihw, int accumulate,
                                    int B, int H, int W, int phases, int variant, void* stream);

/* ---- stem and head (conv_edge.hip) ----------------------------------------------------------------
 * stem: first conv of SharedEncoder.inc (shared_encoder.py:15,67), NCHW fp32 image (Cin <= 6: RGB, or RGB + the
 *       mask channel of conditional_flow_matching_conditional_mask.py:62-64) -> NHWC.
 * head: FlowMatchingDecoder.outc / SegmentationDecoder.outc, Conv2d(k=1) to Cout <= 8 (task_decoders.py:100,132,169),
 *       NHWC -> NCHW fp32; the fused head+loss entry point takes Cout <= 4. */
int s2s_stem_stat_blocks(int B, int H, int W);
int s2s_stem_conv3x3_fwd(int dtype, const float* x_nchw, const float* w_oihw, const float* bias, void* y, int ldy,
                         float* stat_part, int B, int H, int W, int Cin, int Cout, void* stream);
int s2s_stem_wgrad_blocks(int B, int H, int W);
/* part: float[ceil(Cin/3)][2*blocks][Cout][32]; dbias may be NULL */
int s2s_stem_conv3x3_wgrad(int dtype, const void* dy, int lddy, const float* x_nchw, float* part, float* dw_oihw,
                           float* dbias, int accumulate, int B, int H, int W, int Cin, int Cout, void* stream);
/* test-facing: the kernel that the pipelined bf16 kernel replaced (fp32: the same launch); same arguments, same bits */
int s2s_stem_conv3x3_wgrad_ref(int dtype, const void* dy, int lddy, const float* x_nchw, float* part, float* dw_oihw,
                               float* dbias, int accumulate, int B, int H, int W, int Cin, int Cout, void* stream);
/* test-facing, no launch: which kernel the launch takes (0 the reference kernel, 1 the pipelined one: LDS-DMA for dY,
 * double-buffered; < 0 the launch's error); reference != 0: as the _ref entry point chooses */
int s2s_stem_wgrad_family(int dtype, int lddy, int B, int H, int W, int Cin, int Cout, int reference);
/* diagnostic: the kernels s2s_head_conv1x1_fwd (forward = 1) / _bwd (forward = 0) take, from their own dispatch: 1 ... 64 =
 * the lane-per-piece form with that many lanes per pixel (C = 8 lanes), 104 / 108 = the one-thread-per-pixel kernels
 * with 4 / 8 outputs; a negative status for a launch that is refused (Cout > 8; backward: Cout (C + 1) > 2048). */
int s2s_head_family(int dtype, int B, int H, int W, int C, int Cout, int forward);
int s2s_head_conv1x1_fwd(int dtype, const void* x, int ldx, const float* w, const float* bias, float* y_nchw, int B,
                         int H, int W, int C, int Cout, void* stream);
int s2s_head_wgrad_blocks(int B, int H, int W);
/* part: float[blocks][Cout][C+1] */
int s2s_head_conv1x1_bwd(int dtype, const float* dy_nchw, const void* x, int ldx, const float* w, void* dx, int lddx,
                         float* part, float* dw, float* dbias, int accumulate, int B, int H, int W, int C, int Cout,
                         void* stream);

/* head + loss + their backward in one pass over the last activation (training step only):
 * v = W a + b (optional output), loss = mean((v-u)^2), dx = W^T dv, dW/db with dv = 2 (v-u) grad_scale / count
 * (task_decoders.py:132 + conditional_flow_matching.py:72).  part: float[blocks][Cout][C+1]; lpart: double[blocks] */
int s2s_head_loss_blocks(int B, int H, int W);
/* test-facing, no launch: the kernel s2s_head_loss_fused takes, from its own dispatch: 1 ... 64 = the lane-per-piece kernel
 * with that many lanes per pixel (C = 8 lanes, a power of two), 100 = the one-thread-per-pixel kernel (any other
 * C % 8 == 0 up to 96); a negative status for a launch that is refused (Cout > 4, C % 8, C >= 104 off the lanes form) */
int s2s_head_loss_family(int dtype, int B, int H, int W, int C, int Cout);
int s2s_head_loss_fused(int dtype, const void* x, int ldx, const float* w, const float* bias, const float* u_nchw,
                        float* v_nchw, void* dx, int lddx, float grad_scale, float* part, double* lpart, float* dw,
                        float* dbias, float* loss, int accumulate, int B, int H, int W, int C, int Cout, void* stream);

/* fused tail of the training step: the last BatchNorm + ReLU, the head, the MSE loss, the head's backward and that
 * BatchNorm's backward in three passes that read the saved conv output `raw` (T, NHWC); neither the last activation nor
 * its gradient is stored, and the results are those of s2s_bn_relu_apply -> s2s_head_loss_fused -> s2s_bn_relu_bwd.  C = 8 * 2^k <= 512, Cout <= 4.  scale / shift / mean / invstd: s2s_bn_finalize's outputs.
 * s2s_tail_fwd_loss: g = dv (NCHW fp32 out), v optional, loss, head dW / db, dgamma / dbeta (conv_dbias, optional, is
 *   set to its exact value 0 unless accumulating) and the per-channel means of the BatchNorm backward in bnwork.
 *   part: float[blocks][Cout][C+1]; lpart: double[blocks], blocks = s2s_tail_blocks;
 *   bnwork: float[2*C*nb + 2*C], nb = s2s_bn_bwd_blocks(B, H, W, C)
 * s2s_tail_bwd_apply: dx = d raw (T, NHWC) from raw, g and bnwork. */
int s2s_tail_blocks(int B, int H, int W);
/* test-facing, no launch: the instantiation both tail entry points take, from their own dispatch: 256 MO + PCB, PCB = C / 8
 * lanes per pixel and MO = 3 (Cout <= 3) or 4 outputs covered by the loops; a negative status for a refused launch */
int s2s_tail_family(int dtype, int B, int H, int W, int C, int Cout);
int s2s_tail_fwd_loss(int dtype, const void* raw, int ldx, const float* scale, const float* shift, const float* mean,
                      const float* invstd, const float* w, const float* bias, const float* u_nchw, float* v_nchw,
                      float* g_nchw, float grad_scale, float* part, double* lpart, float* bnwork, float* dw,
                      float* dbias, float* loss, float* dgamma, float* dbeta, float* conv_dbias, int accumulate, int B,
                      int H, int W, int C, int Cout, void* stream);
int s2s_tail_bwd_apply(int dtype, const void* raw, int ldx, const float* g_nchw, const float* w, const float* scale,
                       const float* shift, const float* mean, const float* invstd, const float* gamma,
                       const float* bnwork, void* dx, int lddx, int B, int H, int W, int C, int Cout, void* stream);

/* ---- BatchNorm2d + ReLU (+ MaxPool2d(2)) (norm_act.hip) -------------------------------------------
 * nn.BatchNorm2d(eps 1e-5, momentum 0.1) -> nn.ReLU of DoubleConv (shared_encoder.py:16-20) and the
 * nn.MaxPool2d(2) of the following Down block (shared_encoder.py:33). */
int s2s_bn_finalize(const float* part, int nblk, int C, long count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, long* num_batches_tracked, float momentum, float eps,
                    float* mean, float* invstd, float* scale, float* shift, void* stream);
/* the same when the statistics were taken of the convolution WITHOUT its bias (conv_bias: [C] or NULL): mean / invstd /
 * scale / shift refer to the unbiased conv output the caller stores, the running mean is that of conv + bias, as
 * nn.BatchNorm2d behind nn.Conv2d(bias=True) keeps it (shared_encoder.py:15-16) */
int s2s_bn_finalize_b(const float* part, int nblk, int C, long count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, long* num_batches_tracked, float momentum, float eps,
                      float* mean, float* invstd, float* scale, float* shift, const float* conv_bias, void* stream);
int s2s_bn_eval_prepare(int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* scale, float* shift, void* stream);
/* y = relu(x*scale+shift); pool (optional) = 2x2/stride-2 max of y, floor mode */
int s2s_bn_relu_apply(int dtype, const void* x, int ldx, const float* scale, const float* shift, void* y, int ldy,
                      void* pool, int ldp, int B, int H, int W, int C, void* stream);
int s2s_maxpool2(int dtype, const void* x, int ldx, void* pool, int ldp, int B, int H, int W, int C, void* stream);
int s2s_bn_bwd_blocks(int B, int H, int W, int C);
/* g1: gradient wrt the ReLU output (may be NULL if gp given); gp: gradient wrt the pooled output (may be
 * NULL); scale/shift: the forward's folded affine (the ReLU output is recomputed from x, not read);
 * x: saved conv output; work: float[4*blocks*C + 2*C];
 * dbias_conv (optional): gradient of the preceding conv's bias = per-channel sum of dx, which the BatchNorm backward
 * makes identically zero; written as exact 0 (the reference's autograd sums rounding noise there).  With
 * S2S_BN_DBIAS_SUM=1 in the environment the sum is formed instead. */
int s2s_bn_relu_bwd(int dtype, const void* g1, int ldg1, const void* gp, int ldgp, const float* scale,
                    const float* shift, const void* x, int ldx, const float* mean, const float* invstd, const float* gamma, float* dgamma,
                    float* dbeta, float* dbias_conv, int accumulate, void* dx, int lddx, float* work, int B, int H,
                    int W, int C, void* stream);
/* SyncBatchNorm (Lightning's sync_batchnorm: True, configs/trainer/ddp.yaml:9 = torch.nn.SyncBatchNorm): statistics
 * over the GLOBAL batch.  Forward: s2s_bn_partial_sums folds the conv epilogue's partials into sums[2][C] (sum, sum of
 * squares), the host all-reduces them and calls s2s_bn_finalize on them (nblk = 1, count = global element count).
 * Backward: s2s_bn_relu_bwd_phase(phases = 1, count_total = global count) leaves (sum_dy, sum_dy_xhat) / count_total
 * in work[4 nb C .. + 2 C), the host all-reduces those 2 C floats, phases = 2 applies; phases = 3 with the local
 * count is s2s_bn_relu_bwd.  dgamma / dbeta stay rank-local sums (the gradient all-reduce averages them), as in torch. */
int s2s_bn_partial_sums(const float* part, int nblk, int C, float* sums, void* stream);
int s2s_bn_relu_bwd_phase(int dtype, const void* g1, int ldg1, const void* gp, int ldgp, const float* scale,
                          const float* shift, const void* x, int ldx, const float* mean, const float* invstd,
                          const float* gamma, float* dgamma, float* dbeta, float* dbias_conv, int accumulate, void* dx,
                          int lddx, float* work, int B, int H, int W, int C, long count_total, int phases, void* stream);

/* ---- bilinear x2, align_corners=True (+ F.pad to the skip size) (resample.hip) --------------------
 * nn.Upsample + F.pad of Up.forward (task_decoders.py:34,42-47); bias_nc (optional, float[B][C]) is added
 * to the input first: x = bottleneck + t[:, :, None, None] (task_decoders.py:119-125). */
int s2s_upsample2x_bilinear_ac_fwd(int dtype, const void* x, int ldx, const float* bias_nc, void* y, int ldy, int B,
                                   int Hin, int Win, int Hout, int Wout, int C, void* stream);
/* the up-sampling of relu(bn(x)) straight from the convolution's raw output x (scale / shift: float[C], rows 2 and 3 of
 * s2s_bn_finalize_b): s2s_bn_relu_apply followed by the entry point above, bit for bit, without the activation in
 * between.  Register-window shapes only (s2s_upsample2x_fwd_family == 1); others return the shape error. */
int s2s_upsample2x_bn_relu_fwd(int dtype, const void* x, int ldx, const float* scale, const float* shift,
                               const float* bias_nc, void* y, int ldy, int B, int Hin, int Win, int Hout, int Wout, int C,
                               void* stream);
/* test-facing: the row-sweep kernel that the production forward replaced; same arguments, same bits */
int s2s_upsample2x_bilinear_ac_fwd_ref(int dtype, const void* x, int ldx, const float* bias_nc, void* y, int ldy, int B,
                                       int Hin, int Win, int Hout, int Wout, int C, void* stream);
/* test-facing, no launch: which forward kernel the shape takes (0 row sweep, 1 the register-window kernel; < 0 the
 * launch's shape error); reference != 0: as the _ref entry point chooses */
int s2s_upsample2x_fwd_family(int ldx, int ldy, int B, int Hin, int Win, int Hout, int Wout, int C, int reference);
int s2s_upsample2x_bilinear_ac_bwd(int dtype, const void* dy, int lddy, void* dx, int lddx, int B, int Hin, int Win,
                                   int Hout, int Wout, int C, void* stream);
/* test-facing: the per-pixel window kernel that the production backward replaced; same arguments, same bits */
int s2s_upsample2x_bilinear_ac_bwd_ref(int dtype, const void* dy, int lddy, void* dx, int lddx, int B, int Hin,
                                       int Win, int Hout, int Wout, int C, void* stream);
/* test-facing, no launch: which backward kernel the shape takes (0 branching gather, 1 per-pixel window, 2 the 2 x 2
 * kernel; < 0 the launch's shape error); reference != 0: as the _ref entry point chooses */
int s2s_upsample2x_bwd_family(int lddy, int lddx, int B, int Hin, int Win, int Hout, int Wout, int C, int reference);
int s2s_pixel_sum(int dtype, const void* x, int ldx, float* out_nc, int B, int HW, int C, int accumulate,
                  void* stream);

/* ---- flow matching glue (flow.hip) --------------------------------------------------------------- */
/* TimeEmbedding.forward, shared_encoder.py:114-135 */
int s2s_time_embedding(const float* t, float* out, int B, int dim, void* stream);
/* nn.Linear / nn.SiLU of FlowMatchingDecoder.time_mlp, time_proj (task_decoders.py:82-89) */
int s2s_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, void* stream);
int s2s_linear_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int accumulate,
                   int B, int K, int N, void* stream);
int s2s_silu_fwd(const float* h, float* a, int n, void* stream);
int s2s_silu_bwd(const float* h, const float* da, float* dh, int n, void* stream);
/* xt = t*x1 + (1-t)*x0 + sigma*eps, ut = x1 - x0 (conditional_flow_matching.py:66; torchcfm 1.0.7) */
int s2s_cfm_sample(const float* x0, const float* x1, const float* t, const float* eps, float sigma, float* xt,
                   float* ut, int B, long per_sample, void* stream);
/* loss = mean((v-u)^2) (conditional_flow_matching.py:72); dv optional; work: double[1024] */
int s2s_mse_loss(const float* v, const float* u, float* dv, float grad_scale, float* loss, double* work, long count,
                 void* stream);
/* Scaled RMS error of an embedded Runge-Kutta step, the step-size control of the adaptive sampler that stands in for
 * torchdyn's dopri5 (conditional_flow_matching.py:157-170): out[0] = sqrt(mean((e / (atol + rtol max(|y0|,|y1|)))^2));
 * work: double[1024]. */
int s2s_ode_error_norm(const float* e, const float* y0, const float* y1, float atol, float rtol, float* out,
                       double* work, long n, void* stream);
int s2s_axpy(float* x, const float* y, float a, long n, void* stream);
/* ---- per-sample adaptive Dormand-Prince 5(4) (ode.hip) ---------------------------------------------------------
 * fp32 NCHW [B, n] tensors, n % 4 == 0, 16-byte aligned; state: double[B * 8] per-sample rows (t, h, accepted,
 * rejected, last-step-rejected, done, accept mask, aux); status: int[4] (active samples, step limit reached, attempted
 * steps, 0); part: double[2 * B * s2s_dp_partials(n)].  Nothing allocates or synchronises (capturable).
 * s2s_dp_init phase 0 (after k1 = v(0, y)): d0, d1, h0, t = 0, out = y + h0 k1, t_out = h0; phase 1 (after
 * fa = v(h0, out)): the first step h, counters, status.  s2s_dp_stage i = 1..6: out = y + sum_j (h a_ij) k_j,
 * t_out = float(t + c_i h) (i = 6 is y_new).  s2s_dp_error: per-sample scaled square sums of the error estimate;
 * s2s_dp_control: norm, accept / reject, t, h, counters, status; s2s_dp_commit: accepted samples y <- y_new, k1 <- k7. */
int s2s_dp_partials(long n);
int s2s_dp_init(int phase, const float* y, const float* k1, const float* fa, double* state, double* part, float* out,
                float* t_out, int* status, float atol, float rtol, int B, long n, void* stream);
int s2s_dp_stage(int i, const float* y, const float* k1, const float* k2, const float* k3, const float* k4,
                 const float* k5, const float* k6, const double* state, float* out, float* t_out, int B, long n,
                 void* stream);
int s2s_dp_error(const float* k1, const float* k2, const float* k3, const float* k4, const float* k5, const float* k6,
                 const float* k7, const float* y, const float* y_new, const double* state, double* part, float atol,
                 float rtol, int B, long n, void* stream);
int s2s_dp_control(double* state, const double* part, int* status, int max_steps, int B, long n, void* stream);
int s2s_dp_commit(float* y, const float* y_new, float* k1, const float* k7, const double* state, int B, long n,
                  void* stream);
/* ---- fixed-step explicit Runge-Kutta schemes with at most four stages (ode.hip) ------------------------------------
 * fp32 NCHW [B, n] tensors, n % 4 == 0, 16-byte aligned; table: float[table_len] node times, entry step * stages + i
 * the time of stage i of that step; counter: int[1], the current step.  Nothing allocates or synchronises (capturable).
 * s2s_rk_stage: out = x + sum_{j<nk} c_j k_j, each term acc = fma(c_j, k_j, acc) from acc = x in argument order (the
 * rounding of a copy of x followed by one s2s_axpy per term; the caller leaves zero coefficients out and passes
 * c_j = float(h a_ij)), and t_out[0..B) = table[counter * stages + stage].  out may be NULL when nk = 0: the launch
 * then writes the node time alone (the first stage evaluates on x itself).  s2s_rk_combine: x += sum_{j<nk} c_j k_j in
 * place, the same chain with c_j = float(h b_j), nk = 1..4, then counter += 1 from one thread (the only writer of the
 * counter; the stage kernel only reads it). */
int s2s_rk_stage(const float* x, const float* k1, const float* k2, const float* k3, float c1, float c2, float c3, int nk,
                 float* out, float* t_out, const float* table, const int* counter, int stages, int stage, int table_len,
                 int B, long n, void* stream);
int s2s_rk_combine(float* x, const float* k1, const float* k2, const float* k3, const float* k4, float c1, float c2,
                   float c3, float c4, int nk, int* counter, int B, long n, void* stream);
int s2s_fill_f32(float* x, float v, long n, void* stream);
/* t[0..n) <- table[*counter], then *counter += 1: the time input of a hipGraph-captured Euler step (the captured
 * kernel walks a table of the node times, so a replay needs no host-side argument). */
int s2s_euler_tick(float* t, int n, const float* table, int* counter, void* stream);

/* ---- optimiser, packing, layout (optim.hip) ------------------------------------------------------ */
/* torch.optim.Adam step over a flat fp32 buffer (configs/model/*.yaml:3-7) */
int s2s_adam_step(float* p, const float* g, float* m, float* v, long n, int step, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, void* stream);
/* the same step with its scalars in DEVICE memory, hyper[8] = {lr, beta1, beta2, eps, weight_decay, 1 - beta1^step,
 * sqrt(1 - beta2^step), grad_scale}: the launch a hipGraph-captured training step replays while the host refreshes the
 * eight floats (Lightning's optimizer.step() / scheduler surface, conditional_flow_matching.py:112-131) */
int s2s_adam_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, void* stream);
/* The same step over a list of tensors in one launch (ordinary module parameters + the gradients autograd left in .grad:
 * stain2stain_amd.FusedAdam, the optimiser of the drop-in path): desc = device long[ntensors][6] {p, g, m, v, n, first
 * block}; a tensor occupies s2s_adam_multi_blocks(n) blocks, total = their sum. */
long s2s_adam_multi_blocks(long n);
int s2s_adam_multi(const void* desc, int ntensors, long total, int step, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float grad_scale, void* stream);
/* Exponential moving average of the weights fused into the flat Adam pass: p, m, v exactly as s2s_adam_step /
 * s2s_adam_step_dev, then ema = lerp(ema, p_new, ema_weight) on the value just computed (torch.lerp's two-branch form).
 * ema_weight 1.0 copies (the first update of torch.optim.swa_utils.AveragedModel), 1 - decay averages.  p, g, m, v, ema
 * must be 16-byte aligned (S2S_ERR_ALIGN otherwise).  The _dev form reads the weight from device memory (*ema_weight),
 * so a captured step replays it unchanged. */
int s2s_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, long n, int step, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float grad_scale, float ema_weight, void* stream);
int s2s_adam_ema_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, const float* hyper,
                          const float* ema_weight, void* stream);
/* dst = lerp(dst, src, *weight) over a list of tensors in one launch (BatchNorm buffers of the fused trainers, every
 * parameter and buffer of stain2stain_amd.FusedEMA): desc = device long[ntensors][5] {dst, src, n, first block, kind},
 * kind 0 = fp32 lerp, 4 / 8 = copy of 4- / 8-byte integers (num_batches_tracked).  A tensor occupies
 * s2s_ema_multi_blocks(n) blocks (0 for an empty tensor, which then owns no block), total = their sum. */
long s2s_ema_multi_blocks(long n);
int s2s_ema_multi(const void* desc, int ntensors, long total, const float* weight, void* stream);
long s2s_pack_conv3x3_fwd_elems(int Cout, int Cin);
long s2s_pack_conv3x3_dgrad_elems(int Cout, int Cin);
int s2s_pack_conv3x3(int dtype, const float* w_oihw, void* w_fwd, void* w_dgrad, int Cout, int Cin, void* stream);
/* every conv layer in one launch; desc = device int64[nlayers][6] {w_oihw, w_fwd, w_dgrad, Cout, Cin, first 32x32 tile};
 * total = number of 32x32 (co,ci) tiles over all layers */
int s2s_pack_conv3x3_batched(int dtype, const void* desc, int nlayers, long total, void* stream);
int s2s_nchw_to_nhwc(int dtype, const float* x_nchw, void* y, int ldy, int B, int C, int H, int W, void* stream);
int s2s_nhwc_to_nchw(int dtype, const void* x, int ldx, float* y_nchw, int accumulate, int B, int C, int H, int W,
                     void* stream);

/* ---- paired input pipeline (input_pipeline.hip) -- SURVEY section 8 row f1 --------------------------
 * PairedDataset.__getitem__ transform chain (src/data/paired_data_module.py:170-199): shared crop + h/v flips,
 * to_tensor, Normalize(0.5, 0.5).  src/tgt: uint8 [B][Hs][Ws][3]; params: int32 [B][4] {top, left, hflip, vflip};
 * out: float [B][3][S][S]. */
int s2s_paired_crop_flip_normalize(const void* src_u8, const void* tgt_u8, const int* params, float* out_src,
                                   float* out_tgt, int B, int Hs, int Ws, int S, void* stream);
/* The use_augmentation=False branch (paired_data_module.py:200-211): TF.resize on a PIL image =
 * PIL.Image.resize((Wo, Ho), BILINEAR) -- Pillow's two-pass 22-bit fixed-point resampler with a uint8 intermediate
 * (Pillow src/libImaging/Resample.c) -- then to_tensor and Normalize(0.5, 0.5).  The coefficient tables (bounds:
 * int32 [out][2] = first input index, tap count; kk: int32 [out][ksize]) are Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc, built on the host (stain2stain_amd/data.py).  src: uint8 [B][Hs][Ws][3]; tmp: uint8
 * [B][Hs][Wo][3] scratch; out_u8 (optional): uint8 [B][Ho][Wo][3]; out_f (optional): float [B][3][Ho][Wo]. */
int s2s_pil_resize_bilinear_normalize(const void* src_u8, void* tmp_u8, const int* bounds_h, const int* kk_h,
                                      int ksize_h, const int* bounds_v, const int* kk_v, int ksize_v, void* out_u8,
                                      float* out_f, int B, int Hs, int Ws, int Ho, int Wo, void* stream);

/* ---- tiled whole-region translation (region.hip) -----------------------------------------------------
 * What runs between two sampler calls of stain2stain_amd.region.translate_region; no atomics, bit-reproducible.
 * s2s_region_gather: tiles out: float [B][3][T][T] = (u / 255 - 0.5) / 0.5 of a uint8 RGB image (row pitch `pitch`
 *   bytes, 3 contiguous bytes per pixel) whose buffer holds image rows [band_top, band_top + band_h) of an H x W image;
 *   origins: int32 [B][2] {top, left}.  Pixels outside the image fold back as numpy.pad(mode="reflect"); T % 4 == 0.
 * s2s_region_blend: adds tiles [n][c0][T][T] (+ tiles1 [n][c1][T][T], optional) into acc, a ring of band_rows image
 *   rows of C + 1 = c0 + c1 + 1 interleaved floats per pixel (row r at r % band_rows): C sums of w * v and the sum of
 *   w, w = wy(i) * wx(j), w(i) = min(1, (i + 0.5) / overlap, (T - i - 0.5) / overlap) (1 when overlap == 0).  Image
 *   rows [r0, r1) (r1 - r0 <= band_rows) are updated, tiles in the given order, one writer per element.  C <= 8.
 * s2s_region_finalize: rows [r0, r1): out = acc / wsum; out_f (optional) float [.][W][C] with row pitch pitch_f
 *   elements, out_u8 (optional, C >= 3) uint8 [.][W][3] of channels 0..2 as trunc(clamp((out * 0.5 + 0.5) * 255,
 *   0, 255)) with row pitch pitch_u8 bytes; both buffers start at image row out_top.  The ring rows are cleared. */
int s2s_region_gather(const void* img_u8, long pitch, int H, int W, int band_top, int band_h, const int* origins,
                      float* out, int B, int T, void* stream);
int s2s_region_blend(const float* tiles, int c0, const float* tiles1, int c1, const int* origins, int n, int T,
                     int overlap, float* acc, int band_rows, int H, int W, int r0, int r1, void* stream);
int s2s_region_finalize(float* acc, int band_rows, int W, int C, int r0, int r1, void* out_u8, long pitch_u8,
                        float* out_f, long pitch_f, int out_top, void* stream);

/* ---- tissue-aware regions: background tiles skip the sampler (region.hip) ----------
 * All three are atomic-free with one writer per output element, so results are bit-reproducible.
 * s2s_region_tissue_count: counts[k] (int32 [n], every entry written) = the tissue pixels of tile k's intersection
 *   with the H x W image, one workgroup per tile; a pixel is tissue iff min(R, G, B) < white and max(R, G, B) >= black
 *   (white in 1..256, black in 0..255; 0 disables the dark test).  img_u8, pitch, band_top, band_h and origins as in
 *   s2s_region_gather, so a host image can be counted band by band; reflected padding is not counted.  The origins live
 *   on the GPU, out of the host's sight: the host check covers what it can see (S2S_ERR_SHAPE), and a tile whose
 *   in-image rows are not all inside the band reads nothing and gets counts[k] = -1.  Choose the bands so that this
 *   does not happen.
 * s2s_region_skip_weight: ws, a ring of band_rows rows of W floats (row r at r % band_rows), += wy(i) * wx(j) of the
 *   n skipped tiles at origins, in order, over image rows [r0, r1) (r1 - r0 <= band_rows), with s2s_region_blend's
 *   window.  One writer per element; reads no image bytes.
 * s2s_region_finalize_mixed: s2s_region_finalize for a region with skipped tiles.  src_u8: the source image's rows
 *   from image row src_top on (row pitch src_pitch bytes), covering [r0, r1).  Per pixel, with wk = acc[C]:
 *   wk == 0 (no kept tile covers it): out_u8 = the source bytes, copied; out_f[0..2] = (u / 255 - 0.5) / 0.5,
 *   out_f[3..] = 0.  Otherwise x_c = fmaf(ws, (u_c / 255 - 0.5) / 0.5, acc_c) / (wk + ws) for c < 3 and
 *   acc_c / (wk + ws) for the probability channels (a skipped tile's probabilities are 0), then the save conversion of
 *   s2s_region_finalize.  Both ring rows are cleared.  With ws == 0 everywhere it is bit-equal to s2s_region_finalize.
 *   3 <= C <= 8. */
int s2s_region_tissue_count(const void* img_u8, long pitch, int H, int W, int band_top, int band_h, const int* origins,
                            int n, int T, int white, int black, int* counts, void* stream);
int s2s_region_skip_weight(const int* origins, int n, int T, int overlap, float* ws, int band_rows, int H, int W,
                           int r0, int r1, void* stream);
int s2s_region_finalize_mixed(float* acc, float* ws, int band_rows, int W, int C, int r0, int r1, const void* src_u8,
                              long src_pitch, int src_top, void* out_u8, long pitch_u8, float* out_f, long pitch_f,
                              int out_top, void* stream);

/* ---- segmentation loss (seg_loss.hip) -- SURVEY section 8 row f2 --------------------------------------
 * seg = dw * DiceLoss(sigmoid(z), g) + (1-dw) * BCEWithLogits(z, g)  (conditional_flow_matching_multitask.py:36-53,
 * 174-202).  z, g: float[n]; out: float[3] = {seg, dice, bce}; dz (optional) = grad_scale * d seg / dz;
 * work: double[512*4 + 4]. */
int s2s_seg_loss(const float* z, const float* g, float* dz, float* out, double* work, long n, float smooth,
                 float dice_weight, float grad_scale, void* stream);
/* Multiclass form: dw * MulticlassDiceLoss(softmax(z), t) + (1-dw) * CrossEntropy(z, t, ignore_index)
 * (conditional_flow_matching_multitask_multiclassloss.py:41-83, 159, 214-245).  z: float[B][C][HW] logits,
 * target: int64[B][HW]; out: float[3] = {seg, dice, ce}; dz (optional) float[B][C][HW];
 * work: double[(512 + 1) * 26]; 2 <= C <= 8. */
int s2s_seg_loss_multiclass(const float* z, const long* target, float* dz, float* out, double* work, long B, long HW,
                            int C, int ignore_index, float smooth, float dice_weight, float grad_scale, void* stream);

/* ---- evaluation passes (eval_metrics.hip): losses without gradients + segmentation metrics -----------------
 * Validation / test steps of the multitask modules.  Per-workgroup partials and a one-workgroup finalize: no atomics,
 * bit-reproducible, no allocation or host synchronisation (capturable).
 * Binary (conditional_flow_matching_multitask.py:326-343, 366-381): z, g: float[n] (logits, {0,1} mask);
 *   out: float[5] = {seg, dice loss, bce, dice_coef, iou}, the first three as s2s_seg_loss gives them;
 *   counts: int64[4] = {I, P, G, U} of pred = sigmoid(z) > 0.5 (I = sum pred*g, P = sum pred, G = sum g,
 *   U = sum (pred | g)); dice_coef = (2I + 1e-7) / (P + G + 1e-7), iou = (I + 1e-7) / (U + 1e-7) in fp32.
 *   The predicate is the loss kernel's p = 1/(1+exp(-z)) > 0.5; it differs from z > 0 for 0 < z <~ 1e-7.
 *   work: double[512*8].
 * Multiclass (conditional_flow_matching_multitask_multiclassloss.py:437-470): z: float[B][C][HW], target: int64[B][HW],
 *   2 <= C <= 8; out: float[5] = {seg, dice loss, ce, mean dice_coef, mean iou} (first three as
 *   s2s_seg_loss_multiclass); pred = argmax_c z (first maximal index); counts: int64[32] = I_c, P_c, G_c, U_c at
 *   [0|8|16|24 + c] (P_c counts every pixel, ignored targets included); the means run over c != ignore_index.
 *   work: double[512*58].
 * Flow head + MSE (task_decoders.py:132 + conditional_flow_matching.py:72), forward only: loss = mean((W a + b - u)^2)
 *   over the NHWC activation x (C % 8 == 0, ld % 8 == 0, bf16 or fp32) and u: float[B][Cout][H][W], Cout <= 8;
 *   lpart: double[s2s_head_mse_eval_blocks()]. */
int s2s_seg_eval_binary(const float* z, const float* g, float* out, long* counts, double* work, long n, float smooth,
                        float dice_weight, void* stream);
int s2s_seg_eval_multiclass(const float* z, const long* target, float* out, long* counts, double* work, long B,
                            long HW, int C, int ignore_index, float smooth, float dice_weight, void* stream);
int s2s_head_mse_eval_blocks(int B, int H, int W, int C);
/* test-facing, no launch: the instantiation s2s_head_mse_eval takes, from its own dispatch: 256 MO + GL, GL = 1, 2, 4, 8
 * lanes per pixel and MO = 3, 4, 8 outputs unrolled; a negative status for a refused launch */
int s2s_head_mse_family(int dtype, int B, int H, int W, int C, int Cout);
int s2s_head_mse_eval(int dtype, const void* x, int ldx, const float* w, const float* bias, const float* u_nchw,
                      float* loss, double* lpart, int B, int H, int W, int C, int Cout, void* stream);

/* ---- image-quality metrics (image_metrics.hip) ---------------------------------------------------------
 * Per-sample MSE, MAE, PSNR = 10 log10(L^2 / mse) (+inf at mse == 0) and SSIM (Wang et al. 2004: separable Gaussian
 * window of `win` taps, odd, <= 11, normalised, computed by the caller: `taps` is a HOST array of win floats;
 * C1 = (k1 L)^2, C2 = (k2 L)^2, biased local moments, only the (H - win + 1)(W - win + 1) positions per channel whose
 * window lies inside the image), all over every channel.  One fused pass: a workgroup owns 32 x 32 valid positions and
 * writes three fp64 partials (sum ssim, sum d^2, sum |d|) at part[((n * nby + by) * nbx + bx) * 3], by / bx the block's
 * row / column in the whole image; part: double[B * s2s_image_quality_blocks(H, W, win) * 3].  No atomics, no host
 * synchronisation, bit-reproducible; H, W >= win, otherwise free.
 * s2s_image_quality_f32: float [B][C][H][W] pairs in the network's range, C <= 4; quantize 0: clamp(x * 0.5 + 0.5, 0, 1)
 *   with L = 1, quantize 1: trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255)) with L = 255 (s2s_region_finalize's uint8).
 * s2s_image_quality_u8: uint8 [B][.][W][3] pairs, row pitches and sample strides in bytes, L = 255.  The buffers hold
 *   image rows [band_top, band_top + band_h) of an H x W image; block rows [by0, by0 + nby) are computed, which read
 *   image rows [32 by0, min(32 (by0 + nby) + win - 1, H)).
 * s2s_image_quality_finalize: out: float [4][B] = psnr, ssim, mae, mse from the partials, summed in a fixed order;
 *   `range` is L. */
int s2s_image_quality_blocks(int H, int W, int win);
int s2s_image_quality_f32(const float* a, const float* b, int B, int C, int H, int W, int quantize, int win,
                          const float* taps, float k1, float k2, double* part, void* stream);
int s2s_image_quality_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b, int B,
                         int band_top, int band_h, int H, int W, int by0, int nby, int win, const float* taps, float k1,
                         float k2, double* part, void* stream);
int s2s_image_quality_finalize(const double* part, int B, int C, int H, int W, int win, float range, float* out,
                               void* stream);

/* ---- stain quantification (stain_quant.hip) -------------------------------------
 * Colour deconvolution (Ruifrok & Johnston 2001) and the positive-area burden.  od(u) = od_table[u], a HOST array of 256
 * floats (-log10(max(u, 1) / 255), computed in double by the caller); `unmix` is a HOST array of 12 floats: m[3 ch + k],
 * the inverse of the stain basis, then the three thresholds.  c_k = ((od_r m_rk) + (od_g m_gk)) + (od_b m_bk), every
 * operation rounded in fp32; a pixel is tissue by the rule of s2s_region_tissue_count (white, black) and positive for
 * stain k iff tissue and c_k > thr_k.  An owner is a cell_h x cell_w cell of one sample (cell = image: one owner per
 * sample); owner index (n * Gy + gy) * Gx + gx.  A cell is cut into chunks of 16 rows x 1024 columns,
 * s2s_stain_quant_chunks(cell_h, cell_w) of them; a workgroup reduces one chunk and writes 7 (single) or 5 (paired)
 * 8-byte partials at part[(owner * chunks + chunk) * K]: no atomics, bit-reproducible, independent of the banding.
 * s2s_stain_quant_u8: uint8 [B][.][W][3], row pitches and sample strides in bytes; paired != 0 reads b too.  The buffers
 *   hold image rows [band_top, band_top + band_h) of an H x W image; chunk rows [g0, g0 + ng) are computed, chunk row
 *   g = gy * cdiv(cell_h, 16) + cy reading image rows from gy * cell_h + 16 cy on.
 * s2s_stain_quant_f32: float [B][3][H][W] in the network's range through the save conversion
 *   trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255)); one owner per sample.
 * s2s_stain_quant_finalize: single: counts long [owners][4] = tissue, positive_k; sums double [owners][3] = sum over
 *   tissue of max(c_k, 0); out float [owners][6] = burden_k = positive_k / max(tissue, 1), mean_od_k.  paired (for
 *   `stain`): counts long [owners][5] = tissue_a, tissue_b, positive in both, in a only, in b only; out float
 *   [owners][5] = burden_a, burden_b, |burden_a - burden_b|, Dice, IoU (1 when both masks are empty); sums unused.
 * s2s_stain_separate: uint8 [B][H][W][3] (pitch, img_stride in bytes) or float [B][3][H][W] (elements) -> out float
 *   [B][3][H][W], the concentrations.
 * s2s_stain_mask_u8 / s2s_stain_mask_f32: the positive mask of stain `stain` as bytes, bit 0 = positive, bit 1 = tissue,
 *   written into mask [B][H][.] (mask_pitch, mask_stride in bytes) at the image's own rows: the uint8 buffer holds image
 *   rows [band_top, band_top + band_h) as for s2s_stain_quant_u8.  tissue long [B] is ADDED to with integer atomics (the
 *   caller zeroes it; the bands of a region add up in it).  What s2s_objects_label labels with fg_bits = 1. */
int s2s_stain_quant_chunks(int cell_h, int cell_w);
int s2s_stain_quant_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b, int paired,
                       int B, int band_top, int band_h, int H, int W, int cell_h, int cell_w, int g0, int ng,
                       const float* od_table, const float* unmix, int white, int black, int stain, double* part,
                       void* stream);
int s2s_stain_quant_f32(const float* a, const float* b, int paired, int B, int H, int W, const float* od_table,
                        const float* unmix, int white, int black, int stain, double* part, void* stream);
int s2s_stain_quant_finalize(const double* part, long owners, int nchunk, int paired, long* counts, double* sums,
                             float* out, void* stream);
int s2s_stain_separate(const void* img, int is_f32, long pitch, long img_stride, int B, int H, int W,
                       const float* od_table, const float* unmix, float* out, void* stream);
int s2s_stain_mask_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
                      const float* od_table, const float* unmix, int white, int black, int stain, void* mask,
                      long mask_pitch, long mask_stride, long* tissue, void* stream);
int s2s_stain_mask_f32(const float* img, int B, int H, int W, const float* od_table, const float* unmix, int white,
                       int black, int stain, void* mask, long mask_pitch, long mask_stride, long* tissue, void* stream);

/* ---- Macenko stain normalisation (stain_norm.hip) --------------------------------
 * The uint8 buffers hold image rows [band_top, band_top + band_h) of B images of H x W RGB pixels; pitch and img_stride
 * in bytes, any pitch >= 3 W, any base alignment.  od_table as in stain quantification.  A pixel is KEPT iff
 * black <= max(R, G, B) <= u_beta (u_beta = floor(255 exp(-beta)), Macenko's OD cut-off on bytes).
 * s2s_stain_moments_u8: q_table is a HOST array of 256 ints, rint(od_table[u] * 2^12).  A workgroup reduces one chunk of
 *   16 rows x 1024 columns and writes ten int64 partials (n, sum q_c, sum q_c q_d for rr rg rb gg gb bb over the kept
 *   pixels) at part[((n * cdiv(H, 16) + cy) * cdiv(W, 1024) + cx) * 10]; s2s_stain_moments_slots(B, H, W) chunks in
 *   all.  band_top must be a multiple of 16, band_h too unless the band ends the image, and band_h <= 16 * 65535.
 * s2s_stain_moments_finalize: the ten int64 sums over nslots chunks.
 * s2s_stain_angle_hist_u8: plane is a HOST array of 6 floats, plane[2 ch + k], the two leading eigenvectors.  Per kept
 *   pixel x = ((od_r v1_r) + (od_g v1_g)) + (od_b v1_b), y likewise with v2, d = |x| + |y| (d == 0: skipped),
 *   s = y / d, bin = clamp(floor((s + 1) * 2048), 0, 4095), every operation rounded in fp32; hist long [4096].
 * s2s_stain_conc_hist_u8: unmix is a HOST array of 9 floats m[3 ch + k]; c_k as in stain quantification for k = 0, 1,
 *   bin = clamp(floor(c_k * 1024), 0, 4095); hist long [2][4096].
 *   Both histograms are ADDED to with 64-bit integer atomics (bit-reproducible); reset != 0 zeroes hist first, in a
 *   launch of its own on the same stream: the first band of a call passes 1.
 * s2s_stain_normalize_u8: no pixel is gated.  coef is a HOST array of 17 floats: m[3 ch + k] (9), the two concentration
 *   scales, the reference vectors ref[3 k + ch] (6).  c'_k = c_k * scale_k, od'_ch = (c'_0 ref_0ch) + (c'_1 ref_1ch),
 *   u'_ch = clamp(rint(255 * exp2(od'_ch * -log2(10))), 0, 255).  out_f32 == 0: uint8 [B][H][W][3] with out_pitch /
 *   out_img in bytes; else float [B][3][H][W] = (u' / 255 - 0.5) / 0.5 (out_pitch, out_img ignored). */
long s2s_stain_moments_slots(int B, int H, int W);
int s2s_stain_moments_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
                         const int* q_table, int u_beta, int black, long* part, void* stream);
int s2s_stain_moments_finalize(const long* part, long nslots, long* out, void* stream);
int s2s_stain_angle_hist_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
                            const float* od_table, const float* plane, int u_beta, int black, int reset, long* hist,
                            void* stream);
int s2s_stain_conc_hist_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
                           const float* od_table, const float* unmix, int u_beta, int black, int reset, long* hist,
                           void* stream);
int s2s_stain_normalize_u8(const void* img, long pitch, long img_stride, int B, int H, int W, const float* od_table,
                           const float* coef, void* out, long out_pitch, long out_img, int out_f32, void* stream);

/* ---- stain threshold calibration: per-owner histograms, Otsu / triangle (stain_calibrate.hip) ---
 * Images, od_table, unmix (the first nine floats are read), white and black as in stain quantification; c_k and the
 * tissue rule are the same.  bin(c) = clamp(ceil(c * 1024) - 1, 0, 4095), every operation in fp32, clamped as a float:
 * bin(c) >= j <=> c > j / 1024 for j in 1..4095.  An owner is one sample (pool == 0: B owners) or the whole batch
 * (pool != 0: one owner) and holds at most 2^40 pixels (H W, or B H W pooled); B <= 65535.
 * s2s_stain_hist_u8 / _f32: hist long [owners][3][4096]: hist[o][k][b] += the tissue pixels of owner o with
 *   bin(c_k) = b, for the stains k of stain_mask (bits 0..2, not empty; the other rows are not touched by the counting);
 *   tissue long [owners] += the tissue pixels.  Both are ADDED to with 64-bit integer atomics (bit-reproducible; bands
 *   and repeated calls add up); reset != 0 zeroes all of hist and tissue first, in a launch of its own on the same
 *   stream.  The uint8 buffers hold image rows [band_top, band_top + band_h) of B images (pitch, img_stride in bytes, any
 *   alignment); float input is [B][3][H][W] in the network's range through the save conversion.
 * s2s_stain_pair_hist_u8 / _f32: for stain `stain` of a prediction a and a target b, hist long [owners][4][4096]:
 *   [0] a's tissue by bin_a, [1] b's tissue by bin_b, [2] tissue in both by min(bin_a, bin_b), [3] tissue in both with
 *   bin_b >= jt by bin_a (jt in 1..4095; jt == 0: row 3 is not counted); tissue long [owners][2] (a, b).
 *   A launch whose workgroups would count 2^32 pixels or more each is refused (a uint32 bin in LDS could wrap).
 * s2s_stain_thresholds: hist long [rows][4096] -> positive long [rows][4096], positive[j] = sum over b >= j of hist[b];
 *   bins / valid int [rows][2 + nquant], thr double [rows][2 + nquant] = bins / 1024: column 0 Otsu (S1[j] = sum over
 *   b >= j of b hist[b], N = positive[0], S = S1[0]; sigma(j) = a a / (double(P) double(N - P)) with P = positive[j] and
 *   a = double(N S1[j] - P S) formed exactly and rounded once, 0 when P is 0 or N; the smallest j >= 1 of maximal sigma;
 *   valid 0 and bin 0 when every sigma is 0), column 1 the triangle rule on the histogram summed in groups of `coarse`
 *   (a power of two in 1..4096) bins: p the smallest index of the maximal group g, e the largest non-empty index,
 *   T(i) = g[p] (e - p) + (g[e] - g[p]) (i - p) - g[i] (e - p) for p < i < e, bin = coarse * (the smallest i of maximal
 *   T); valid 0 and bin 0 when e <= p + 1), columns 2.. the quantiles (a HOST array of nquant <= 8 doubles in [0, 1]):
 *   the smallest j >= 1 with positive[j] <= floor(q double(N)); 4095 and valid 0 when there is none or N = 0.
 * s2s_stain_pair_thresholds: hist long [owners][4][4096] -> counts long [owners][4][4096] = the suffix sums positive_a,
 *   positive_b, both_common, both_cond; dice double [owners][2][4096] = 2 both_common / (positive_a + positive_b) and
 *   2 both_cond / (positive_a + positive_b[jt]), 1 where the denominator is 0 (the second row is 0 without jt); bins /
 *   valid int [owners][2]: the smallest j >= 1 of minimal |positive_a[j] N_b - positive_b[jt] N_a| and the smallest
 *   j >= 1 of maximal conditional Dice, both compared exactly in 128 bits; valid iff jt > 0 and both images have
 *   tissue.  vals double [owners][8]: the two thresholds, Dice and the prediction's burden at the best-Dice bin, the
 *   target's burden at jt, the prediction's burden, |burden difference| and Dice at the burden-matching bin. */
int s2s_stain_hist_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
                      const float* od_table, const float* unmix, int white, int black, int stain_mask, int pool,
                      int reset, long* hist, long* tissue, void* stream);
int s2s_stain_hist_f32(const float* img, int B, int H, int W, const float* od_table, const float* unmix, int white,
                       int black, int stain_mask, int pool, int reset, long* hist, long* tissue, void* stream);
int s2s_stain_pair_hist_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b, int B,
                           int band_top, int band_h, int H, int W, const float* od_table, const float* unmix, int white,
                           int black, int stain, int jt, int pool, int reset, long* hist, long* tissue, void* stream);
int s2s_stain_pair_hist_f32(const float* a, const float* b, int B, int H, int W, const float* od_table,
                            const float* unmix, int white, int black, int stain, int jt, int pool, int reset, long* hist,
                            long* tissue, void* stream);
int s2s_stain_thresholds(const long* hist, long rows, int coarse, const double* quantiles, int nquant, long* positive,
                         int* bins, int* valid, double* thr, void* stream);
int s2s_stain_pair_thresholds(const long* hist, long owners, int jt, long* counts, double* dice, int* bins, int* valid,
                              double* vals, void* stream);

/* ---- zonal stain quantification: burden and objects per class of a zone map (zonal.hip) ----------
 * Images, od_table, unmix (twelve floats: m, then the three thresholds), white and black as in stain quantification; c_k,
 * the tissue rule and "positive" (tissue and c_k > thr_k) are the same.  q_k = min((int)rintf(fmaxf(c_k, 0) * 1024),
 * 4095) as in s2s_objfeat_intensity_*, but summed over TISSUE pixels only.  zones: one byte per pixel, [B][.][.] with
 * zone_pitch and zone_stride in bytes (any pitch >= W, any alignment); num_zones = Z in 1..256; a pixel whose byte is
 * >= Z belongs to no zone.  An owner is one sample (pool == 0: B owners) or the whole batch (pool != 0: one owner) and
 * holds at most 2^40 pixels; B <= 65535.  The grid is at most one resident round (2048 workgroups over all owners, 1792 paired); a
 * launch whose workgroups would take 2^20 pixels or more each is refused with the shape status before any launch (a
 * uint32 cell of the workgroup's LDS table holds at most pixels * 4095).
 * s2s_zonal_u8 / _f32: table long [owners][Z][8] += pixels, tissue, positive_0, positive_1, positive_2, sum q_0, sum q_1,
 *   sum q_2 of the owner's pixels of each zone; unzoned long [owners] += the pixels of no zone.  Both are ADDED to with
 *   64-bit integer atomics (bit-reproducible; bands and repeated calls add up); reset != 0 zeroes table and unzoned
 *   first, in a launch of its own on the same stream.  The uint8 image and zone buffers hold rows [band_top, band_top +
 *   band_h) of B images of H x W pixels; float input is [B][3][H][W] in the network's range through the save conversion,
 *   with the zones of all H rows.
 * s2s_zonal_pair_u8 / _f32: for stain `stain` of a prediction a and a target b over one zone map, table long
 *   [owners][Z][6] += pixels, tissue_a, tissue_b, positive in both, in a only, in b only.
 * s2s_zonal_finalize: one thread per (owner, zone), fp64, no contraction, in this order.  paired == 0: out double
 *   [owners][Z][8]: td = (double)max(tissue, 1);
 *     0..2  burden_k = (double)positive_k / td
 *     3..5  mean_conc_k = ((double)sum q_k / td) / 1024
 *     6     tissue_frac = (double)tissue / (double)max(pixels, 1)
 *     7     area_frac = (double)pixels / (double)max(N, 1), N = unzoned[owner] + the sum over the owner's zones of pixels
 *   paired != 0 (unzoned may be null): out double [owners][Z][5]: na = both + a_only, nb = both + b_only;
 *     0, 1  burden_pred = (double)na / (double)max(tissue_a, 1), burden_target = (double)nb / (double)max(tissue_b, 1)
 *     2     burden_abs_err = fabs(burden_pred - burden_target)
 *     3     dice = (double)(2 * both) / (double)(na + nb), 1 when na + nb == 0
 *     4     iou = (double)both / (double)(both + a_only + b_only), 1 when that is 0
 * s2s_zonal_object_overlap: labels int [B][H][W], dense, as s2s_objfeat_shape reads them (0 = background, objects
 *   1..count, M = max_objects >= 1, labels above M not tabulated); H, W <= 32767; B M Z < 2^31, refused with the shape
 *   status otherwise.  overlap int [B][M][Z] += the pixels of object m + 1 whose zone byte is z < Z; area int [B][M] +=
 *   all pixels of object m + 1; count int [B] = max(count, the largest label).  The CALLER ZEROES all three.  One launch.
 * s2s_zonal_object_assign: one wave per row (b, m).  The zone of an object is the z of largest overlap, ties to the
 *   smaller z: zone int [B][M] = it, zone_pixels long [B][M] = that overlap; -1 and 0 when every overlap is 0 and in rows
 *   at or beyond min(count, M).  objects long [B][Z] += 1 and object_pixels long [B][Z] += area at the object's zone (the
 *   caller zeroes both).
 * s2s_zonal_object_density: table as s2s_zonal_u8 writes it, scale a HOST double (mpp^2 * 1e-6); per_mm2 double
 *   [owners][Z] = (double)objects / ((double)tissue * scale), 0 where tissue == 0.
 * s2s_zonal_bands: d2_bg, d2_fg int [B][H][W] as s2s_morph_edt writes them (to_foreground = 0 / 1; 16-byte aligned, out
 *   4-byte aligned, S2S_ERR_ALIGN otherwise); edges2 a HOST array of n ints in 1..126, 0 <= E_i < 2^31 - 1, not
 *   descending.  A pixel is foreground iff d2_bg > 0.  Foreground: byte = #{i : d2_bg > E_i}; background: byte = n + 1 +
 *   #{i : d2_fg > E_i}; side 1 ("inside") writes 255 on the background, side 2 ("outside") 255 on the foreground, side 0
 *   neither.  out: bytes [B][H][W], dense. */
int s2s_zonal_u8(const void* img, long pitch, long img_stride, const void* zones, long zone_pitch, long zone_stride, int B,
                 int band_top, int band_h, int H, int W, int num_zones, const float* od_table, const float* unmix,
                 int white, int black, int pool, int reset, long* table, long* unzoned, void* stream);
int s2s_zonal_f32(const float* img, const void* zones, long zone_pitch, long zone_stride, int B, int H, int W,
                  int num_zones, const float* od_table, const float* unmix, int white, int black, int pool, int reset,
                  long* table, long* unzoned, void* stream);
int s2s_zonal_pair_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b, const void* zones,
                      long zone_pitch, long zone_stride, int B, int band_top, int band_h, int H, int W, int num_zones,
                      const float* od_table, const float* unmix, int white, int black, int stain, int pool, int reset,
                      long* table, long* unzoned, void* stream);
int s2s_zonal_pair_f32(const float* a, const float* b, const void* zones, long zone_pitch, long zone_stride, int B, int H,
                       int W, int num_zones, const float* od_table, const float* unmix, int white, int black, int stain,
                       int pool, int reset, long* table, long* unzoned, void* stream);
int s2s_zonal_finalize(const long* table, const long* unzoned, long owners, int num_zones, int paired, double* out,
                       void* stream);
int s2s_zonal_object_overlap(const int* labels, const void* zones, long zone_pitch, long zone_stride, int B, int H, int W,
                             int num_zones, int max_objects, int* overlap, int* area, int* count, void* stream);
int s2s_zonal_object_assign(const int* overlap, const int* area, const int* count, int B, int num_zones, int max_objects,
                            int* zone, long* zone_pixels, long* objects, long* object_pixels, void* stream);
int s2s_zonal_object_density(const long* objects, const long* table, long owners, int num_zones, const double* scale,
                             double* per_mm2, void* stream);
int s2s_zonal_bands(const int* d2_bg, const int* d2_fg, int B, int H, int W, const int* edges2, int n, int side, void* out,
                    void* stream);

/* ---- stain object analysis: connected-component labelling (objects.hip) -----------
 * A sample is H x W <= 2^31 - 2 pixels and has an index space of its own: nothing joins two samples.  B <= 65535.
 * s2s_objects_words(B, H, W): the int32 words of scratch s2s_objects_label needs (parents, then chunk counts);
 *   s2s_objects_hit_words: those of s2s_objects_hits.  Negative: a status code.
 * s2s_objects_label: mask bytes [B][H][.] (pitch, img_stride in bytes), foreground iff (byte & fg_bits) != 0;
 *   connectivity 4 or 8.  An object is kept iff its area >= min_area; kept objects are numbered 1..count[n] in raster
 *   order of their first pixel.  labels int [B][H][W]: the number, 0 for background and dropped objects.  count int [B]
 *   is written; kept_pixels long [B], largest int [B] and size_hist long [B][32] (bin floor(log2(area))) are ADDED to /
 *   maxed into with integer atomics: the caller zeroes them.  max_objects > 0: rows < min(count, max_objects) of
 *   tab_area int [B][M], tab_bbox int [B][M][4] (y0, x0, y1, x1, end-exclusive) and tab_sums long [B][M][2] (sum of y,
 *   sum of x) are written, the other rows are not touched (the caller zeroes the tables).  max_objects == 0: no table,
 *   the three pointers are ignored.  Nine launches, no host synchronisation.
 * s2s_objects_label_seeded: s2s_objects_label of the components SELECTED by a marker.  marker
 *   bytes [B][H][.] (marker_pitch, marker_img_stride in bytes; it may be the mask's buffer under other bits): a seed is a
 *   foreground pixel with (marker byte & seed_bits) != 0, seed_bits in 1..255.  seeds(component) = its seeds; a component
 *   is selected iff (seeds >= min_seed) != invert, min_seed >= 1, invert 0 or 1.  The pixels of the components not
 *   selected are background for everything s2s_objects_label computes (min_area, numbering, statistics and tables then
 *   work on the selected ones as above).  out_mask (bytes [B][H][.], out_pitch / out_img_stride in bytes, may be null):
 *   every byte is written, 1 on the pixels of the selected components (before the area filter) and 0 elsewhere, | (mask
 *   byte & 2) when fg_bits == 1 (the stain-mask convention: bit 0 positive, bit 1 tissue).  candidates int [B] = the
 *   components of the mask, seeded int [B] = those with seeds >= min_seed (before invert and the area filter),
 *   seed_pixels long [B] = the seeds; all three are written (zeroed by a launch of this call).  scratch: the words of
 *   s2s_objects_words.  Thirteen launches, no host synchronisation.
 * s2s_objects_centroid: centroid float [B][M][2] = float((double)sum / area) for rows < count, 0 beyond.
 * s2s_objects_hits: hits int [B][2] = the objects of labels_pred that share a pixel with an object of labels_target, and
 *   the other way round (per-object bit flags in scratch set by atomicOr, then counted).  Both are written.
 * s2s_objects_scores: out float [B][3] = recall = hits_target / count_target, precision = hits_pred / count_pred (a
 *   ratio whose count is 0 is 1 when the other count is 0 too, else 0), f1 = 2 p r / (p + r) (0 when p + r = 0), each
 *   evaluated in double and rounded once; abs_err int [B] = |count_pred - count_target|.
 * s2s_objects_density: burden float [B] = float((double)kept / max(tissue, 1)).  mm2_per_pixel: a HOST double
 *   (mpp^2 * 1e-6), or null; given, per_mm2 double [B] = count / (tissue * mm2_per_pixel), 0 when tissue is 0. */
long s2s_objects_words(int B, int H, int W);
long s2s_objects_hit_words(int B, int H, int W);
int s2s_objects_label(const void* mask, long pitch, long img_stride, int fg_bits, int B, int H, int W, int connectivity,
                      int min_area, int max_objects, int* scratch, int* labels, int* count, long* kept_pixels,
                      int* largest, long* size_hist, int* tab_area, int* tab_bbox, long* tab_sums, void* stream);
int s2s_objects_label_seeded(const void* mask, long pitch, long img_stride, int fg_bits, const void* marker,
                             long marker_pitch, long marker_img_stride, int seed_bits, int min_seed, int invert, int B,
                             int H, int W, int connectivity, int min_area, int max_objects, int* scratch, int* labels,
                             int* count, long* kept_pixels, int* largest, long* size_hist, int* tab_area, int* tab_bbox,
                             long* tab_sums, void* out_mask, long out_pitch, long out_img_stride, int* candidates,
                             int* seeded, long* seed_pixels, void* stream);
int s2s_objects_centroid(const int* count, const int* tab_area, const long* tab_sums, int B, int max_objects,
                         float* centroid, void* stream);
int s2s_objects_hits(const int* labels_pred, const int* labels_target, int B, int H, int W, int* scratch, int* hits,
                     void* stream);
int s2s_objects_scores(const int* count_pred, const int* count_target, const int* hits, int B, float* out,
                       int* abs_err, void* stream);
int s2s_objects_density(const long* kept_pixels, const long* tissue, const int* count, int B,
                        const double* mm2_per_pixel, float* burden, double* per_mm2, void* stream);

/* ---- mask morphology and boundary metrics: exact distance transform (morphology.hip) -
 * Masks are bytes [B][H][.] (pitch, img_stride in bytes), foreground iff the byte is not 0.  H, W <= 32767 (so that
 *   H^2 + W^2 < 2^31) and B <= 65535; anything beyond is refused with the shape status.  Nothing lies outside the
 *   image.  FAR = 2^31 - 1.  Outputs are dense [B][H][W].  scratch: int32 words, 8-byte aligned.
 * s2s_morph_words(B, H, W, agreement): the words s2s_morph_edt / s2s_morph_threshold (agreement = 0) or
 *   s2s_morph_boundary_agreement (agreement = 1) need; s2s_morph_fill_holes_words: those of s2s_morph_fill_holes (the
 *   labelling's own scratch included).  Negative: a status code.
 * s2s_morph_edt: out int = the squared distance to the nearest background pixel (to_foreground = 0) or foreground pixel
 *   (1) of the same sample, FAR when the sample has none; values above max_d2 are reported as FAR (max_d2 = FAR: no
 *   limit).  Four launches.
 * s2s_morph_threshold: out bytes = D_fg <= r2 (erode = 0: dilation by the disc of squared radius r2) or D_bg > r2
 *   (erode = 1), 0 <= r2 < FAR.  The search stops at r2.  Four launches, no int32 map.
 * s2s_morph_boundary: out bytes = 1 on foreground pixels with a 4-neighbour that is background or outside the image.
 * s2s_morph_fill_holes: out bytes = mask != 0, or the pixel lies in a connectivity-(4 or 8)-connected component of the
 *   background that has no pixel on the first or last row or column.
 * s2s_morph_boundary_agreement: per sample, the pooled squared distances from every boundary pixel of pred to the nearest
 *   boundary pixel of target and the other way round; leaves max, the percentile-th nearest-rank percentile (1..100),
 *   the sum of isqrt(65536 s) and #{s <= tol2} in scratch.  s2s_morph_boundary_finalize (same scratch, B, H, W) writes
 *   max_d2, pq_d2, valid int [B]; sum_q8, within, boundary_pred, boundary_target long [B]; hausdorff = sqrt(max_d2), hd =
 *   sqrt(pq_d2), assd = sum_q8 / (256 n), surface_dice = within / n double [B], n = boundary_pred + boundary_target.
 *   Both boundaries empty: integers 0, surface_dice 1, valid 0.  One empty: max_d2 = pq_d2 = (H-1)^2 + (W-1)^2, sum_q8 =
 *   n isqrt(65536 max_d2), within 0, valid 0.  Fifteen + one launches, no host synchronisation. */
long s2s_morph_words(int B, int H, int W, int agreement);
long s2s_morph_fill_holes_words(int B, int H, int W);
int s2s_morph_edt(const void* mask, long pitch, long img_stride, int B, int H, int W, int to_foreground, int max_d2,
                  int* scratch, int* out, void* stream);
int s2s_morph_threshold(const void* mask, long pitch, long img_stride, int B, int H, int W, int erode, int r2,
                        int* scratch, void* out, void* stream);
int s2s_morph_boundary(const void* mask, long pitch, long img_stride, int B, int H, int W, void* out, void* stream);
int s2s_morph_fill_holes(const void* mask, long pitch, long img_stride, int B, int H, int W, int connectivity,
                         int* scratch, void* out, void* stream);
int s2s_morph_boundary_agreement(const void* pred, long pred_pitch, long pred_img, const void* target, long target_pitch,
                                 long target_img, int B, int H, int W, int tol2, int percentile, int* scratch,
                                 void* stream);
int s2s_morph_boundary_finalize(const int* scratch, int B, int H, int W, int* max_d2, int* pq_d2, long* sum_q8,
                                long* within, long* boundary_pred, long* boundary_target, int* valid, double* hausdorff,
                                double* hd, double* assd, double* surface_dice, void* stream);

/* ---- stain object morphometry: per-object shape, thickness and intensity (object_features.hip) ---
 * labels: int [B][H][W], dense, as s2s_objects_label writes them: 0 = background or a dropped object, objects 1..count.
 *   M = max_objects >= 1; objects numbered above M are not tabulated, but where a neighbour rule asks whether a label
 *   differs they are a different label.  H, W <= 32767 and B <= 65535; anything beyond is refused with the shape status
 *   before any launch.  The CALLER ZEROES count and every table; rows at or beyond min(count, M) are not touched, and a
 *   sample's values do not depend on its batch mates.  Every table is an integer, added to or maxed into by integer
 *   atomics, so the bits do not depend on the order.
 * s2s_objfeat_shape: count int [B] = the largest label of the sample.  Per object (row = label - 1): area long [B][M];
 *   bbox int [B][M][4] = y0, x0, y1, x1, end-exclusive; moments long [B][M][5] = sum y, sum x, sum y^2, sum x^2, sum yx
 *   (each below 2^61); edges long = the crack length: the pairs (pixel of the object, one of its four neighbours) whose
 *   neighbour carries another label or lies outside the image; boundary long = the object's pixels with at least one
 *   such neighbour; border int = 1 iff the object has a pixel in the first or last row or column.  d2 (optional): the
 *   int [B][H][W] map of s2s_morph_edt; given, max_d2 int [B][M] = its maximum over the object's pixels.  Two launches.
 * s2s_objfeat_intensity_u8 / _f32: images, od_table (256 HOST floats) and unmix (HOST floats, m[3 * channel + stain];
 *   only the first nine are read) as s2s_stain_mask_u8 / _f32.  Per pixel whose label is in 1..M: c = ((od_r m_rk) +
 *   (od_g m_gk)) + (od_b m_bk) in fp32, every operation rounded on its own; q = min((int)rintf(fmaxf(c, 0) * 1024),
 *   4095); sum_q long [B][M] += q, sum_q2 long [B][M] += q^2, max_q int [B][M] = max(max_q, q).  No tissue gate.  The
 *   bands of a region accumulate in the same tables.  One launch.
 * s2s_objfeat_finalize: out double [B][M][15], one thread per object, fp64, no contraction, in this order (A = area, Ad =
 *   (double)A, A2 = Ad * Ad; N(s2, s, s') = A * s2 - s * s' formed exactly in 128 bits from 64 x 64 -> 128 multiplies,
 *   converted to double once, sign applied after):
 *     0, 1  centroid y, x = (double)sum_y / Ad, (double)sum_x / Ad
 *     2     equivalent_diameter = sqrt((4 * Ad) / pi)
 *     3..5  mu_yy = N(sum_y2, sum_y, sum_y) / A2, mu_xx = N(sum_x2, sum_x, sum_x) / A2, mu_yx = N(sum_yx, sum_y, sum_x) / A2
 *           t = mu_xx + mu_yy; d = mu_xx - mu_yy; root = sqrt(d * d + 4 * (mu_yx * mu_yx));
 *           l1 = max(0.5 * (t + root), 0); l2 = max(0.5 * (t - root), 0)
 *     6, 7  major_axis = 4 * sqrt(l1), minor_axis = 4 * sqrt(l2)
 *     8     eccentricity = sqrt(max(1 - l2 / l1, 0)), 0 when l1 == 0
 *     9     orientation = 0.5 * atan2(2 * mu_yx, d), 0 when both arguments are 0
 *     10    compactness = (4 pi * Ad) / (E * E), E = (double)edges, 4 pi = 12.566370614359172
 *     11    mean_conc = ((double)sum_q / Ad) / 1024
 *     12    std_conc = sqrt(max(N(sum_q2, sum_q, sum_q) / A2, 0)) / 1024
 *     13    max_conc = (double)max_q / 1024
 *     14    inscribed_radius = sqrt((double)max_d2), inf when max_d2 == 2^31 - 1
 *   11..13 are 0 when sum_q is null, 14 when max_d2 is null.  Rows at or beyond min(count, M), and rows of area 0, are 0. */
int s2s_objfeat_shape(const int* labels, const int* d2, int B, int H, int W, int max_objects, int* count, long* area,
                      int* bbox, long* moments, long* edges, long* boundary, int* border, int* max_d2, void* stream);
int s2s_objfeat_intensity_u8(const int* labels, const void* img, long pitch, long img_stride, int B, int band_top,
                             int band_h, int H, int W, int max_objects, const float* od_table, const float* unmix,
                             int stain, long* sum_q, long* sum_q2, int* max_q, void* stream);
int s2s_objfeat_intensity_f32(const int* labels, const float* img, int B, int H, int W, int max_objects,
                              const float* od_table, const float* unmix, int stain, long* sum_q, long* sum_q2, int* max_q,
                              void* stream);
int s2s_objfeat_finalize(const int* count, const long* area, const long* moments, const long* edges, const long* sum_q,
                         const long* sum_q2, const int* max_q, const int* max_d2, int B, int max_objects, double* out,
                         void* stream);

/* ---- splitting touching objects at their necks: watershed on the distance map (split.hip) ---
 * d2: int [B][H][W], dense, the squared distance to the background as s2s_morph_edt(to_foreground = 0) writes it;
 *   foreground iff d2 > 0 (2^31 - 1 everywhere in a sample without background).  H, W <= 32767 and B <= 65535; anything
 *   beyond is refused with the shape status before any launch.  A sample's values do not depend on its batch mates.
 * s2s_split_words(B, H, W): the int32 words of scratch s2s_split_label needs (4 H W + ceil(H W / 1024) per sample; the
 *   scratch must be 8-byte aligned, S2S_ERR_ALIGN otherwise).  Negative: a status code.
 * s2s_split_label: key(p) = (d2[p], y W + x), compared lexicographically; neighbours = the 4 or 8 (connectivity)
 *   foreground neighbours inside the image.  up(p) = the neighbour of largest key if it exceeds key(p), else p; a basin
 *   is the set of pixels whose up-chain ends in the same root r, its peak P = d2[r].  Over all neighbouring pixels (p, q)
 *   with a = root(p) != b = root(q) and key(b) > key(a), best(a) = the lexicographic maximum of (min(d2[p], d2[q]), b);
 *   basin a links to that b iff P(a) <= core2 or (long)m << 20 >= (long)neck_q * neck_q * P(a), neck_q in 0..1024 (the
 *   neck ratio times 1024), core2 >= 0.  The links form a forest; a part is one of its trees.  One round, no
 *   re-evaluation.  basins int [B] = the number of basins (written).  From there on exactly s2s_objects_label with
 *   "part" for "object": labels, count (written), kept_pixels, largest, size_hist and the tables (the caller zeroes
 *   them), min_area and max_objects as there.  Exact and independent of scheduling: every choice is a maximum over a
 *   strict total order.  Thirteen launches, no host synchronisation. */
long s2s_split_words(int B, int H, int W);
int s2s_split_label(const int* d2, int B, int H, int W, int connectivity, int neck_q, int core2, int min_area,
                    int max_objects, int* scratch, int* labels, int* count, int* basins, long* kept_pixels, int* largest,
                    long* size_hist, int* tab_area, int* tab_bbox, long* tab_sums, void* stream);

/* ---- fused paired augmentation: crop, D4, stain jitter, masks (augment.hip) --------
 * Geometry: params is a DEVICE int [B][param_cols], param_cols 4 or 5 = (top, left, hflip, vflip[, transpose]); with
 *   f[a][b] = img[n][top + (vflip ? S-1-a : a)][left + (hflip ? S-1-b : b)], out[y][x] = transpose ? f[x][y] : f[y][x].
 *   The same geometry applies to source, target and mask.  The caller validates the windows; the kernel does not clamp.
 * Pixel map: a DEVICE float [B][12] per image kind = A[3][3] row-major, then b[3]; od_table is the HOST table of the
 *   stain entry points.  od'_c = ((od_r A[0][c] + od_g A[1][c]) + od_b A[2][c]) + b[c], every operation rounded on its
 *   own; u'_c = clamp(rint(255 * exp2(od'_c * -log2(10))), 0, 255).  white in 0..255: a pixel with min(R, G, B) >= white
 *   keeps its bytes; -1: off.  A null map: the bytes pass unchanged.
 * s2s_paired_augment: src / tgt uint8 [B][Hs][Ws][3], mask (optional) uint8 [B][Hs][Ws], each with a row pitch and an
 *   image stride in bytes.  out_src / out_tgt float [B][3][S][S] = (u' / 255 - 0.5) / 0.5.  mask_kind 0: no mask (mask_u8
 *   and out_mask null); 1 / 2 / 3: out_mask float / uint8 / int64 [B][1][S][S], the byte's value.  out_src_u8 /
 *   out_tgt_u8 (each optional): uint8 [B][S][S][3], the augmented bytes.  One launch.
 * s2s_stain_augment_u8: the pixel map alone on uint8 [B][H][W][3], any H and W.  out_f32 == 0: uint8 [B][H][W][3] with
 *   out_pitch / out_img in bytes; else float [B][3][H][W] (out_pitch, out_img ignored).  One launch. */
int s2s_paired_augment(const void* src_u8, long src_pitch, long src_img, const void* tgt_u8, long tgt_pitch,
                       long tgt_img, const void* mask_u8, long mask_pitch, long mask_img, int B, int Hs, int Ws, int S,
                       const int* params, int param_cols, const float* src_map, const float* tgt_map,
                       const float* od_table, int white, float* out_src, float* out_tgt, void* out_mask, int mask_kind,
                       void* out_src_u8, void* out_tgt_u8, void* stream);
int s2s_stain_augment_u8(const void* img, long pitch, long img_stride, int B, int H, int W, const float* maps,
                         const float* od_table, int white, void* out, long out_pitch, long out_img, int out_f32,
                         void* stream);

/* ---- paired tile registration: integer-shift ZNCC search (registration.hip) --------
 * uint8 images are addressed by pitch / img_stride in bytes; any pitch and any base alignment are accepted, and the
 * samples of an input may interleave (the cells of one row of a region: img_stride = 3 * cell, pitch = 3 * W).
 * s2s_structure_map_u8: img uint8 [B][H][W][3]; q_table HOST int [256] = rint(od(u) * 2^12); w HOST int [3] =
 *   rint(unmix[ch][k] * gain * 16); acc = w_r q[R] + w_g q[G] + w_b q[B], f = clamp((acc + 2^15) >> 16, 0, 255)
 *   (arithmetic shift); ds in {1, 2, 4}: out = (sum of the ds x ds block of f + ds^2 / 2) / ds^2 over whole blocks.
 *   out uint8 [B][H / ds][W / ds], contiguous.  One launch.
 * s2s_register_sums: a, b uint8 [B][h][w], contiguous; 0 <= R <= 32, S = 2 R + 1; center DEVICE int [B][2] = (cy, cx)
 *   or null = 0.  my = R + |cy|, mx = R + |cx| in 64 bits; the template is a[my : h - my, mx : w - mx], the window of
 *   shift (dy, dx) in centre + [-R, R]^2 is b[my + dy : h - my + dy, mx + dx : w - mx + dx].  tsum long [B][3] = n,
 *   sum a, sum a^2; sums long [B][S][S][3] = sum b, sum b^2, sum a b; both are zeroed here.  A sample whose template is
 *   empty keeps zeros and none of its pixels is read; no centre moves a read outside [0, h) x [0, w).  Shape status for
 *   R > 32, h <= 2 R, w <= 2 R or (h - 2 R)(w - 2 R) > 2^18.  Two memsets and one launch.
 * s2s_register_pick: va = n sum a^2 - (sum a)^2, vb alike, num = n sum a b - sum a sum b in int64; score = double(num) /
 *   sqrt(double(va) * double(vb)), 0 when vb = 0.  Pick: highest score, then smallest (dy - cy)^2 + (dx - cx)^2, then
 *   smallest dy, then smallest dx.  shift int [B][2] = (dy, dx) * ds; score double [B][3] = best, at the centre, best
 *   minus the best outside the 3 x 3 neighbourhood of the peak (0 when R < 2); valid int [B]: 0 when n = 0 or va = 0,
 *   and then shift = centre * ds clamped to int32 and the three scores are 0.  One launch.
 * s2s_shift_tiles_u8: img uint8 [B][H][W][C], C = 1 or 3; shift DEVICE int [B][2] = (dy, dx), any values;
 *   out[b][y][x] = img[b][y + dy][x + dx] inside the image, else fill (0..255).  One launch. */
int s2s_structure_map_u8(const void* img, long pitch, long img_stride, int B, int H, int W, const int* q_table,
                         const int* w, int ds, void* out, void* stream);
int s2s_register_sums(const void* a, const void* b, int B, int h, int w, int R, const int* center, long* tsum,
                      long* sums, void* stream);
int s2s_register_pick(const long* tsum, const long* sums, const int* center, int B, int R, int ds, int* shift,
                      double* score, int* valid, void* stream);
int s2s_shift_tiles_u8(const void* img, long pitch, long img_stride, int B, int H, int W, int C, const int* shift,
                       int fill, void* out, long out_pitch, long out_img, void* stream);

/* ---- dense region alignment: shift-field cleaning and warp (warp.hip) --------------
 * Displacements are in 1/16 pixel.  A field is D int [Gy][Gx][2] = (dy, dx); node (gy, gx) is the centre of cell
 * (gy, gx) of an H x W region, Gy = H / cell, Gx = W / cell.  Dense displacement, per axis in doubled coordinates:
 * span = 2 cell, u = 2 p + 1 - cell; G >= 2: g0 = clamp(floor(u / span), 0, G - 2), g1 = g0 + 1, w = clamp(u - g0 span,
 * 0, span); G = 1: g0 = g1 = 0, w = 0 (positions outside the node centres, the ragged remainder included, take the
 * nearest node's value).  In 64 bits num = (span - wy) ((span - wx) D[y0][x0] + wx D[y0][x1]) + wy ((span - wx) D[y1][x0]
 * + wx D[y1][x1]); d = floor((num + span^2 / 2) / span^2), clamped to +-16 max_shift per component by the kernel.
 * Image sampling (C = 3): sy = 16 y + d_y, iy = sy >> 4 (arithmetic), fy = sy & 15, columns alike; taps p00 = T[iy][ix],
 *   p01 = T[iy][ix + 1], p10 = T[iy + 1][ix], p11 = T[iy + 1][ix + 1]; a tap outside [0, H) x [0, W) of the whole region
 *   takes fill and is not read; out = ((16 - fy) ((16 - fx) p00 + fx p01) + fy ((16 - fx) p10 + fx p11) + 128) >> 8.
 *   out[y][x] is the target brought onto src[y][x]: a constant field 16 (dy, dx) is s2s_shift_tiles_u8 byte for byte.
 * Mask sampling (C = 1): nearest, iy = (sy + 8) >> 4, ix alike, one tap, fill outside.
 * s2s_warp_region_u8: src = rows [src_row0, src_row0 + src_rows) of the uint8 [H][W][C] region, out = rows [row0, row0 +
 *   rows) of the result; pitches in bytes, any pitch >= W C and any base alignment; field DEVICE, any values.  Shape
 *   status when the rows present do not cover [max(0, row0 - max_shift - 1), min(H, row0 + rows + max_shift + 1)), when
 *   Gy != H / cell, Gx != W / cell, cell < 1 or cell > 2^14 (num must fit 64 bits), Gy Gx outside 1 .. 65536, max_shift
 *   outside 0 .. 1024, or a pitch is smaller than a row.  One launch; the result does not depend on the banding.
 * s2s_field_clean: shift DEVICE int [Gy][Gx][2] in pixels, reliable DEVICE uint8 [Gy][Gx]; a cell is reliable when its
 *   byte is not 0 and max(|dy|, |dx|) <= max_shift.  (1) All cells are judged against the input: a reliable cell with n >= 3
 *   reliable cells among its 8 neighbours is dropped when max(|dy - med_y|, |dx - med_x|) > max_dev, med the
 *   component-wise lower median (element (n - 1) / 2 of the sorted values) of those neighbours.  (2) field = 16 shift on
 *   the kept cells, which are known.  (3) Jacobi iterations on the previous iteration's state: every unknown cell with
 *   n >= 1 known 8-neighbours becomes floor((2 sum + n) / (2 n)) per component over them and known; until nothing is
 *   unknown (at most max(Gy, Gx) - 1 iterations).  No cell kept: all zeros, 0 iterations.  field int [Gy][Gx][2] in
 *   1/16 px; kept uint8 [Gy][Gx] (1 measured, 0 filled); stats int [2] = cells kept, iterations run; work int
 *   [6 Gy Gx].  Shape status for Gy Gx outside 1 .. 65536, max_shift outside 0 .. 1024, max_dev < 0.  One workgroup. */
int s2s_field_clean(const int* shift, const void* reliable, int Gy, int Gx, int max_dev, int max_shift, int* field,
                    void* kept, int* stats, int* work, void* stream);
int s2s_warp_region_u8(const void* src, long src_pitch, int src_row0, int src_rows, const int* field, int Gy, int Gx,
                       int cell, int max_shift, int H, int W, int C, int fill, int row0, int rows, void* out,
                       long out_pitch, void* stream);

/* ---- rigid region pre-alignment: overview maps and the rigid warp (rigid.hip) -----
 * s2s_structure_overview_u8: img = rows of a uint8 [H][W][3] region, any pitch >= 3 W and any base alignment; q_table and
 *   w HOST, as s2s_structure_map_u8 takes them; f the structure byte of that entry point; ds a power of two in 1 .. 64;
 *   out uint8 [H / ds][W / ds], contiguous = (sum of the ds x ds block of f + ds^2 / 2) / ds^2 over whole blocks (the sum
 *   is at most 64^2 255 < 2^32).  For ds in {1, 2, 4} this is s2s_structure_map_u8 bit for bit.  Shape status for another
 *   ds, H or W below ds or above 2^30, a pitch below a row, or a table and weights that could overflow int32.  One launch.
 * s2s_rigid_warp_u8: a transform is long [6] = (c, s, ty, tx, Cy, Cx): cosine and sine in Q24, the translation in 1/16
 *   pixel, the doubled centre (the centre of an H-row region is Cy = H - 1).  The kernel clamps c, s to +-2^24, ty, tx to
 *   +-2^36 and Cy, Cx to +-2^24.  For output pixel (y, x) with the displacement (dy, dx) in 1/16 pixel -- 0 when field is
 *   null, else the dense displacement of s2s_warp_region_u8, its +-16 max_shift clamp included -- in 64 bits:
 *     Uy = 32 y + 2 dy - 16 Cy, Ux = 32 x + 2 dx - 16 Cx; Vy = c Uy - s Ux, Vx = s Uy + c Ux;
 *     sy = ((Vy + Cy 2^28 + 2^24) >> 25) + ty (arithmetic shift), sx likewise with Cx and tx.
 *   That is out[p] = T[C + R (p + d - C) + t] with R = [[cos, -sin], [sin, cos]] acting on (y, x).  Sampling at (sy, sx)
 *   is that of s2s_warp_region_u8: nearest = 0 bilinear in 1/16 pixel with fill for a tap outside, nearest = 1 the tap at
 *   ((sy + 8) >> 4, (sx + 8) >> 4); either for C = 3 and for C = 1.  transform DEVICE long [A][6], any values: result a is
 *   written at out + a out_img.  src = rows [src_row0, src_row0 + src_rows) of the region; out = rows [row0, row0 + rows)
 *   of each result; a tap on a row that is not present takes the fill, so the caller provides the rows a band reads; no
 *   read leaves the rows present whatever the transform and the field hold.  Shape status for H or W outside 1 .. 2^20,
 *   A outside 1 .. 65535, a bad C, nearest, fill or band, a pitch smaller than a row, out_img < out_pitch rows for A > 1,
 *   and with a field the grid conditions of s2s_warp_region_u8.  One launch; the result does not depend on the banding. */
int s2s_structure_overview_u8(const void* img, long pitch, int H, int W, const int* q_table, const int* w, int ds,
                              void* out, void* stream);
int s2s_rigid_warp_u8(const void* src, long src_pitch, int src_row0, int src_rows, const long* transform, int A,
                      const int* field, int Gy, int Gx, int cell, int max_shift, int H, int W, int C, int nearest,
                      int fill, int row0, int rows, void* out, long out_pitch, long out_img, void* stream);

/* ---- tile quality control: focus, ink and dark-artefact counts (qc.hip) -----------
 * Integer throughout.  mx / mn = max / min(R, G, B); tissue = mn < white and mx >= black; Y = (77 R + 150 G + 29 B + 128)
 * >> 8; L(y, x) = Y(y-1, x) + Y(y+1, x) + Y(y, x-1) + Y(y, x+1) - 4 Y(y, x); a focus pixel is a tissue pixel with
 * 1 <= y <= H - 2 and 1 <= x <= W - 2 of the IMAGE (its neighbours may lie outside the window); green = tissue and
 * G - max(R, B) >= ink_chroma; blue = tissue and B - R >= ink_chroma and G >= R; dark = tissue and mx < dark.
 * A window is the win_h x win_w rectangle at origins[w] = (top, left), clipped to the image on all four sides; an owner
 * is window w of sample b, owner index b n + w.  Per owner eight int64 numbers: tissue, focus pixels, sum L, sum L^2
 * (over focus pixels), sum Y over tissue, green, blue, dark.
 * s2s_qc_chunks: chunks per window (16 rows x 256 columns each); a slab is long [B n chunks][8].  Shape status for
 *   sizes outside 1 .. 2^30.
 * s2s_qc_windows_u8: img = rows [band_top, band_top + band_h) of the uint8 [H][W][3] image, per sample at img_stride
 *   bytes, any pitch >= 3 W and any base alignment; origins DEVICE int [n][2], any values.  The launch accounts for image
 *   rows [row0, row1) of every window and writes its WHOLE slab (zeros for a chunk with no row in range).  Shape status
 *   when the rows present do not cover [max(0, row0 - 1), min(H, row1 + 1)), for white outside 1 .. 256, black outside
 *   0 .. 255, ink_chroma outside 1 .. 255, dark outside 0 .. 256, B outside 1 .. 65535, n chunks > 2^32.  One launch.
 * s2s_qc_finalize: counts long [owners][8] = (accumulate ? counts : 0) + the sum of the owner's nchunk chunks; launches
 *   over disjoint row ranges that together cover the image add up to the exact counts in any order.  derived double
 *   [owners][5], from the counts as they then stand, every operation rounded on its own and 0 where the denominator is
 *   0: focus = lap_sq / focus_n - (lap_sum / focus_n)^2, tissue / area (the window's pixels inside the image, from
 *   origins [n][2] and the sizes, owners a multiple of n), (green + blue) / tissue, dark / tissue, luma_sum / tissue.
 *   One launch. */
int s2s_qc_chunks(int win_h, int win_w);
int s2s_qc_windows_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
                      const int* origins, int n, int win_h, int win_w, int row0, int row1, int white, int black,
                      int ink_chroma, int dark, long* slab, void* stream);
int s2s_qc_finalize(const long* slab, long owners, int nchunk, int accumulate, const int* origins, int n, int H, int W,
                    int win_h, int win_w, long* counts, double* derived, void* stream);

/* ---- result rendering: overlays, heat maps, comparisons, thumbnails (render.hip) ---
 * Integer throughout.  mix(b, c, a) = (b (256 - a) + c a + 128) >> 8 per channel, a in 0 .. 256: a = 0 returns b and
 * a = 256 returns c exactly.  A region is a base pointer, a row pitch in bytes (any pitch >= a row, any base alignment),
 * H and W, both in 1 .. 2^30.  A launch writes rows [row0, row0 + rows); base, a, b and out point at row row0.  An input
 * that is read at neighbouring rows is present at rows [src_row0, src_row0 + src_rows) and points at row src_row0.
 * Everything is computed from global coordinates, so the bytes do not depend on the banding.  A null pointer returns the
 * null status and every shape, range or pitch violation the shape status, before any HIP call.  out may be base itself
 * (same pointer and pitch): an output pixel reads only its own base pixel.  One launch each.
 * s2s_render_classes_u8 / s2s_render_labels_u8: base uint8 [H][W][3]; a uint8 class mask [H][W] or an int label image
 *   [H][W] (pitch in bytes, a multiple of 4; the pointer dword-aligned, else the alignment status); palette DEVICE uint8
 *   [256][3]; fill_alpha DEVICE int [256], entries in 0 .. 256 (the kernel clamps them); edge radius r in 0 .. 4;
 *   edge_alpha in 0 .. 256; edge_rgb = -1 (the edge takes the palette colour) or 0xRRGGBB.  Per pixel p: id(p) = the mask
 *   byte, or max(L, 0); k(p) = the mask byte, or 0 for L <= 0 and ((L - 1) mod 255) + 1 otherwise.  p is an edge pixel iff
 *   r >= 1, id(p) != 0 and some offset with 1 <= |dy| + |dx| <= r leads to a pixel q outside [0, H) x [0, W) of the whole
 *   region or with id(q) != id(p): identities are compared, not colours; with r = 1 on a binary mask this is the rule of
 *   s2s_mask_boundary.  out = mix(base, edge colour, edge_alpha) on edge pixels, mix(base, palette[k], fill_alpha[k])
 *   otherwise.  Shape status unless the mask rows present cover [max(0, row0 - r), min(H, row0 + rows + r)); the kernel
 *   tests every neighbour against the region, so no mask content moves a read.
 * s2s_render_heat_u8: Q DEVICE int [Gy][Gx], one node per cell x cell cell, Gy in {H / cell, ceil(H / cell)} and >= 1, Gx
 *   alike, Gy Gx <= 65536, cell in 1 .. 2^14; lut DEVICE uint8 [256][3]; alpha and min_index in 0 .. 256; smooth 0 or 1.
 *   smooth = 0: g = min(p / cell, G - 1) per axis, d = Q[gy][gx].  smooth = 1: the dense interpolation of
 *   s2s_warp_region_u8 with D = Q (nodes at the cell centres, doubled coordinates, span = 2 cell, the nearest node outside
 *   the centres), d = floor((num + span^2 / 2) / span^2), without the max_shift clamp.  d is clamped to 0 .. 65280 =
 *   255 * 256 by the kernel, whatever Q holds (num < 2^46 for nodes in range, below 2^62 for any int).  idx = (d + 128)
 *   >> 8; out = mix(base, lut[idx], alpha) where idx >= min_index, base otherwise.
 * s2s_render_compare_u8: a, b uint8 [H][W][3].  mode 0: a where (y / cell + x / cell) is even, b otherwise; mode 1:
 *   mix(a, b, alpha); mode 2: min(255, |a - b| gain).  cell in 1 .. 2^30, alpha in 0 .. 256, gain in 1 .. 255, each
 *   checked whatever the mode.
 * s2s_box_down_u8: src = rows [src_row0, src_row0 + src_rows) of a uint8 [H][W][C] region, C = 3 or 1; f in 1 .. 256; out
 *   = rows [row0, row0 + rows) of the uint8 [ceil(H / f)][ceil(W / f)][C] result.  An output pixel covers the n pixels of
 *   its f x f block that lie inside the region.  C = 3: floor((2 sum + n) / (2 n)) (sum <= 255 * 65536); C = 1: the
 *   maximum.  Shape status unless the source rows present cover [row0 f, min(H, (row0 + rows) f)).  f = 1 is a copy. */
int s2s_render_classes_u8(const void* base, long base_pitch, const void* mask, long mask_pitch, int mask_row0,
                          int mask_rows, const void* palette, const int* fill_alpha, int r, int edge_alpha, int edge_rgb,
                          int H, int W, int row0, int rows, void* out, long out_pitch, void* stream);
int s2s_render_labels_u8(const void* base, long base_pitch, const int* labels, long labels_pitch, int labels_row0,
                         int labels_rows, const void* palette, const int* fill_alpha, int r, int edge_alpha, int edge_rgb,
                         int H, int W, int row0, int rows, void* out, long out_pitch, void* stream);
int s2s_render_heat_u8(const void* base, long base_pitch, const int* Q, int Gy, int Gx, int cell, const void* lut,
                       int alpha, int min_index, int smooth, int H, int W, int row0, int rows, void* out, long out_pitch,
                       void* stream);
int s2s_render_compare_u8(const void* a, long a_pitch, const void* b, long b_pitch, int mode, int cell, int alpha, int gain,
                          int H, int W, int row0, int rows, void* out, long out_pitch, void* stream);
int s2s_box_down_u8(const void* src, long src_pitch, int src_row0, int src_rows, int H, int W, int C, int f, int row0,
                    int rows, void* out, long out_pitch, void* stream);

/* ---- loss variants and class conditioning (loss_variants.hip) -- SURVEY section 8 row f4 -----------------
 * ROI-weighted MSE (conditional_flow_matching_masked.py:76-90): w = 1 + roi_lambda * mask,
 *   out[0] = sum(w (v-u)^2) / (sum(w) + 1e-8), w broadcast over C.  v, u: float[B][C][HW]; mask: float[B][HW];
 *   dv optional; work: double[512*2 + 2].
 * ROI Charbonnier (conditional_flow_matching_ROI_loss.py:78-95): out[0] = sum(sqrt((p-t)^2 + eps_charb^2) * mask)
 *   / (sum(mask) * C + eps_area); value only (its inputs are data).
 * Class conditioning (class_conditional_flow_matching.py:39-71, build-defined network side): out = temb + table[y]. */
int s2s_weighted_mse(const float* v, const float* u, const float* mask, float* dv, float* out, double* work, long B,
                     int C, long HW, float roi_lambda, float grad_scale, void* stream);
int s2s_charbonnier_roi(const float* pred, const float* truth, const float* mask, float* out, double* work, long B,
                        int C, long HW, float eps_charb, float eps_area, void* stream);
int s2s_class_embed_add(const float* temb, const float* table, const long* y, float* out, int B, int dim,
                        void* stream);
int s2s_class_embed_bwd(const float* dout, const long* y, float* dtable, int accumulate, int B, int dim,
                        int num_classes, void* stream);

/* ---- InstanceNorm2d + LeakyReLU, fused (instnorm.hip) ----------------------------------------------
 * Row a13 of SURVEY.md section 8 (pix2pix generator / PatchGAN discriminator named by BASELINE.json's north_star).
 * The reference repository has no such model, so these replace no reference line: the semantics are
 * torch's nn.InstanceNorm2d(C, eps, affine = gamma/beta given or both NULL, no running statistics) followed by
 * nn.LeakyReLU(slope) (slope 0 = ReLU), NHWC with a pixel stride, C % 8 == 0.
 * work: float[2*B*C*s2s_instnorm_blocks()] for the forward, that + 2*B*C for the backward.
 * stats: float[4][B][C] = mean, 1/std, scale, shift; written by the forward, read by the backward.
 * backward: dx = d/dx of sum(g * y); dgamma/dbeta (both or neither) receive or accumulate the affine gradients.  x and
 * eps are the forward's: the fp32 single-launch form (no dgamma, at most 32 x 32) takes mean and 1/std again from x in
 * fp64 -- on a map of a few pixels dx is what a cancellation down to eps / (var + eps) leaves, beyond an fp32 1/std -- and
 * reads stats only for the sign of z and the scale; every other form reads mean and 1/std from stats and ignores eps. */
int s2s_instnorm_blocks(int B, int H, int W, int C);
int s2s_instnorm_lrelu_fwd(int dtype, const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy,
                           float* work, float* stats, int B, int H, int W, int C, float eps, float slope,
                           void* stream);
int s2s_instnorm_lrelu_bwd(int dtype, const void* g, int ldg, const void* x, int ldx, const float* stats, void* dx,
                           int lddx, float* dgamma, float* dbeta, int accumulate, float* work, int B, int H, int W,
                           int C, float eps, float slope, void* stream);

/* ---- 2x2-tap convolution on the MFMA loop (conv3x3_mfma.hip) -----------------------------------------
 * Row a13 again (no reference line to replace): nn.Conv2d(k=4, stride=2, padding=1) of a pix2pix
 * encoder / PatchGAN layer is a 2x2 "valid" convolution over the space-to-depth image of the zero-padded input
 * (4*Cin channels, no wasted MACs) - pad = 0, input (H+1) x (W+1) - and its data gradient, which is also
 * nn.ConvTranspose2d(k=4, stride=2, padding=1), is the same loop with flipped taps - pad = 1, input (H-1) x (W-1).
 * H, W: OUTPUT size.  w_packed: bf16 [ceil(cin/32)][tap a*2+b][Cout][32].  bf16 only so far.
 * stat_part (optional): float[2][Cout][s2s_conv2x2_stat_blocks()] as for the 3x3 kernel. */
int s2s_conv2x2_stat_blocks(int B, int H, int W, int Cout);
int s2s_conv2x2_nhwc(int dtype, const void* x, int ldx, int cin, const void* w_packed, const float* bias, void* y,
                     int ldy, float* stat_part, int B, int H, int W, int Cout, int pad, void* stream);
/* Layout change ahead of s2s_conv2x2_nhwc: xs[n][p][q][(r*2+s)*C + c] = xpad[n][2p+r][2q+s][c] with xpad = x plus a
 * one-pixel zero border; x [B][H][W][C] (H, W even), xs [B][H/2+1][W/2+1][4C].  inverse != 0 writes x from xs (the data
 * gradient's way back; the border cells are dropped).  bf16. */
int s2s_space_to_depth_pad1(int dtype, const void* x, int ldx, void* xs, int ldxs, int inverse, int B, int H, int W,
                            int C, void* stream);
/* out[c] (+)= sum over the npix pixels of an NHWC tensor (bias gradient of the 4x4 layers); work:
 * float[2*C*s2s_channel_sum_blocks()]. */
int s2s_channel_sum_blocks(long npix, int C);
int s2s_channel_sum(int dtype, const void* x, int ldx, float* work, float* out, long npix, int C, int accumulate,
                    void* stream);
/* fp32 master weight [Cout][Cin][4][4] of a 4x4 layer -> its two bf16 MFMA operands: wf (forward,
 * [ceil(K/32)][taps][Cout][32]) and wd (data gradient / transposed form, [ceil(Cout/32)][taps][K][32], taps flipped);
 * stride 2: taps = 4, K = 4*Cin (space-to-depth channel order); stride 1: taps = 16, K = Cin. */
int s2s_pack_conv4x4(const float* w_oihw, void* wf, void* wd, int Cout, int Cin, int stride, void* stream);
/* nn.Conv2d(k=4, stride=1, padding=1) of the PatchGAN's last two layers (pad = 1, input (H+1) x (W+1)) and its data
 * gradient (pad = 2, input (H-1) x (W-1), taps flipped by the packing) on the same loop with 16 taps.
 * w_packed: bf16 [ceil(cin/32)][tap kh*4+kw][Cout][32]. */
int s2s_conv4x4s1_nhwc(int dtype, const void* x, int ldx, int cin, const void* w_packed, const float* bias, void* y,
                       int ldy, float* stat_part, int B, int H, int W, int Cout, int pad, void* stream);
/* weight gradient of the pad = 1 form: grad16[tap kh*4+kw][Cout][cin] (+)= sum over the batch, dY [B][H][W][Cout],
 * X [B][H+1][W+1][cin]; part: float[s2s_conv4x4s1_wgrad_splits()][16][Cout][cin] scratch. */
int s2s_conv4x4s1_wgrad_splits(int B, int H, int W, int Cin, int Cout);
int s2s_conv4x4s1_wgrad_nhwc(int dtype, const void* dy, int lddy, int Cout, const void* x, int ldx, int cin,
                             float* part, float* grad16, int accumulate, int B, int H, int W, void* stream);
/* weight gradient of the pad = 0 form: grad2[tap a*2+b][Cout][cin] (+)= sum_{n,i,j} dY[n][i][j][:] x X[n][i+a][j+b][:],
 * dY [B][H][W][Cout], X [B][H+1][W+1][cin]; part: float[s2s_conv2x2_wgrad_splits()][4][Cout][cin] scratch. */
int s2s_conv2x2_wgrad_splits(int B, int H, int W, int Cin, int Cout);
int s2s_conv2x2_wgrad_nhwc(int dtype, const void* dy, int lddy, int Cout, const void* x, int ldx, int cin, float* part,
                           float* grad2, int accumulate, int B, int H, int W, void* stream);

/* ---- the pix2pix G + D step's remaining kernels (row a13; no reference line to replace) -------------
 * General form of the two convolutions above, both dtypes (fp32 = three-way bf16 split, the parity mode):
 *   ks = 2, pad 0 | 1: 4x4 stride-2 convolution on the space-to-depth image | its data gradient = transposed convolution
 *   ks = 4, pad 1 | 2: 4x4 stride-1 convolution | its data gradient.          H, W: OUTPUT size.
 * w_packed: [ceil(cin/32)][ks*ks][Cout][32] in the activation dtype (s2s_pack_conv4x4_t).
 * act != 0: y = t > 0 ? t : act_slope * t on the bias-added output (the layers WITHOUT a norm: LeakyReLU(0.2) / ReLU).
 * y2 (optional, pixel stride ldy2): a second copy max(y, 0), the ReLU'd skip tensor written into the decoder's
 * concatenation buffer.  bias_mod (0 = Cout): the bias of output channel n is bias[n % bias_mod] -- Cout / 4 for the
 * transposed layers, whose four sub-pixel channel groups share the layer's bias vector.  stat_part (optional): float[2][Cout][s2s_convkxk_stat_blocks()]. */
int s2s_convkxk_stat_blocks(int dtype, int B, int H, int W, int Cout, int ks);
int s2s_convkxk_nhwc(int dtype, const void* x, int ldx, int cin, const void* w_packed, const float* bias, int bias_mod,
                     void* y, int ldy, void* y2, int ldy2, int act, float act_slope, float* stat_part, float* kwork, int B,
                     int H, int W, int Cout, int ks, int pad, void* stream);
/* Split-K for the small maps of the inner U-Net levels: with kwork = float[s2s_convkxk_ksplit()][B*H*W][Cout] (optional,
 * bf16 only) that many workgroups share an output tile, each reducing a range of the input-channel chunks, and a
 * second launch folds the fp32 partial tiles (+ bias, activation).  Returns 1 when the launch is not split. */
int s2s_convkxk_ksplit(int dtype, int B, int H, int W, int Cout, int cin, int ks);
/* Weight gradient of the pad-0 (ks = 2) / pad-1 (ks = 4) forms: dY [B][H][W][Cout], X [B][H+1][W+1][cin].
 * layout 0: grad[ks*ks][Cout][cin]; layout 1: nn.Conv2d's [Cout][C][4][4] (ks = 2: cin = 4 C over the space-to-depth
 * channels; with the roles of a transposed layer's input and output gradient exchanged the same call yields
 * nn.ConvTranspose2d's [Cin][Cout][4][4]).  part: float[s2s_convkxk_wgrad_splits()][ks*ks][Cout][cin] scratch. */
int s2s_convkxk_wgrad_splits(int dtype, int B, int H, int W, int Cin, int Cout, int ks);
int s2s_convkxk_wgrad_nhwc(int dtype, const void* dy, int lddy, int Cout, const void* x, int ldx, int cin, float* part,
                           float* grad, int layout, int accumulate, int B, int H, int W, int ks, int x_plain, void* stream);
/* The 4x4 stride-2 layers without a layout pass (bf16): s2s_conv4x4s2_nhwc reads the PLAIN input x [B][2H][2W][Cin]
 * (Cin a power of two; the loader does the space-to-depth in its addresses) -> y [B][H][W][Cout];
 * s2s_convt4x4s2_nhwc is the transposed layer / the convolution's data gradient by sub-pixel phase, x [B][h][w][Cin] ->
 * PLAIN y [B][2h][2w][C] (C % 64 == 0), wd = the data-gradient operand of s2s_pack_conv4x4.  kwork (optional):
 * float[..._ksplit()][output pixels][channels] for the split-K form of the small maps.  The weight gradient takes the
 * plain tensor with x_plain = 1 in s2s_convkxk_wgrad_nhwc (cin = 4 C stays the virtual channel count).
 * s2s_conv4x4s2_plan / s2s_convt4x4s2_plan (host only): the launch plan such a call takes when it is given kwork, 0..5 =
 * the tile plans 8x32x128, 8x32x64, 4x32x128, 4x32x64, 8x16x128, 8x16x64 (rows x columns x channels of one workgroup),
 * 6 = the flat form of the power-of-two maps up to 8 x 8; a negative status for bad arguments. */
int s2s_conv4x4s2_ksplit(int B, int H, int W, int Cout, int Cin);
int s2s_conv4x4s2_plan(int B, int H, int W, int Cout, int Cin);
int s2s_conv4x4s2_nhwc(int dtype, const void* x, int ldx, int Cin, const void* wf, const float* bias, void* y, int ldy,
                       void* y2, int ldy2, int act, float act_slope, float* kwork, int B, int H, int W, int Cout,
                       void* stream);
int s2s_convt4x4s2_ksplit(int B, int h, int w, int C, int Cin);
int s2s_convt4x4s2_plan(int B, int h, int w, int C, int Cin);
int s2s_convt4x4s2_nhwc(int dtype, const void* x, int ldx, int Cin, const void* wd, const float* bias, void* y, int ldy,
                        float* kwork, int B, int h, int w, int C, void* stream);
/* The same two layers on the generator's INNER levels as ONE launch with what follows them (conv_small.hip; bf16):
 * a workgroup owns whole samples x 16 output channels and all of K, so there is no split-K, no partial slab and no
 * reduce, and InstanceNorm + activation (forward) or their backward (data gradient) are the epilogue.
 *   mode 1: nn.Conv2d(4, 2, 1) from the plain x [B][2h][2w][Cin] with wf -> [B][h][w][Cout], h * w <= 64;
 *   mode 2: nn.ConvTranspose2d(4, 2, 1) / the convolution's data gradient from x [B][h][w][Cin] with wd ->
 *           [B][2h][2w][Cout], h * w <= 16.   h, w powers of two, Cin % 64 == 0, Cout % 16 == 0; s2s_convsm_ok() != 0 says a shape is taken.
 *   epi 0: y = act ? lrelu(conv + bias, slope) : conv + bias; y2 (optional) = relu(y).
 *   epi 1: raw (optional) = bf16(conv + bias); stats[4][B][Cout] = mean, invstd, invstd, -mean * invstd of raw per
 *          (sample, channel) [InstanceNorm2d(affine=False, eps)]; y = lrelu(norm(raw), slope); y2 (optional) = relu(norm).
 *   epi 2: g = conv (no bias).  Output channels [0, bwd_c0): y2 = g (pixel stride ldy2, channel index unchanged).
 *          Output channels [bwd_c0, Cout), as channel c - bwd_c0 of z / stats_in / g2 / y: the backward of epi 1 for
 *          that tensor, dzn = norm(z) > 0 ? g + g2 : slope * g, y = invstd * (dzn - mean(dzn) - xhat * mean(dzn xhat)). */
int s2s_convsm_ok(int dtype, int mode, int B, int h, int w, int Cin, int Cout);
int s2s_convsm_nhwc(int dtype, int mode, const void* x, int ldx, int Cin, const void* w_packed, const float* bias, int epi,
                    int act, float slope, float eps, void* raw, int ldraw, void* y, int ldy, void* y2, int ldy2,
                    float* stats, const float* stats_in, const void* z, int ldz, const void* g2, int ldg2, int bwd_c0,
                    int B, int h, int w, int Cout, void* stream);
/* InstanceNorm + LeakyReLU with a second output y2 = relu(z) (pixel stride ldy2, optional) and, backward, a second
 * incoming gradient g2 (wrt y2, optional): dz = z > 0 ? g + g2 : slope * g.  Otherwise as s2s_instnorm_lrelu_fwd/bwd. */
int s2s_instnorm_lrelu_fwd2(int dtype, const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy,
                            void* y2, int ldy2, float* work, float* stats, int B, int H, int W, int C, float eps,
                            float slope, void* stream);
int s2s_instnorm_lrelu_bwd2(int dtype, const void* g, int ldg, const void* g2, int ldg2, const void* x, int ldx,
                            const float* stats, void* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                            float* work, int B, int H, int W, int C, float eps, float slope, void* stream);
/* The single-launch forms (bf16, no affine, maps of at most 32 x 32: s2s_instnorm_split_ok() != 0) with the input folded
 * from a split-K convolution's partial slabs, float[S][B*H*W][C] as s2s_conv4x4s2_nhwc / s2s_convt4x4s2_nhwc leave them in
 * kwork when called with y == NULL -- one launch instead of reduce + norm, bit-identical to the two-launch form.
 * fwd: raw (bf16, what the backward reads) <- fold + bias, then s2s_instnorm_lrelu_fwd2 on it; bwd: g <- fold. */
int s2s_instnorm_split_ok(int dtype, int H, int W, int C);
int s2s_instnorm_lrelu_fwd_split(int dtype, const float* slabs, int S, const float* bias, void* raw, int ldraw, void* y,
                                 int ldy, void* y2, int ldy2, float* stats, int B, int H, int W, int C, float eps,
                                 float slope, void* stream);
int s2s_instnorm_lrelu_bwd_split(int dtype, const float* gslabs, int S, const void* g2, int ldg2, const void* x, int ldx,
                                 const float* stats, void* dx, int lddx, int B, int H, int W, int C, float slope,
                                 void* stream);
/* s2s_pack_conv4x4 with the operands in the activation dtype; the batched form re-packs every 4x4 layer of a network in
 * one launch after the fused Adam step: desc = device long[nlayers][7] {w master, wf, wd, Cout, Cin, stride == 2, first
 * block}, a layer occupies s2s_pack_conv4x4_blocks() blocks, total = their sum. */
int s2s_pack_conv4x4_t(int dtype, const float* w_oihw, void* wf, void* wd, int Cout, int Cin, int stride, void* stream);
long s2s_pack_conv4x4_blocks(int Cout, int Cin, int stride);
int s2s_pack_conv4x4_batched(int dtype, const void* desc, int nlayers, long total, void* stream);
/* out[B][H][W][8] (pixel stride ldo) <- [a (ca channels) | b (cb channels, optional) | zeros] from NCHW fp32 images: the
 * generator's input (source tile) and the discriminator's (source | target). */
int s2s_p2p_pack_input(int dtype, const float* a_nchw, int ca, const float* b_nchw, int cb, void* out, int ldo, int B,
                       int H, int W, void* stream);
/* The inverse for gradients: out_nchw[n][c][p] (fp32) = in[n][p][c0 + c], in = an 8-channel NHWC image (pixel stride ldi). */
int s2s_p2p_unpack(int dtype, const void* in, int ldi, int c0, int C, float* out_nchw, int B, int H, int W, void* stream);
/* Generator head: fake = tanh(h[..., :C]); d_in <- [src | fake | zeros] (the discriminator's input, 8 channels);
 * fake_nchw (optional) <- fake as NCHW fp32; l1_out[0] = mean |fake - tgt|.  work: double[s2s_p2p_tanh_l1_blocks()]. */
int s2s_p2p_tanh_l1_blocks(int B, int H, int W);
int s2s_p2p_tanh_l1_fwd(int dtype, const void* h, int ldh, const float* src_nchw, const float* tgt_nchw, void* d_in,
                        int ldd, float* fake_nchw, float* l1_out, void* work, int B, int H, int W, int C, void* stream);
/* dh[..., c] = (l1_scale * sign(fake - tgt) + gd[..., C + c]) * (1 - fake^2) for c < C, 0 on the padding channels;
 * gd (optional) = gradient wrt the discriminator's input. */
int s2s_p2p_tanh_l1_bwd(int dtype, const void* h, int ldh, const float* tgt_nchw, const void* gd, int ldg, float l1_scale,
                        void* dh, int lddh, int B, int H, int W, int C, void* stream);
/* BCEWithLogits of a PatchGAN logit map z[N][HW][ldz] (logit = channel 0): samples n < n_real against ones, the others
 * against zeros.  out2[0] / out2[1] = the two means; dz (optional, 8 channels, pixel stride lddz)[..., 0] =
 * w_real * (sigmoid(z) - 1) | w_fake * sigmoid(z), 0 on the padding channels. */
int s2s_p2p_bce_logits(int dtype, const void* z, int ldz, int n_real, float w_real, float w_fake, void* dz, int lddz,
                       float* out2, int N, int HW, void* stream);
/* The same spread over s2s_p2p_bce_blocks(N, HW) workgroups (one workgroup's softplus / sigmoid arithmetic for a
 * batch-64 map is 20-40 us); work: double[2 * s2s_p2p_bce_blocks(N, HW)], summed in workgroup order. */
int s2s_p2p_bce_blocks(int N, int HW);
int s2s_p2p_bce_logits_w(int dtype, const void* z, int ldz, int n_real, float w_real, float w_fake, void* dz, int lddz,
                         float* out2, double* work, int N, int HW, void* stream);
/* Backward of a LeakyReLU / ReLU without a norm in front, from its stored output a: dz = a > 0 ? g + g2 : slope * g
 * (g2 optional: the gradient wrt the ReLU'd copy); dbias (optional) (+)= per-channel sum of dz.
 * work: float[C * s2s_p2p_act_bwd_blocks()]. */
int s2s_p2p_act_bwd_blocks(long npix, int C);
int s2s_p2p_act_bwd(int dtype, const void* g, int ldg, const void* g2, int ldg2, const void* a, int lda, float slope,
                    void* dz, int lddz, float* work, float* dbias, int accumulate, long npix, int C, void* stream);

/* ---- stain background subtraction: grey opening and top-hat (grey_morph.hip) ----------
 * Grey images are uint8 (dtype 0) or int16 (dtype 1) [B][H][.] with pitch and img_stride in ELEMENTS; results are dense
 *   [B][H][W].  H, W <= 32767 and B <= 65535; the radius is at most MAX_RADIUS = 128 and smooth at most 16; anything
 *   beyond is refused with the shape status before any launch.  Nothing lies outside the image: a minimum or maximum
 *   runs over the in-image pixels of the footprint only (scipy.ndimage.grey_erosion(mode="constant", cval=type max) and
 *   grey_dilation(cval=type min)).
 * Footprints: 0 disc, {(dy, dx): dy^2 + dx^2 <= size}, size = floor(radius^2) <= 128^2 (the r2 of s2s_morph_threshold);
 *   1 square, |dy|, |dx| <= size = floor(radius) <= 128.
 * Operations: 0 erode (min), 1 dilate (max), 2 open = dilate(erode), 3 close = erode(dilate), 4 tophat = x - open(x),
 *   5 bothat = close(x) - x; the differences are formed in 32 bits and saturated to the dtype.
 * s2s_grey_words: the int32 words of scratch s2s_grey_morph needs (the span tables of one pass and one intermediate
 *   plane); negative: a status code.  scratch must be 2-byte aligned.
 * s2s_grey_morph: 1 + levels launches per erosion or dilation (levels = floor(log2(min(2 floor(radius) + 1, W))) + 1),
 *   twice that for the four compound operations.  Every element of out is written.
 * s2s_grey_box_mean: int16 values >= 0, dense: out = (2 sum + n) / (2 n) in integer division, sum and n over the
 *   in-image pixels of the (2 smooth + 1)^2 window; smooth = 0 copies.
 * s2s_grey_bins_u8 / _f32: images, od_table, unmix (nine floats are read), white, black as in stain threshold
 *   calibration; bins short [B][rows][W] = bin(c_stain) = clamp(ceil(c * 1024) - 1, 0, 4095) of EVERY pixel (no tissue
 *   gate), with the fp32 operations of s2s_stain_hist_*; tissue (bytes, may be null) = the tissue rule, 0 / 1.  The uint8
 *   buffers hold `rows` rows of B images (pitch, img_stride in bytes).
 * s2s_grey_corrected: t = max(bins - bg, 0) (bg null: t = bins) over rows [row0, row0 + nrows) of dense short
 *   [B][rows][W] buffers (the other rows are a band's halo: read by the morphology, not counted here).  An owner is a
 *   sample, or the batch (pool != 0).  counts long [owners][3] += tissue pixels, tissue pixels with t >= j (j in
 *   1..4095), the sum of t over tissue; hist long [owners][3][4096]: row `stain` += tissue pixels by t.  64-bit integer
 *   atomics; reset != 0 zeroes all of counts and hist first, in a launch of its own.  mask (bytes, may be null): bit 0
 *   positive, bit 1 tissue; corrected (short, may be null): t; both [B][nrows][W] with out_img elements per sample.
 *   A launch whose workgroups would count 2^32 pixels or more each is refused.
 * s2s_grey_corrected_finalize: out double [owners][2] = positive / max(tissue, 1), sum_t / max(tissue, 1).
 * s2s_grey_pair: both long [B] = the pixels with bit 0 set in both of two dense byte masks [B][H][W] (written).
 * s2s_grey_pair_finalize: counts_a / counts_b as s2s_grey_corrected leaves them for B owners: out double [B][5] = the
 *   two burdens, their absolute difference, Dice = 2 both / (positive_a + positive_b) and IoU, both 1 when both masks
 *   are empty. */
long s2s_grey_words(int B, int H, int W, int footprint, int size);
int s2s_grey_morph(const void* src, int dtype, long pitch, long img_stride, int B, int H, int W, int op, int footprint,
                   int size, int* scratch, void* out, void* stream);
int s2s_grey_box_mean(const short* src, int B, int H, int W, int smooth, short* out, void* stream);
int s2s_grey_bins_u8(const void* img, long pitch, long img_stride, int B, int rows, int W, const float* od_table,
                     const float* unmix, int white, int black, int stain, short* bins, void* tissue, void* stream);
int s2s_grey_bins_f32(const float* img, int B, int H, int W, const float* od_table, const float* unmix, int white,
                      int black, int stain, short* bins, void* tissue, void* stream);
int s2s_grey_corrected(const short* bins, const short* bg, const void* tissue, int B, int rows, int W, int row0,
                       int nrows, int j, int stain, int pool, int reset, long* counts, long* hist, void* mask,
                       short* corrected, long out_img, void* stream);
int s2s_grey_corrected_finalize(const long* counts, long owners, double* out, void* stream);
int s2s_grey_pair(const void* mask_a, const void* mask_b, int B, int H, int W, long* both, void* stream);
int s2s_grey_pair_finalize(const long* counts_a, const long* counts_b, const long* both, int B, double* out,
                           void* stream);

/* ---- hysteresis thresholding: the dual-threshold mask (hysteresis.hip) ------------------
 * s2s_hyst_mask: t short [B][rows][W] on the 1/1024 OD grid (the bins of s2s_grey_bins_*, or the corrected t of
 *   s2s_grey_corrected) and tissue bytes of the same layout (0 / not 0; null: every pixel is tissue), over rows
 *   [row0, row0 + nrows) (the other rows are a band's halo).  0 <= j_low <= j_high <= 4095.  mask bytes [B][nrows][W]
 *   with out_img elements per sample, every one written: bit 0 = tissue and t >= j_low (weak), bit 1 = tissue, bit 2 =
 *   tissue and t >= j_high (strong).  An owner is a sample, or the batch (pool != 0).  counts long [owners][3] += the
 *   tissue, weak and strong pixels (64-bit integer atomics, one set per workgroup); reset != 0 zeroes counts first, in a
 *   launch of its own.  rows, W <= 32767, B <= 65535; a launch whose workgroups would count 2^32 pixels or more each is
 *   refused.  The hysteresis mask is s2s_objects_label_seeded of this byte with fg_bits = 1, seed_bits = 4.
 * s2s_hyst_finalize: positive long [owners], counts as s2s_hyst_mask leaves them: burden double [owners] =
 *   positive / max(tissue, 1). */
int s2s_hyst_mask(const short* t, const void* tissue, int B, int rows, int W, int row0, int nrows, int j_low, int j_high,
                  int pool, int reset, long* counts, void* mask, long out_img, void* stream);
int s2s_hyst_finalize(const long* positive, const long* counts, long owners, double* burden, void* stream);

/* ---- streams (runtime.hip) -------------------------------------------------------------------------
 * A HIP stream confined to the compute units whose bits are set in mask_words (bit i of word i/32 = CU i, as
 * hipExtStreamCreateWithCUMask numbers them); *out_stream receives the hipStream_t.  Used for the weight-gradient side
 * stream of the fused trainers; any hipStream_t may be passed as `stream` to every entry point above. */
int s2s_stream_create_cu_mask(const unsigned* mask_words, int n_words, long* out_stream);
int s2s_stream_destroy(void* stream);
/* Events for timing brackets: timing_only != 0 creates the event with hipEventDisableSystemFence (a timestamp marker
 * without the system-scope fence of a default event); elapsed_ms wants both events complete. */
int s2s_event_create(int timing_only, long* out_event);
int s2s_event_record(void* event, void* stream);
int s2s_event_elapsed_ms(void* start, void* stop, float* out_ms);
int s2s_event_synchronize(void* event);
int s2s_event_destroy(void* event);

#ifdef __cplusplus
}
#endif
#endif /* STAIN2STAIN_HIP_H */
