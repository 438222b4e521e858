/* dfd_hip.h — C ABI of libdfd_hip.so: the MI355X (gfx950) kernels behind the
 * DeepfakeDetection image-classifier hot loop.
 *
 * The reference (thourihan/DeepfakeDetection) has no FFI of its own: its hot loop
 * calls third-party nn.Modules (efficientnet_pytorch 0.7.1 / timm 1.0.20) whose
 * arithmetic runs in ATen/cuDNN.  Every entry point below therefore cites the
 * reference CALL SITE whose arithmetic it carries:
 *
 *   forward          logits = model(inputs)            trainers/efficientnet.py:297, :254
 *                                                      orchestration/orchestrator.py:529, :590
 *   loss             criterion(logits, targets)        trainers/efficientnet.py:298, :412
 *   backward         scaler.scale(loss).backward()     trainers/efficientnet.py:302
 *   optimizer        scaler.step(opt)                  trainers/efficientnet.py:305-306, :487-491
 *   inference tail   softmax(dim=1) / argmax           orchestration/orchestrator.py:591-592
 *
 * Rules of the boundary ("B-inner"):
 *   - plain pointers and sizes only; no torch types.
 *   - every buffer (inputs, outputs, workspaces, partial-sum slabs) is allocated by
 *     the caller; the library never allocates, frees or keeps a pointer past return.
 *   - every call only enqueues work on `stream` and never synchronises; it is safe
 *     under hipGraph stream capture and re-entrant across host threads.
 *   - return value: DFD_OK or a negative DFD_E* code; no exceptions cross the ABI.
 *   - layouts: activations NHWC ([N*H*W][C] row-major) of dtype DFD_F32 or DFD_BF16,
 *     C % 8 == 0; depthwise weights [C][k][k] f32 (torch's [C,1,k,k]); pointwise
 *     weights [Cout][Cin]; BN statistics / coefficients / SE gates f32.
 *   - reductions over rows (BN statistics, weight gradients) are written as
 *     per-workgroup partial slabs and summed by a second kernel in a fixed order:
 *     results are bitwise reproducible run to run.
 */
#ifndef DFD_HIP_H
#define DFD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dfd_stream;          /* a hipStream_t */

#define DFD_OK            0
#define DFD_EINVAL       (-1)      /* bad argument / shape not divisible as required */
#define DFD_EUNSUPPORTED (-2)      /* kernel size / stride / activation not implemented */
#define DFD_ELAUNCH      (-3)      /* hipGetLastError() != hipSuccess after the launch */
#define DFD_EWORKSPACE   (-4)      /* caller's workspace too small */

#define DFD_F32   0
#define DFD_BF16  1

#define DFD_ACT_NONE 0
#define DFD_ACT_SILU 1
#define DFD_ACT_RELU 2
#define DFD_ACT_GELU 3

/* upper bound on the number of partial-sum rows any kernel writes */
#define DFD_MAX_PARTIALS 1024

/* BN state: float[4][C] = scale, shift, mean, rstd  (z = scale*y + shift)
 * BN backward coefficients: float[3][C] = a, b, c   (dy = a*g + b*y + c)      */
#define DFD_BNSTATE_ROWS 4
#define DFD_BNCOEF_ROWS  3

/* ABI revision: 100 = first release; 101 = workspace arguments on the pooling entry points,
 * dfd_pool_ws, dfd_image_prep; 102 = dfd_prep_weights_multi, dfd_se_fc_fwd accepts a prepared w2t;
 * 110 = the EfficientFormerV2 / FasterViT set (section "token mixers" below), the *_ex BatchNorm entry
 * points (convolution bias and LayerScale folded into the BatchNorm coefficients), GELU in every
 * prologue, and the bookkeeping kernels (dfd_rand, dfd_step_tick, dfd_axpby, dfd_add);
 * 111 = dfd_se_fwd / dfd_se_bwd (squeeze-excite in two / three launches); dfd_rowtable_grad takes a workspace;
 * dfd_conv_fwd / dfd_conv_wgrad (implicit-GEMM dense convolution); dfd_sum_batch_begin / _end;
 * dfd_bn_eval_coeffs_multi;
 * 112 = the eval / inference form of the MBConv block: dfd_pwconv_fwd_eval, dfd_dwconv_fwd_eval(_tiles),
 * dfd_se_fwd_parts;
 * 120 = MX fp8 weights (dfd_mx_*), fused window attention on bf16 MFMA (dfd_wattn_*),
 * batched coordinate MLPs (dfd_coord_mlp_*_multi, dfd_relpos_bias_*_multi), dfd_resize_crop_u8;
 * 121 = dfd_bias_grad / dfd_bias_grad_ws; 122 = dfd_gemm_bias_act;
 * 130 = dfd_tune; the bf16 depthwise entry points run on the matrix cores where the shape allows (same signatures);
 * 131 = dfd_augment_u8, dfd_gemm_plan, dfd_dw_mm_plan, dfd_pwconv_bwd_fused;
 * 132 = dfd_pw_ntd_plan (mid-size 1x1 layers on the LDS-DMA ring kernel; same entry points), tune keys 4-7;
 * 133 = dfd_attn_scores / dfd_attn_apply; 134 = dfd_act_bn_bwd_se, dfd_sum_batch_end_deferred, dfd_sum_passengers_flush / _discard;
 * 135 = dfd_tune keys 8-13 (grids of the vector-unit depthwise kernels — their default changed, so partial-row counts did — and of the
 * tiled weight gradient); immediate partial-row sums of 33..256 rows in one launch (same order, same bits);
 * 136 = Grad-CAM: dfd_gradcam_map, dfd_cam_render / dfd_cam_render_ws;
 * 137 = dfd_ema_update (exponential moving average of the weights);
 * 138 = dfd_mix_batch (Mixup / CutMix of a batch in place, with its soft targets), dfd_ce_loss_soft (cross entropy with
 * probability targets);
 * 139 = dfd_augment_policy_u8 (RandAugment / TrivialAugmentWide behind rotation and ColorJitter, in dfd_augment_u8's launch shape);
 * 140 = dfd_grad_sumsq, dfd_grad_clip_finish, dfd_adamw_step_clip (gradient clipping by global norm or by value in the AdamW step);
 * 141 = the one-kernel depthwise backward export of 120 (3x3 stride 1, data and weight gradient together) removed;
 * 142 = dfd_jpeg_u8, dfd_jpeg_ws (JPEG-compression augmentation: the pixels of a baseline JPEG round trip, byte-exact with Pillow);
 * 143 = dfd_tune keeps keys 0, 4 and 8-11; keys 1-3, 5-7, 12 and 13 (A/B-only sizes and the timing-only ablation mask) are DFD_EINVAL;
 * 144 = dfd_blur_u8 (Gaussian-blur augmentation: Pillow's three box passes along x and three along y, byte-exact);
 * 145 = dfd_softmax_argmax returns index 0 for a row that holds a NaN or an infinity (it returned 0x7fffffff), dfd_ce_loss with
 * label_smoothing 0 keeps a finite loss beside a -inf logit off the target (it returned NaN); finite inputs give the same bits;
 * 146 = dfd_roc_curve / dfd_roc_ws, dfd_roc_sweep, dfd_confusion (exact ROC curve, rank statistic, threshold sweep and confusion matrix);
 * 147 = dfd_ce_loss_w (cross entropy with per-class weights and the focal modulating factor, index or probability targets);
 * 148 = dfd_bgemm_plan, dfd_attn_softmax_plan (which kernel dfd_bgemm runs, and the rows per workgroup and threads per (head, row)
 * of dfd_attn_softmax_fwd / _bwd: host-side queries for the tests that name a tier; no kernel changed);
 * 149 = dfd_rowtable_grad_plan (the window splits, windows per split and row lanes of dfd_rowtable_grad: host-side query; no kernel
 * changed);
 * 150 = dfd_calib_bins / _ws, dfd_calib_nll / _ws, dfd_calib_plan, dfd_softmax_argmax_t (reliability bins, Brier sum, NLL of
 * temperature-scaled logits with two derivatives, softmax / arg max at a temperature); dfd_softmax_argmax itself is unchanged;
 * 151 = dfd_fuse_scores, dfd_fuse_nll / _ws, dfd_fuse_agree, dfd_fuse_plan (the ensemble of K models: fused scores of a logit or a
 * probability pool, the pool's NLL with gradient and Hessian in its coefficients, right / wrong agreement tables);
 * 152 = dfd_stem_bwd_fused / _ok (the stem's weight gradient straight from the incoming gradient, without a stored dz; same bits as
 * dfd_act_bn_bwd + dfd_stem_conv_wgrad); dfd_act_bn_bwd takes dz = NULL: the partial sums only;
 * 153 = dfd_boot_stats, dfd_boot_counts, dfd_boot_plan, dfd_boot_ws (bootstrap resamples of the ROC statistics: Philox draws into
 * integer counts, weighted sweeps of the sorted scores; all outputs integers);
 * 154 = dfd_group_pool, dfd_group_plan, dfd_group_ws (the rows of a group, such as the frames of a video, pooled into one row: exact
 * integer sums), dfd_boot_stats_grouped, dfd_boot_plan_grouped, dfd_boot_ws_grouped (the cluster bootstrap: a resample draws whole
 * groups); dfd_boot_stats itself is unchanged. */
int dfd_version(void);

/* Planner knobs: the tier switches and grid sizes by which tests and per-layer scripts reach a kernel tier.  Process-wide plain ints:
 * set them before the first launch — they are not synchronised with concurrent callers.  Any other key: DFD_EINVAL.  (Keys 1-3, 5-7,
 * 12 and 13 of ABI 130-142 were A/B knobs; each was swept once and its winner is now a named constant at its point of use.)
 *   0 DFD_TUNE_DW_MFMA    bit 0: the depthwise forward runs on the matrix cores (bf16, C % 16 == 0) for the shapes where that form
 *                         measured faster (5x5 stride 1 on maps of at most 64 pixels); bit 3: for every shape it can serve
 *                         (tests, A/B runs); 0 = the vector-unit kernels everywhere                          (default 1)
 *   4 DFD_TUNE_PW_NTD     bit 0: dfd_pwconv_fwd runs bf16 layers of 1 k .. 64 k rows on the LDS-DMA ring kernel (dfd_pw_ntd_plan
 *                         tells which); 0 = the register-staged tile kernel everywhere (A/B runs)             (default 1)
 *   8 / 9 / 10            workgroups a vector-unit depthwise launch aims for (all channel chunks together): forward / data gradient /
 *                         weight gradient.  1024 = what is co-resident at four per CU: every workgroup starts at once and walks
 *                         its work items, nobody queues behind a first round (measured against 768 / 1536 / 2048 / 3072 per
 *                         EfficientNet-B0 layer, scripts/dw_ab.py; 2048 was the value of rounds 2-4: B0 12.94 -> 12.75,
 *                         EfficientFormerV2-S1 17.00 -> 16.65 ms per step)                                    (default 1024)
 *   11                    fewest work slots per channel chunk of those launches                             (default 32) */
int dfd_tune(int key, int value);

/* Batched final summation of weight gradients.  The weight-gradient entry points whose result goes straight to the
 * optimizer (dfd_pwconv_wgrad, dfd_dwconv_bwd_weight, dfd_stem_conv_wgrad) end with a fixed-order sum of their workspace's
 * partial rows into dw.  (dfd_conv_wgrad, dfd_rowtable_grad and dfd_sum_rows always sum at once: their callers' next
 * launch reads the result.)  Between dfd_sum_batch_begin() and dfd_sum_batch_end() ON THE CALLING HOST THREAD these sums are
 * recorded instead of launched, and _end() (or the ninth recorded sum) adds them all up with one pair of launches —
 * same order, same bits.  Contract while a batch is open: each call gets its OWN workspace, which must stay untouched
 * until _end(); dw is valid only after _end(); all calls use one stream.  The state is thread-local: other threads are
 * unaffected (the ABI stays re-entrant).  begin inside an open batch / end without one: DFD_EINVAL.                   */
int dfd_sum_batch_begin(void);
int dfd_sum_batch_end(void);
/* dfd_sum_batch_end_deferred(): closes the batch like _end() but launches nothing — the two stages of the recorded sums ride along as
 * extra workgroups of the next two dfd_act_bn_bwd / dfd_act_bn_bwd_se launches on their stream (one per network block; the sums are read by
 * the optimizer only, so they need not sit on the backward pass's dependency chain), and dfd_sum_passengers_flush(stream) launches whatever
 * is still waiting.  Contract on top of _end()'s: the workspaces stay untouched, and dw is valid, only after the SECOND carrying launch
 * or the flush — callers keep three generations of workspaces and flush at the end of the backward pass (kernels.sum_batch).  A batch that
 * finds the previous one still waiting launches that one at once.  Process-wide state keyed by the stream.  A carrying call that
 * returns an error carries nothing: the waiting batches stay as they were.                                                              */
int dfd_sum_batch_end_deferred(void);
int dfd_sum_passengers_flush(dfd_stream stream);
/* drops every waiting batch without launching it (a new backward pass calls it before anything carries: after a pass that ended in an
 * exception the waiting jobs point at memory the next pass may no longer own) */
int dfd_sum_passengers_discard(void);

/* ---------------------------------------------------------------- BatchNorm ---
 * F.batch_norm inside every conv-bn(-act) triple of the reference's modules
 * (efficientnet_pytorch MBConvBlock._bn0/_bn1/_bn2; timm BatchNormAct2d).      */

/* training mode: partial (sum, sumsq) slabs [nparts][2][C] -> bnstate, running stats */
int dfd_bn_finalize(const float* partials, int nparts, int C, double count,
                    const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* bnstate, dfd_stream stream);
/* eval mode: running stats -> bnstate */
int dfd_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int C, float* bnstate,
                       dfd_stream stream);
/* The same for every BatchNorm of a network at once (eval / inference forward: 49 launches of EfficientNet-B0 become 2).
 * jobs: host array, copied into kernel arguments; all pointers are device pointers, bnstate float[4][C] each.        */
typedef struct {
    const float *gamma, *beta, *conv_bias, *ls, *running_mean, *running_var;   /* gamma .. ls may be NULL */
    float* bnstate;
    float eps;
    int C;
} dfd_bn_eval_job;
int dfd_bn_eval_coeffs_multi(const dfd_bn_eval_job* jobs, int njobs, dfd_stream stream);
/* backward: partial (sum g, sum g*xhat) slabs -> dgamma, dbeta, coef.  train==0:
 * statistics were constants (eval-mode BN), so dy = gamma*rstd*g.               */
int dfd_bn_bwd_finalize(const float* partials, int nparts, int C, double count,
                        const float* gamma, const float* bnstate, int train,
                        float* dgamma, float* dbeta, int accumulate, float* coef,
                        dfd_stream stream);

/* The same three with the two per-channel vectors timm's ConvNorm / LayerScale2d add around a BatchNorm
 * (timm efficientformer_v2.py ConvNorm: conv(bias=True) -> BatchNorm2d; LayerScale2d: x * gamma):
 *   conv_bias [C] (optional): bias of the producing convolution.  It never enters the conv kernels: under
 *     batch statistics it cancels, so it only shifts the running mean (training) / the mean used (eval);
 *   ls_gamma  [C] (optional): LayerScale applied to the BatchNorm output, folded into (scale, shift).
 * Backward: partial sums are of dz = d loss / d (ls * BN(y)); dls / dbias are optional outputs.      */
int dfd_bn_finalize_ex(const float* partials, int nparts, int C, double count, const float* gamma,
                       const float* beta, const float* conv_bias, const float* ls_gamma,
                       float* running_mean, float* running_var, float momentum, float eps,
                       float* bnstate, dfd_stream stream);
int dfd_bn_eval_coeffs_ex(const float* gamma, const float* beta, const float* conv_bias,
                          const float* ls_gamma, const float* running_mean, const float* running_var,
                          float eps, int C, float* bnstate, dfd_stream stream);
int dfd_bn_bwd_finalize_ex(const float* partials, int nparts, int C, double count, const float* gamma,
                           const float* beta, const float* ls_gamma, const float* bnstate, int train,
                           float* dgamma, float* dbeta, float* dls, float* dbias, int accumulate,
                           float* coef, dfd_stream stream);

/* out = act(scale*y + shift) [* row_scale[n]] [+ residual]; all [N][HW][C].     */
int dfd_bn_act_apply(int dtype, const void* y, const float* bnstate, int act,
                     const void* residual, const float* row_scale, void* out,
                     int N, int HW, int C, dfd_stream stream);
/* partial sums of (g*rs, g*rs*xhat) per channel, xhat = (y-mean)*rstd            */
int dfd_bn_bwd_reduce(int dtype, const void* g, const void* y, const float* bnstate,
                      const float* row_scale, int N, int HW, int C,
                      float* partials, int pcap, int* nparts, dfd_stream stream);
/* Linear layer without statistics in ONE kernel (bf16, many rows, K % 64 == 0: csrc/dfd_gemm.hip; else DFD_EUNSUPPORTED and the
 * caller runs dfd_pwconv_fwd + dfd_bn_act_apply):  out = act(scale[n] * y + shift[n]) [* row_scale[row / HW]] [+ residual] with
 * y = bf16(a w^T) — the same arithmetic on the same rounded y as the two-kernel form, identical bits.  state: float[>=2][N]
 * (dfd_bn_eval_coeffs*: scale, shift = LayerScale and bias folded); act: DFD_ACT_NONE / DFD_ACT_GELU; yraw (optional, [M][N])
 * also receives y itself.  ABI 122.                                                                                          */
int dfd_gemm_bias_act(int dtype, const void* a, const void* w_nk, int M, int K, int N, const float* state, int act,
                      const void* residual, const float* row_scale, int HW, void* yraw, void* out, dfd_stream stream);
/* Rows per tile (256 or 128) with which the LDS-DMA product kernel (csrc/dfd_gemm.hip) serves a plain bf16 [M][K] x [N][K]^T
 * through dfd_pwconv_fwd / dfd_gemm_bias_act, 0 when the shape stays with the 128 x 128 kernel of dfd_pwconv.hip. */
int dfd_gemm_plan(int M, int K, int N);
/* Column-tile width (64 / 96 / 128 / 192) with which the LDS-DMA ring kernel serves a bf16 dfd_pwconv_fwd of this shape; 0: the
 * shape stays with the register-staged kernels (the prologue / epilogue combination can still decline at launch).            */
int dfd_pw_ntd_plan(int M, int K, int Nout);
/* dbias[c] (+)= sum over rows of g[row][c] (* row_scale[n]): the bias gradient of a Linear layer (no statistics).  ws:
 * dfd_bias_grad_ws bytes; its final fixed-order summation joins an open dfd_sum_batch like a weight gradient's.  ABI 121 */
size_t dfd_bias_grad_ws(int N, int HW, int C);
int dfd_bias_grad(int dtype, const void* g, const float* row_scale, int N, int HW, int C, float* dbias, int accumulate,
                  float* ws, size_t ws_bytes, dfd_stream stream);
/* dz = (D*gate[n,c] + dpool[n,c]/HW) * act'(scale*y+shift); writes dz and the partial
 * sums (dz, dz*xhat).  D, gate, dpool are each optional (NULL): D==NULL means the
 * incoming gradient is dpool/HW only (global-average-pool backward).  dz == NULL
 * (ABI 152): the same partial sums, dz is not written.                           */
int dfd_act_bn_bwd(int dtype, const void* D, const void* y, const float* gate,
                   const float* dpool, const float* bnstate, int act, void* dz,
                   int N, int HW, int C, float* partials, int pcap, int* nparts,
                   dfd_stream stream);
/* dfd_act_bn_bwd with the squeeze-excite FC weight gradients of the same block riding along as extra workgroups of the launch:
 * dw1[R][C] = sum_n dh[n][r] pooled[n][c], db1, dw2[C][R] = sum_n g[n][c] h[n][r], db2, from dfd_se_bwd's workspace se_ws
 * (= [g: N x C | dh: N x R | h: N x R]) — what dfd_se_bwd's third launch computes when it is given dw1 / dw2 (pass NULL there).
 * Only AdamW reads these gradients, so they need not be a launch of their own on the block's dependency chain; same summation
 * order, same bits.  The workspace must stay untouched between dfd_se_bwd and this call (both on `stream`).                     */
int dfd_act_bn_bwd_se(int dtype, const void* D, const void* y, const float* gate, const float* dpool,
                      const float* bnstate, int act, void* dz, int N, int HW, int C, float* partials, int pcap,
                      int* nparts, const float* se_pooled, const float* se_ws, int R, float* dw1, float* db1, float* dw2,
                      float* db2, int accumulate, dfd_stream stream);
/* pooled[n,c] = mean_hw act(scale*y+shift): SE squeeze and the classifier's
 * global average pool.
 * ws (optional, may be NULL): dfd_pool_ws() bytes of scratch; lets the library split large
 * images over several workgroups (partial vectors, summed in a fixed order by a second
 * small kernel).  No initial contents required.                                          */
size_t dfd_pool_ws(int dtype, int N, int HW, int C);
int dfd_pool_act(int dtype, const void* y, const float* bnstate, int act, float* pooled,
                 int N, int HW, int C, void* ws, size_t ws_bytes, dfd_stream stream);
/* dgate[n,c] = sum_hw D * act(scale*y+shift)                                      */
int dfd_pool_bwd_reduce(int dtype, const void* D, const void* y, const float* bnstate,
                        int act, float* dgate, int N, int HW, int C, void* ws, size_t ws_bytes,
                        dfd_stream stream);
/* out = x * row_scale[n] (drop-connect on the gradient side)                      */
int dfd_scale_rows(int dtype, const void* x, const float* row_scale, void* out,
                   int N, int HW, int C, dfd_stream stream);

/* ------------------------------------------------------------ squeeze-excite ---
 * MBConvBlock._se_reduce/_se_expand (efficientnet_pytorch), SqueezeExcite (timm):
 * gate = sigmoid(W2 * act(W1*pooled + b1) + b2).                                 */
/* w2 is torch's [C][R]; w2t [R][C] is written by the forward (coalesced reads) and is
 * what the backward takes.  w2 == NULL: w2t was prepared by the caller (dfd_prep_weights_multi). */
int dfd_se_fc_fwd(const float* pooled, const float* w1, const float* b1, const float* w2,
                  const float* b2, int N, int C, int R, int act, float* hpre, float* gate,
                  float* w2t, dfd_stream stream);
/* ws: float[N*C + 2*N*R] scratch; R <= 128, C <= 4096 */
int dfd_se_fc_bwd(const float* dgate, const float* gate, const float* hpre,
                  const float* pooled, const float* w1, const float* w2t,
                  int N, int C, int R, int act, float* dpooled,
                  float* dw1, float* db1, float* dw2, float* db2, int accumulate,
                  float* ws, dfd_stream stream);
/* The whole squeeze-excite branch behind one call each way (reference call sites: the `x * self.se(x)` step of
 * timm's InvertedResidual.forward / efficientnet_pytorch's MBConvBlock.forward, reached from
 * trainers/efficientnet.py:297 `model(x)`): pooling kernel + ONE workgroup per image that adds the pooling
 * splits and runs both FC layers (forward: 2 launches instead of 4; backward: 3 instead of 5).
 *   forward : pooled = mean_hw act_in(scale*y+shift); hpre = W1 pooled + b1; gate = sigmoid(W2 act(hpre) + b2)
 *   backward: dgate = sum_hw D*act_in(scale*y+shift) -> dpooled, dw1, db1, dw2, db2 (as dfd_se_fc_bwd)
 * pool ws / ws_bytes as for dfd_pool_act; ws (backward) as for dfd_se_fc_bwd.  C % 4 == 0.               */
int dfd_se_fwd(int dtype, const void* y, const float* bnstate, int act_in, int N, int HW, int C,
               const float* w1, const float* b1, const float* w2, const float* b2, int R, int act,
               float* pooled, float* hpre, float* gate, float* w2t, void* ws, size_t ws_bytes,
               dfd_stream stream);
int dfd_se_bwd(int dtype, const void* D, const void* y, const float* bnstate, int act_in, int N, int HW,
               int C, const float* gate, const float* hpre, const float* pooled, const float* w1,
               const float* w2t, int R, int act, float* dgate, float* dpooled, float* dw1, float* db1,
               float* dw2, float* db2, int accumulate, void* pool_ws, size_t pool_ws_bytes, float* ws,
               dfd_stream stream);

/* ----------------------------------------------------------- depthwise conv ---
 * F.conv2d(groups=C) of MBConvBlock._depthwise_conv / timm conv_dw, k in {3,5},
 * stride in {1,2}, arbitrary (asymmetric "SAME") top/left padding.               */
typedef struct {
    int N, H, W, C;        /* input  [N][H][W][C]   */
    int Ho, Wo;            /* output [N][Ho][Wo][C] */
    int k, stride, pad_top, pad_left;
} dfd_dwconv_shape;

/* y = dwconv(act(scale*x+shift)) (in_bnstate==NULL: x used as is); optional stats */
int dfd_dwconv_fwd(int dtype, const void* x, const float* in_bnstate, int in_act,
                   const float* w, void* y, const dfd_dwconv_shape* s,
                   float* partials, int pcap, int* nparts, dfd_stream stream);
/* dy = a*dz + b*y + c (coef; coef==NULL: dy = dz).  da = dwconv^T(dy).
 * xin != NULL: dzin = da * act'(scale*xin+shift) and partial sums (dzin, dzin*xhat);
 * xin == NULL: dzin = da.                                                        */
int dfd_dwconv_bwd_data(int dtype, const void* dz, const void* y, const float* coef,
                        const float* w, const void* xin, const float* in_bnstate, int in_act,
                        void* dzin, const dfd_dwconv_shape* s,
                        float* partials, int pcap, int* nparts, dfd_stream stream);
/* dw[c][kh][kw] = sum dy * act(scale*xin+shift) (in_bnstate==NULL: xin as is)      */
int dfd_dwconv_bwd_weight(int dtype, const void* dz, const void* y, const float* coef,
                          const void* xin, const float* in_bnstate, int in_act,
                          float* dw, const dfd_dwconv_shape* s, int accumulate,
                          float* ws, size_t ws_bytes, dfd_stream stream);

/* Diagnostics: the tile plan the matrix-core depthwise forward would use for a shape (pro: the staging phase applies an
 * activation): out[12] = NI, TH, TW, runs, IH, IW, row pitch, plane pixels, work items, whole-image flag, LDS bytes in / out. */
int dfd_dw_mm_plan(const dfd_dwconv_shape* s, int pro, int* out);

/* ---- eval / inference form of the MBConv block -----------------------------------------------------------------
 * With running statistics every BatchNorm is an affine map known before the layer runs, so the PRODUCER can apply
 * its own BatchNorm + activation in the epilogue and store the activated tensor (training cannot: the batch
 * statistics only exist once the whole layer has run).  Replaces, for `model.eval()` forwards without autograd
 * (reference: orchestration/orchestrator.py:127-151 `class_probabilities`, evaluate.py:238-260, the validation loop
 * trainers/efficientnet.py:333-352), the raw-output + consumer-prologue chain of the training form:
 *   dfd_pwconv_fwd_eval : out = act(scale*(a @ w^T) + shift)               (the expand 1x1 convolution + bn1 + SiLU)
 *   dfd_dwconv_fwd_eval : y = act(scale*dwconv(x) + shift), and pool_parts[tile][N][C] = per-(tile, image) channel sums
 *                         of y as stored — the squeeze-excite pooling pass disappears
 *   dfd_se_fwd_parts    : dfd_se_fwd from those sums (mean = sum over tiles / HW)
 * out_bnstate: float[>=2][C] scale, shift (dfd_bn_eval_coeffs*).  out_act: DFD_ACT_SILU (the EfficientNet blocks);
 * anything else returns DFD_EUNSUPPORTED.  Values equal the training-form chain bit for bit except the pooled mean
 * (same addends, summed tile by tile instead of split by split).
 * dfd_dwconv_fwd_eval_tiles: rows of pool_parts the call will write (0 = invalid shape); ntiles returns the same. */
int dfd_pwconv_fwd_eval(int dtype, const void* a, const void* w, const float* out_bnstate, int out_act,
                        void* out, int M, int K, int Nout, dfd_stream stream);
int dfd_dwconv_fwd_eval_tiles(int dtype, const dfd_dwconv_shape* s);
int dfd_dwconv_fwd_eval(int dtype, const void* x, const float* w, const float* out_bnstate, int out_act, void* y,
                        const dfd_dwconv_shape* s, float* pool_parts, int* ntiles, dfd_stream stream);
int dfd_se_fwd_parts(const float* parts, int splits, int N, int HW, int C, const float* w1, const float* b1,
                     const float* w2, const float* b2, int R, int act, float* pooled, float* hpre, float* gate,
                     float* w2t, dfd_stream stream);
size_t dfd_dwconv_bwd_weight_ws(const dfd_dwconv_shape* s);

/* ----------------------------------------------------------- pointwise conv ---
 * 1x1 convolutions (_expand_conv, _project_conv, _conv_head; timm conv_pw/conv_pwl/
 * conv_head) as MFMA GEMMs over the NHWC row matrix, with the producer's BN + act
 * (+ SE gate) applied to the A operand on the way in.                            */
#define DFD_PRO_NONE        0   /* a                                              */
#define DFD_PRO_BN_ACT      1   /* act(scale[k]*a + shift[k])                     */
#define DFD_PRO_BN_ACT_GATE 2   /* act(scale[k]*a + shift[k]) * gate[row/HW][k]   */
#define DFD_PRO_AFFINE2     3   /* ca[k]*a + cb[k]*a2 + cc[k]                     */
typedef struct {
    int mode;
    int act;
    int HW;                 /* rows per image (gate lookup) */
    int _pad;
    const void* a2;         /* AFFINE2: second operand, same shape/dtype as a */
    const float* coef;      /* BN_ACT*: bnstate [4][K]; AFFINE2: coef [3][K]  */
    const float* gate;      /* BN_ACT_GATE: [N][K] */
} dfd_prologue;

/* out[M][Nout] = P(a)[M][K] * w[Nout][K]^T (+ residual); w in `dtype`.
 * partials != NULL: (sum, sumsq) per output channel of the rounded output.       */
int dfd_pwconv_fwd(int dtype, const void* a, const dfd_prologue* pro, const void* w,
                   void* out, const void* residual, int M, int K, int Nout,
                   float* partials, int pcap, int* nparts, dfd_stream stream);
/* dw[Ni][Nj] = sum_m P(p)[m][i] * Q(q)[m][j]                                       */
int dfd_pwconv_wgrad(int dtype, const void* p, const dfd_prologue* pro_p, int Ni,
                     const void* q, const dfd_prologue* pro_q, int Nj, int M,
                     float* dw, int accumulate, float* ws, size_t ws_bytes,
                     dfd_stream stream);
/* The EXPAND 1x1 layer's backward in one pass over its widest operands (MBConvBlock._expand_conv / timm conv_pw):
 *   d = coef[0]*dz + coef[1]*y + coef[2]  (the BN-backward map, as the AFFINE2 prologue),  dx = d * w (+ residual),  dw = d^T * x.
 * dz, y [M][Cm]; x [M][Cin]; w_kn = the layer's weight in the activation dtype as [Cin][Cm] (the [K][N] copy dfd_pw_prep_weights /
 * dfd_prep_weights_multi write); residual [M][Cin] or NULL; dx [M][Cin]; dw f32 [Cm][Cin]; ws as for dfd_pwconv_wgrad(M, Cm, Cin).
 * Bit-identical to dfd_pwconv_fwd(dz, AFFINE2, w_kn, residual) + dfd_pwconv_wgrad(dz, AFFINE2, x) — (dz, y) cross HBM once
 * instead of twice.  bf16, Cin <= 32, Cm <= 128 or Cm = 144, M >= 196,608 (EfficientNet blocks 1-3 at the benchmark batch); anything else:
 * DFD_EUNSUPPORTED, the caller runs the two entry points. */
int dfd_pwconv_bwd_fused(int dtype, const void* dz, const void* y, const float* coef, const void* x, const void* w_kn,
                         const void* residual, int M, int Cm, int Cin, void* dx, float* dw, int accumulate, float* ws,
                         size_t ws_bytes, dfd_stream stream);
size_t dfd_pwconv_wgrad_ws(int M, int Ni, int Nj);
/* f32 master [N][K] -> w_nk [N][K] and w_kn [K][N] in `dtype` (either may be NULL) */
int dfd_pw_prep_weights(int dtype, const float* w, void* w_nk, void* w_kn, int N, int K,
                        dfd_stream stream);
/* Every derived weight of a network in one call (launched 32 jobs at a time): src f32 [N][K] -> nk ([N][K],
 * element type `dtype`) and / or kn ([K][N]); either destination may be NULL.  Also used for the [R][C] copy
 * of the squeeze-excite expand weight (dtype DFD_F32, kn only).  `jobs` is a HOST array.                   */
typedef struct dfd_prep_job {
    const float* src;
    void* nk;
    void* kn;
    int N, K;
    int dtype;
    int _pad;
} dfd_prep_job;
int dfd_prep_weights_multi(const dfd_prep_job* jobs, int njobs, dfd_stream stream);

/* ------------------------------------------------------------------- stem ---
 * _conv_stem / conv_stem: k x k stride-2 convolution on the 3-channel f32 image.  */
typedef struct {
    int N, H, W, Cout, Ho, Wo, k, stride, pad_top, pad_left;
} dfd_stem_shape;
int dfd_stem_conv_fwd(int dtype, const float* x, const float* w, void* y,
                      const dfd_stem_shape* s, float* partials, int pcap, int* nparts,
                      dfd_stream stream);
int dfd_stem_conv_wgrad(int dtype, const float* x, const void* dz, const void* y,
                        const float* coef, float* dw, const dfd_stem_shape* s,
                        int accumulate, float* ws, size_t ws_bytes, dfd_stream stream);
size_t dfd_stem_conv_wgrad_ws(const dfd_stem_shape* s);
/* The stem's weight gradient straight from g (ABI 152; bf16, Cout 16 or 32, the shapes of dfd_stem_conv_wgrad's matrix-core kernel:
 * dfd_stem_bwd_fused_ok says 1; everything else: DFD_EUNSUPPORTED, nothing launched).  g = d loss / d act(BN(y)), y the raw convolution
 * output, bnstate the forward's (scale, shift, mean, rstd), coef the (a, b, c) of dfd_bn_bwd_finalize_ex.  The kernel recomputes
 * dz = act'(scale y + shift) g as dfd_act_bn_bwd (D = g, no gate, no dpool) rounds and stores it, and applies a dz + b y + c as
 * dfd_stem_conv_wgrad does: dw has the bits of that pair of calls, and the dz tensor does not exist.  The sums for coef come from
 * dfd_act_bn_bwd with dz = NULL (ABI 152: the sums only, same partial rows).  ws: dfd_stem_conv_wgrad_ws bytes; the final
 * summation joins an open dfd_sum_batch like dfd_stem_conv_wgrad's.  max_rows > 0 caps the grid (tests; another summation order). */
int dfd_stem_bwd_fused_ok(int dtype, const dfd_stem_shape* s, const float* x);
int dfd_stem_bwd_fused(int dtype, const float* x, const void* g, const void* y, const float* bnstate, int act,
                       const float* coef, float* dw, const dfd_stem_shape* s, int accumulate, float* ws,
                       size_t ws_bytes, int max_rows, dfd_stream stream);

/* ------------------------------------------------- classifier, loss, optimizer --- */
/* out = u >= p ? x/(1-p) : 0   (forward and, with x = grad, backward)              */
int dfd_dropout(const float* x, const float* u, float p, float* out, int n, dfd_stream stream);
int dfd_linear_fwd(const float* x, const float* w, const float* b, float* out,
                   int N, int K, int J, dfd_stream stream);
int dfd_linear_bwd(const float* dout, const float* x, const float* w, float* dx,
                   float* dw, float* db, int N, int K, int J, int accumulate,
                   dfd_stream stream);
/* nn.CrossEntropyLoss(label_smoothing) mean-reduced; dlogits (optional) is
 * d(loss*grad_scale)/dlogits.  With label_smoothing 0 a -inf logit off the target
 * leaves the loss finite and has gradient 0, as in torch.  Targets are not range-checked. */
int dfd_ce_loss(const float* logits, const int64_t* targets, int N, int J,
                float label_smoothing, float grad_scale, float* row_loss, float* loss,
                float* dlogits, dfd_stream stream);
/* The same with probability targets, f32 [N][J] (torch's cross_entropy with a floating target): q = targets * (1 - ls) + ls / J,
 * row_loss[n] = -sum_j q[n][j] * logp[n][j], loss = mean, dlogits = (softmax * sum_j q[n][j] - q) * grad_scale / N.  The rows
 * of `targets` need not sum to one.                                                  */
int dfd_ce_loss_soft(const float* logits, const float* targets, int N, int J,
                     float label_smoothing, float grad_scale, float* row_loss, float* loss,
                     float* dlogits, dfd_stream stream);
/* Class-weighted and focal cross entropy (ABI 147).  targets: int64 [N] class indices (soft = 0) or f32 [N][J] probabilities
 * (soft != 0).  With p = softmax(logits) per row, ls = label_smoothing in [0, 1), gamma = focal_gamma >= 0 and w = class_weight
 * (f32 [J]; NULL: all ones):
 *   q[n][j]     = (1 - ls) * (j == targets[n]) + ls / J      (indices)     or     targets[n][j] * (1 - ls) + ls / J
 *   row_loss[n] = -sum_j w[j] * q[n][j] * (1 - p[n][j])^gamma * logp[n][j]   ((1 - p)^0 = 1 also at p = 1)
 *   loss        = sum_n row_loss[n] / D,   D = sum_n w[targets[n]] for indices, N for probabilities
 * which are the rules of torch's cross_entropy(weight=, label_smoothing=, reduction="mean"): with gamma 0 the loss is torch's.
 * At D = 0 (every target names a class of weight 0) the loss is NaN, as torch's is, whatever the rows sum to.  A term whose q is 0 is 0 whatever its logit is (a -inf logit off the target with ls = 0 keeps the loss
 * finite and has gradient 0).  dlogits (optional) = grad_scale / D * (g[n][k] - p[n][k] * sum_j g[n][j]) with
 *   g[n][j] = w[j] * q[n][j] * (gamma * (1 - p)^(gamma - 1) * p * logp - (1 - p)^gamma),   the bracket 0 at p = 1 for gamma > 0.
 * denom: one float of device scratch the caller owns (D of the weighted index case is summed there first, in a fixed order;
 * its content afterwards is unspecified).  No atomics: equal inputs give equal bits.  Two launches, three with indices and
 * weights.  NULL logits / targets / denom / row_loss / loss, N < 1, J < 1, gamma < 0 or not finite, ls outside [0, 1):
 * DFD_EINVAL, nothing is launched.  Index targets are not range-checked (one outside [0, J) matches no class). */
int dfd_ce_loss_w(const float* logits, const void* targets, int soft, int N, int J,
                  float label_smoothing, float focal_gamma, const float* class_weight,
                  float grad_scale, float* denom, float* row_loss, float* loss,
                  float* dlogits, dfd_stream stream);
/* probs (optional) = softmax(logits) per row, preds = its arg max, the lowest index on ties.  A row that holds a NaN or an
 * infinity has NaN probabilities and preds 0 (torch.argmax(torch.softmax(row))): preds is always an index into the row. */
int dfd_softmax_argmax(const float* logits, int N, int J, float* probs, int64_t* preds,
                       dfd_stream stream);
/* Resize + CenterCrop / RandomResizedCrop of decoded uint8 RGB images on the device, bit-exact with Pillow's bilinear
 * Image.resize (two passes, 8-bit intermediate, anti-aliased when shrinking) — trainers/efficientnet.py:111-234,
 * orchestrator.py:316-347.  src: the batch's images, tightly packed HWC, one after the other in one buffer.  Per image:
 * out = window (cx, cy, OW x OH) of  crop(bx, by, bw, bh).resize((rw, rh)); pixels outside the resized image are 0.
 * jobs_dev: DEVICE array of N descriptors.  max_shrink: ceil of the largest bw/rw, bh/rh of the batch (<= 46).        */
typedef struct dfd_resize_job {
    long offset;            /* byte offset of the image in src                                  */
    int H, W;               /* source size                                                       */
    int bx, by, bw, bh;     /* box of the source that is resized                                 */
    int rw, rh;             /* size it is resized to                                             */
    int cx, cy;             /* origin of the output window in the resized image (may be < 0)    */
    int _pad[2];
} dfd_resize_job;
int dfd_resize_crop_u8(const unsigned char* src, const dfd_resize_job* jobs_dev, unsigned char* dst, int N, int OH, int OW,
                       int max_shrink, dfd_stream stream);
/* RandomRotation + ColorJitter on the device for a uint8 [N][H][W][3] batch (between dfd_resize_crop_u8 and dfd_image_prep): the
 * reference's DEFAULT 224-pixel training pipeline has both (trainers/efficientnet.py:173-181).  Byte-exact with the PIL pipeline of
 * deepfakedetection_amd/data.py (csrc/dfd_augment.hip restates Pillow's rotate / blend / HSV arithmetic; oracle/image_ref.py).
 * One job per picture, drawn by the host with the same distributions as the CPU transforms:
 *   mode   0 copy, 1 affine rotation with the 16.16 coefficients a[6] (data.rotate_plan), 2 / 3 / 4 rotation by 180 / 90 / 270 degrees
 *          (the last two for square pictures only);
 *   order  the permutation of (0 brightness, 1 contrast, 2 saturation, 3 hue) ColorJitter drew; enable bit k: operation k runs;
 *   fb, fc, fs the three blend factors; dh the hue shift in 8-bit hue units (0..255).
 * src != dst.  DFD_EUNSUPPORTED when H * W * 3 exceeds 156 KiB (the picture stays in one CU's LDS): callers keep the PIL pipeline. */
typedef struct {
    int mode;
    int a[6];
    int order[4];
    float fb, fc, fs;
    int dh;
    int enable;
} dfd_augment_job;   /* 64 bytes */
int dfd_augment_u8(const unsigned char* src, const dfd_augment_job* jobs_dev, unsigned char* dst, int N, int H, int W,
                   dfd_stream stream);
/* The automatic augmentation policies RandAugment / TrivialAugmentWide (torchvision transforms/autoaugment.py; data.RandAugment,
 * data.TrivialAugmentWide are their PIL form) behind rotation and ColorJitter, in the same launch and over the same LDS-resident
 * picture, byte-exact with Pillow.  A job is a dfd_augment_job followed by
 *   flip   != 0: RandomHorizontalFlip, applied where the PIL pipeline applies it, after the rotation and before ColorJitter (it does
 *          not commute with the geometric operations below, so with a policy on dfd_image_prep gets no flip);
 *   nops   how many of ops[] run, in order (0..DFD_AUG_MAX_OPS);
 *   ops[]  op: a DFD_AUG_* code.  ShearX/Y, TranslateX/Y, Rotate: ip = gather mode as dfd_augment_job.mode (0 = leave alone) and a[6] its
 *          16.16 coefficients (data.shear_plan / translate_plan / rotate_plan).  Brightness, Color, Contrast, Sharpness: fp = the
 *          ImageEnhance factor.  Posterize: ip = the byte mask.  Solarize: fp = the threshold (v >= fp becomes 255 - v).
 * The jobs are validated on the host before the launch, so they are passed in host memory (`jobs_host`) as well as on the device
 * (`jobs_dev`, the same N records; its copy may still be in flight on `stream`): DFD_EINVAL for nops outside 0..DFD_AUG_MAX_OPS, an
 * unknown operation or gather mode, or a 90 / 270-degree transpose mode on a picture that is not square; DFD_EUNSUPPORTED as above. */
#define DFD_AUG_MAX_OPS 4
#define DFD_AUG_IDENTITY     0
#define DFD_AUG_SHEAR_X      1
#define DFD_AUG_SHEAR_Y      2
#define DFD_AUG_TRANSLATE_X  3
#define DFD_AUG_TRANSLATE_Y  4
#define DFD_AUG_ROTATE       5
#define DFD_AUG_BRIGHTNESS   6
#define DFD_AUG_COLOR        7
#define DFD_AUG_CONTRAST     8
#define DFD_AUG_SHARPNESS    9
#define DFD_AUG_POSTERIZE    10
#define DFD_AUG_SOLARIZE     11
#define DFD_AUG_AUTOCONTRAST 12
#define DFD_AUG_EQUALIZE     13
#define DFD_AUG_NUM_OPS      14
typedef struct {
    int op;
    int ip;
    float fp;
    int a[6];
} dfd_augment_op;           /* 36 bytes */
typedef struct {
    dfd_augment_job base;
    int flip;
    int nops;
    dfd_augment_op ops[DFD_AUG_MAX_OPS];
} dfd_augment_policy_job;   /* 216 bytes */
int dfd_augment_policy_u8(const unsigned char* src, const dfd_augment_policy_job* jobs_host, const dfd_augment_policy_job* jobs_dev,
                          unsigned char* dst, int N, int H, int W, dfd_stream stream);
/* JPEG-compression augmentation (data.RandomJpeg is its PIL form): picture n of the uint8 [N][H][W][3] batch `src` becomes in `out` what
 * Image.save(buf, "JPEG", quality=q) followed by Image.open(buf) makes of it, byte for byte — 4:2:0 chroma, the Annex K tables
 * with baseline clamping, libjpeg's integer DCT both ways and its triangle chroma upsampling, without the lossless entropy coding
 * (csrc/dfd_jpeg.hip; tests/_jpeg_ref.py restates it in numpy).  jobs_dev: DEVICE int32 [N][2] = {quality, flip}: quality 0 copies the
 * picture through, 1..100 compress; flip != 0 reads the picture mirrored in x BEFORE it is compressed or copied (RandomHorizontalFlip
 * in front of the round trip, with which it does not commute).  ws: dfd_jpeg_ws(N, H, W) bytes of scratch (the reconstructed Y
 * plane and the two half-size chroma planes, about 1.5 bytes per pixel), no initial contents required.  src != out; any H, any
 * W >= 5 (libjpeg upsamples a chroma plane of width 1 or 2 differently): DFD_EINVAL otherwise, and for a NULL pointer.  Two launches. */
int dfd_jpeg_u8(const unsigned char* src, const int* jobs_dev, void* ws, unsigned char* out, int N, int H, int W, dfd_stream stream);
size_t dfd_jpeg_ws(int N, int H, int W);
/* Gaussian-blur augmentation (data.RandomBlur is its PIL form): picture n of the uint8 [N][H][W][3] batch `src` becomes in `out` what
 * Image.filter(ImageFilter.GaussianBlur(radius=sigma)) makes of it, byte for byte: three extended box blurs along x, then three along
 * y, each pass out[x] = (ww * sum_{|d| <= r} in[x + d] + fw * (in[x - r - 1] + in[x + r + 1]) + 2^23) >> 24 on replicated edges,
 * rounded to a byte, the three channels apart (csrc/dfd_blur.hip; tests/_blur_ref.py restates it in numpy).  jobs_dev: DEVICE int32
 * [N][4] = {r, ww, fw, 0} as data.blur_plan(sigma) gives them.  A job with ww == 0 copies its picture through, and so does one with r
 * outside 0..DFD_BLUR_MAX_RADIUS (sigma 16 has r = 15): defined behaviour, the jobs cannot be checked on the host.  The blur commutes
 * with a mirror in x, so the jobs carry no flip.  src != out; H * W <= DFD_BLUR_MAX_PIXELS (two byte planes of one channel stay in one
 * CU's LDS through all six passes): DFD_EINVAL otherwise, and for a NULL pointer or N, H or W below 1.  One launch. */
#define DFD_BLUR_MAX_RADIUS 32
#define DFD_BLUR_MAX_PIXELS (78 * 1024)
int dfd_blur_u8(const unsigned char* src, const int* jobs_dev, unsigned char* out, int N, int H, int W, dfd_stream stream);

/* Evaluation metrics on the device, exact (csrc/dfd_metrics.hip; tests/_metrics_ref.py restates them in numpy and Python integers).
 * All three are integer counting: the results do not depend on the order in which workgroups run, no workgroup waits for another
 * (dependent work is a later launch on the same stream), and the only atomics are integer adds.
 *
 * dfd_roc_curve: `score` = n f32 scores sorted ASCENDING (NaN last, as torch.sort leaves them) and `label` their int64 labels in the
 * same order; a sample is a positive when its label == `positive`, a negative otherwise.  A tie group is a maximal run with
 * score[i] == score[i + 1] under float comparison (-0.0 and +0.0 are one group, every NaN is a group of its own); the order inside a
 * group does not matter.  Outputs, with G the number of groups:
 *   thr[g]                   the score of group g (of its last member: the sign of a zero group is that member's), g < G
 *   cum_pos[g], cum_neg[g]   positives / negatives in groups 0..g inclusive; entries g >= G of the three arrays are NOT written
 *   stats[DFD_ROC_STATS_LEN] = {P, N, G, nonfinite (scores that are NaN or +-inf), two_u}
 *   two_u = sum_g p_g * (cum_neg[g - 1] + cum_neg[g]), p_g the positives of group g: twice the Mann-Whitney U with ties counted
 *   half, so AUC = two_u / (2 P N) exactly (the caller divides once).
 * ws: dfd_roc_ws(n) bytes of scratch (int32 tile totals), no initial contents required.  n == 0 is valid and leaves zeros in stats;
 * n > DFD_ROC_MAX_N (two_u stays below 2^56), a negative n or a NULL pointer: DFD_EINVAL (dfd_roc_ws: 0); a small ws: DFD_EWORKSPACE.
 * Four launches: per-tile sums (DFD_ROC_TILE scores per workgroup), one workgroup of DFD_ROC_SCAN_WIDTH threads that scans the tile
 * totals (looping when there are more tiles than threads), the tile pass that writes the compacted arrays, the pass over the groups.
 *
 * dfd_roc_sweep: for each of T <= DFD_ROC_MAX_CUTS ascending f64 cut points, tp[k] = #{positive, score >= cuts[k]} and fp[k] likewise
 * for the negatives, the comparison in f64 (the promotion numpy applies to float32 scores against a float64 cut: rounding the cut to
 * f32 moves it across scores).  One thread per cut, a binary search in thr[0..G); G, P and N are read from `stats` on the device (G
 * clamped to `cap`, the arrays' length), so no host synchronisation separates it from dfd_roc_curve.  Scores must be free of NaN.
 *
 * dfd_confusion: counts[J][J] (int64, row = truth, column = prediction) over n int64 label pairs; a pair with either label outside
 * [0, J) is left out of the matrix and counted in *oob.  Both outputs are zeroed first.  J <= DFD_CONFUSION_LDS_MAX_J: an int32
 * histogram per workgroup in LDS (J * J * 4 bytes, at most 64 KiB), flushed with 64-bit integer adds; above, up to
 * DFD_CONFUSION_MAX_J: one 64-bit integer add per sample.  J outside 1..DFD_CONFUSION_MAX_J, n < 0 or a NULL pointer: DFD_EINVAL. */
#define DFD_ROC_TILE 2048
#define DFD_ROC_SCAN_WIDTH 1024
#define DFD_ROC_MAX_N (1 << 28)
#define DFD_ROC_MAX_CUTS 4096
#define DFD_ROC_STATS_LEN 5
#define DFD_CONFUSION_LDS_MAX_J 128
#define DFD_CONFUSION_MAX_J 1024
size_t dfd_roc_ws(int n);
int dfd_roc_curve(const float* score, const int64_t* label, int n, int64_t positive, void* ws, size_t ws_bytes, float* thr,
                  int64_t* cum_pos, int64_t* cum_neg, int64_t* stats, dfd_stream stream);
int dfd_roc_sweep(const float* thr, const int64_t* cum_pos, const int64_t* cum_neg, const int64_t* stats, int cap, const double* cuts,
                  int T, int64_t* tp, int64_t* fp, dfd_stream stream);
int dfd_confusion(const int64_t* truth, const int64_t* pred, int n, int J, int64_t* counts, int64_t* oob, dfd_stream stream);

/* Calibration of the probabilities on the device (csrc/dfd_calib.hip, ABI 150).  Rows are samples, J <= DFD_CALIB_MAX_J classes,
 * n <= DFD_CALIB_MAX_N rows.  In both reducing entry points a row that holds a NaN or an infinity is counted as `nonfinite` and
 * otherwise left out; a finite row whose target is outside [0, J) is counted as `oob` and otherwise left out; the rest are valid.
 *
 * dfd_calib_bins: `probs` f32 [n][J], `targets` int64 [n], M <= DFD_CALIB_MAX_BINS bins.  Per valid row conf = max_j probs[i][j],
 * pred = the lowest index that attains it (dfd_softmax_argmax's tie rule), bin = #{k in 1..M-1 : (double)conf > (double)k / (double)M}
 * (compared in f64, right-closed bins: conf <= 0 lands in bin 0, conf >= 1 in bin M - 1) and q = llrint((double)conf * 2^32).
 *   bins[M][3]  = {rows, rows with pred == target, sum of q} per bin (int64)
 *   stats[4]    = {valid rows, nonfinite rows, oob rows, valid rows with pred == target}
 *   *brier      = sum over valid rows of sum_j (probs[i][j] - [j == target])^2, in f64
 * An f32 conf >= 2^-9 is a multiple of 2^-32 and conf >= 1 / J, so up to J = 512 q is exact; sum q < 2^61.  The integers are
 * exact and independent of the order of the rows and of the launch geometry (integer adds only, LDS histogram per workgroup).
 * brier is a two-stage f64 sum in a fixed order: equal inputs give equal bits.  Probabilities are expected in [0, 1]; a finite
 * conf outside is binned by the rule above.  Three launches (zero, bin, sum).
 *
 * dfd_calib_nll: `logits` f32 [n][J], `targets` int64 [n], `betas` K <= DFD_CALIB_MAX_BETAS f64 values IN HOST MEMORY (they are
 * checked here and travel by value in the launch), each finite and > 0.  All arithmetic in f64; per valid row and beta, with
 * a_j = beta z_j, m = max_j a_j, s = sum_j exp(a_j - m), p_j = exp(a_j - m) / s:
 *   out[k][0] (nll) += m + log s - a_y,   out[k][1] (g = d nll / d beta) += sum_j p_j z_j - z_y,
 *   out[k][2] (h = d2 nll / d beta2) += sum_j p_j z_j^2 - (sum_j p_j z_j)^2
 *   stats[2]   = {nonfinite rows, oob rows}
 * One pass over the logits serves every beta (a row is read once and held in registers); the same two-stage fixed-order f64
 * sum: equal inputs give equal bits.  Two launches.
 *
 * ws: dfd_calib_bins_ws(n, J) / dfd_calib_nll_ws(n, J, K) bytes of scratch, 8-byte aligned, no initial contents required.
 * n == 0 is valid (zeros).  n, J, M or K outside its range, a beta that is not finite and > 0, or a NULL pointer: DFD_EINVAL
 * (the _ws queries: 0), nothing is launched; a small ws: DFD_EWORKSPACE.
 *
 * dfd_calib_plan: out[4] = {row layout (DFD_CALIB_LAYOUT_THREAD: one thread per row, J <= DFD_CALIB_THREAD_MAX_J;
 * DFD_CALIB_LAYOUT_WAVE: one wave per row with wave shuffles), rows per workgroup and trip, stage-1 workgroups (at most
 * DFD_CALIB_MAX_BLOCKS; a workgroup strides over the rest), trips of the stage-2 loop (DFD_CALIB_STAGE2_WIDTH partials per
 * trip)} of both entry points above: host code, for the tests that name a tier.
 *
 * dfd_softmax_argmax_t (csrc/dfd_misc.hip, dfd_softmax_argmax's kernel): dfd_softmax_argmax of beta * z:
 * p_j = exp((z_j - max_j z) * beta) / sum, beta = inv_temperature finite and > 0 (else DFD_EINVAL); the same rules for non-finite
 * rows and ties; at beta == 1.0f the same bits as dfd_softmax_argmax. */
#define DFD_CALIB_MAX_N (1 << 28)
#define DFD_CALIB_MAX_J 1024
#define DFD_CALIB_MAX_BINS 64
#define DFD_CALIB_MAX_BETAS 64
#define DFD_CALIB_THREAD_MAX_J 16
#define DFD_CALIB_MAX_BLOCKS 1024
#define DFD_CALIB_STAGE2_WIDTH 64
#define DFD_CALIB_LAYOUT_THREAD 0
#define DFD_CALIB_LAYOUT_WAVE 1
size_t dfd_calib_bins_ws(int n, int J);
int dfd_calib_bins(const float* probs, const int64_t* targets, int n, int J, int M, void* ws, size_t ws_bytes, int64_t* bins,
                   int64_t* stats, double* brier, dfd_stream stream);
size_t dfd_calib_nll_ws(int n, int J, int K);
int dfd_calib_nll(const float* logits, const int64_t* targets, int n, int J, const double* betas, int K, void* ws, size_t ws_bytes,
                  double* out, int64_t* stats, dfd_stream stream);
int dfd_calib_plan(int n, int J, int* out);
int dfd_softmax_argmax_t(const float* logits, int N, int J, float inv_temperature, float* probs, int64_t* preds, dfd_stream stream);

/* The ensemble of K <= DFD_FUSE_MAX_MODELS models on the device (csrc/dfd_fuse.hip, ABI 151).  Member k's logits are an f32 [n][J]
 * buffer of its own; `ptrs` is an array of K device addresses IN HOST MEMORY (they travel by value in the launch), and so are coef,
 * beta and cands.  J <= DFD_FUSE_MAX_J classes, n <= DFD_FUSE_MAX_N rows.  A row with a NaN or an infinity in any member is
 * `nonfinite`; in the reducing entry points a finite row whose target is outside [0, J) is `oob`; both are left out of the sums.
 *
 * dfd_fuse_scores: all arithmetic in f64, one rounding to f32 on store.
 *   mode DFD_FUSE_LOGIT (log-linear pool): f_j = sum_k coef[k] z_kj (k ascending), p = softmax(f); any finite coef; beta is not read.
 *   mode DFD_FUSE_PROB (linear pool): p_j = sum_k coef[k] softmax(beta[k] z_k)_j, f_j = log p_j; coef[k] >= 0, |sum coef - 1| <=
 *   1e-12 and beta[k] > 0, else DFD_EINVAL.
 *   probs f32 [n][J] = p, logits_out f32 [n][J] = f (either may be NULL), preds int64 [n] = the lowest index that attains the
 *   maximum of the STORED f32 probabilities, stats int64 [1] = nonfinite rows; such a row gets NaN in probs and logits_out and
 *   pred 0 (dfd_softmax_argmax's contract for one model).  Two launches (zero, scores).
 *
 * dfd_fuse_nll: the logit pool at C <= DFD_FUSE_MAX_CANDS coefficient vectors cands[C][K] (finite).  With T = 1 + K + K (K + 1) / 2
 * (at most DFD_FUSE_MAX_TERMS), out f64 [C][T] = {nll, g[0..K), H[0][0..K), H[1][1..K), ..., H[K-1][K-1]} summed over the valid rows:
 *   nll += m + log s - f_y,  g[k] += E_p z_k - z_ky,  H[k][l] += E_p[z_k z_l] - E_p z_k E_p z_l  (l >= k),
 * where f_j = sum_k a_k z_kj, m = max_j f_j, s = sum_j exp(f_j - m), p_j = exp(f_j - m) / s, E_p x = sum_j p_j x_j.
 *   stats int64 [2] = {nonfinite rows, oob rows}.
 * ws: dfd_fuse_nll_ws(n, J, K, C) bytes of scratch, 8-byte aligned, no initial contents required.  A two-stage f64 sum in an order
 * that (n, J, K) alone fixes: equal inputs give equal bits.  Two launches.
 *
 * dfd_fuse_agree: pred_ptrs = K int64 [n] prediction buffers, targets int64 [n].  With r_k = (pred_k == target) per valid row:
 *   pair int64 [K][K][4] = rows with (r_a, r_b) = {(1, 1), (1, 0), (0, 1), (0, 0)}, the diagonal included,
 *   hist int64 [K + 1]   = rows by the number of members that are right,
 *   stats int64 [2]      = {valid rows, rows whose target is outside [0, J)}.
 * Integer adds only: independent of the order of the rows and of the launch geometry.  Two launches (zero, count).
 *
 * dfd_fuse_plan: out[4] = {row layout (DFD_FUSE_LAYOUT_THREAD: one thread per row, K J <= DFD_FUSE_THREAD_MAX_KJ;
 * DFD_FUSE_LAYOUT_WAVE: one wave per row), rows per workgroup and trip, stage-1 workgroups (at most DFD_FUSE_MAX_BLOCKS; a
 * workgroup strides over the rest), trips of dfd_fuse_nll's stage-2 loop (DFD_FUSE_STAGE2_WIDTH partials per trip)} of
 * dfd_fuse_scores and dfd_fuse_nll: host code, for the tests that name a tier.
 *
 * n == 0 is valid (zeros; the member addresses may then be NULL).  n, J, K, C or mode outside its range, a coefficient that is
 * not finite, or a NULL pointer: DFD_EINVAL (dfd_fuse_nll_ws: 0), nothing is launched; a small ws: DFD_EWORKSPACE. */
#define DFD_FUSE_MAX_MODELS 8
#define DFD_FUSE_MAX_CANDS 8
#define DFD_FUSE_MAX_J 1024
#define DFD_FUSE_MAX_N (1 << 28)
#define DFD_FUSE_MAX_TERMS 45
#define DFD_FUSE_THREAD_MAX_KJ 16
#define DFD_FUSE_MAX_BLOCKS 1024
#define DFD_FUSE_STAGE2_WIDTH 64
#define DFD_FUSE_LAYOUT_THREAD 0
#define DFD_FUSE_LAYOUT_WAVE 1
#define DFD_FUSE_LOGIT 0
#define DFD_FUSE_PROB 1
int dfd_fuse_scores(const float* const* ptrs, int K, int n, int J, int mode, const double* coef, const double* beta, float* probs,
                    float* logits_out, int64_t* preds, int64_t* stats, dfd_stream stream);
size_t dfd_fuse_nll_ws(int n, int J, int K, int C);
int dfd_fuse_nll(const float* const* ptrs, int K, const int64_t* targets, int n, int J, const double* cands, int C, void* ws,
                 size_t ws_bytes, double* out, int64_t* stats, dfd_stream stream);
int dfd_fuse_agree(const int64_t* const* pred_ptrs, int K, const int64_t* targets, int n, int J, int64_t* pair, int64_t* hist,
                   int64_t* stats, dfd_stream stream);
int dfd_fuse_plan(int n, int J, int K, int* out);

/* The nonparametric bootstrap of the ROC statistics on the device (csrc/dfd_boot.hip, ABI 153).  B <= DFD_BOOT_MAX_REPLICATES
 * resamples of n <= DFD_BOOT_MAX_N samples, M <= DFD_BOOT_MAX_MEMBERS score vectors ("members") over the same samples.
 *
 * The resampling rule: draw t (0 <= t < n) of resample b (0 <= b < B) runs Philox4x32-10 (csrc/dfd_philox.h) with the key
 * (seed & 0xffffffff, seed >> 32) and the counter (t >> 2, b, 0, DFD_BOOT_STREAM); u = output word t & 3; the drawn sample is
 * idx = ((uint64_t)u * n) >> 32.  c_b[i] is how often sample i was drawn, i in the CALLER'S order (not the sorted one), so that
 * every member sees the same resamples.  The multiply-shift gives each index either floor(2^32 / n) or that plus one of the 2^32
 * values of u: the index probabilities differ by at most n / 2^32 relative (0.4 % at n = 2^24, 2.3e-5 at n = 10^5).
 *
 * dfd_boot_stats: score_ptrs / perm_ptrs = M device addresses each IN HOST MEMORY (they travel by value in the launch): member
 * m's n f32 scores sorted ASCENDING and the int32 permutation that sorted them (score_ptrs[m][i] is the score of sample
 * perm_ptrs[m][i]; an entry outside [0, n) counts for nothing).  is_positive uint8 [n] and hit uint8 [n] (or NULL) are in sample
 * order and shared; cuts = M doubles in host memory (NULL or a NaN: no cut).  Scores must be finite.  Every sample i counts
 * c_b[i] times:
 *   stats int64 [M][B][DFD_BOOT_STATS_LEN] = {P, N, two_u, tp, fp, hits, f0, t0, f1, t1}
 *   P, N    weighted positives (is_positive != 0) / negatives; two_u as dfd_roc_curve defines it over the tie groups of the scores
 *   tp, fp  positives / negatives with (double)score >= cut, 0 without a cut; hits = sum c_b[i] * (hit[i] != 0), 0 without hit
 *   f0, t0, f1, t1  (fps, tps) at the two ends of the segment of the resample's ROC curve (thresholds descending) on which the
 *           equal error rate is interpolated: the segment ends at the first tie-group end where fps P + tps N - P N >= 0 and starts
 *           at the group end before it, or at (0, 0); all four are 0 when P == 0 or N == 0.  Tie groups that a resample leaves
 *           empty stay in as repeated points, which changes none of the four.
 * Two tiers; dfd_boot_plan tells which one runs.  n <= DFD_BOOT_LDS_MAX_N: one workgroup per resample keeps its uint32 counts in
 * LDS (4 n bytes behind DFD_BOOT_SCRATCH_BYTES of reduction scratch: together the 160 KiB one workgroup may declare), draws with LDS
 * integer adds and sweeps every member; ws is not read.  Above: counts are uint32 [R][n] in ws, R = min(B, ws_bytes / (4 n))
 * resamples per pass, and the call loops over ceil(B / R) passes of three launches: zero, draw (one workgroup per (resample,
 * tile of DFD_BOOT_DRAW_TILE draws), global integer adds without return), statistics (one workgroup per (resample, member)).
 * The atomics add integers only: counts and statistics do not depend on arrival order or launch geometry.
 *
 * dfd_boot_ws(n, B): the bytes for R = B in the global tier, 0 in the LDS tier or for arguments out of range.
 * dfd_boot_plan: plan[4] = {tier (DFD_BOOT_TIER_LDS / _GLOBAL), R, passes, draw tiles per resample}.
 * dfd_boot_counts: the global tier's zero and draw alone: counts uint32 [R][n] of resamples b0 .. b0 + R - 1 (any n).
 * n == 0 is valid (zeros).  n, B, M, b0 or R out of range, a NULL pointer, or a global-tier ws too small for one resample:
 * DFD_EINVAL, nothing is launched. */
#define DFD_BOOT_STREAM 0x626f6f74u
#define DFD_BOOT_MAX_N (1 << 24)
#define DFD_BOOT_MAX_REPLICATES 65536
#define DFD_BOOT_MAX_MEMBERS 8
#define DFD_BOOT_STATS_LEN 10
#define DFD_BOOT_SCRATCH_BYTES 512
#define DFD_BOOT_LDS_MAX_N ((160 * 1024 - DFD_BOOT_SCRATCH_BYTES) / 4)
#define DFD_BOOT_DRAW_TILE 4096
#define DFD_BOOT_TIER_LDS 0
#define DFD_BOOT_TIER_GLOBAL 1
size_t dfd_boot_ws(int n, int B);
int dfd_boot_plan(int n, int B, int M, size_t ws_bytes, int* plan);
int dfd_boot_counts(int n, int b0, int R, uint64_t seed, uint32_t* counts, dfd_stream stream);
int dfd_boot_stats(const float* const* score_ptrs, const int* const* perm_ptrs, int M, const unsigned char* is_positive,
                   const unsigned char* hit, const double* cuts, int n, int B, uint64_t seed, void* ws, size_t ws_bytes, int64_t* stats,
                   dfd_stream stream);

/* The cluster bootstrap (csrc/dfd_boot.hip, ABI 154): the samples fall into G groups (the frames of a video), and a resample draws
 * whole groups.  group int32 [n] holds each sample's group id in sample order, ids in any order.
 *
 * The resampling rule is the one above with n replaced by G: draw t (0 <= t < G) of resample b runs Philox4x32-10 with the key
 * (seed & 0xffffffff, seed >> 32) and the counter (t >> 2, b, 0, DFD_BOOT_STREAM); u = output word t & 3; the drawn group is
 * ((uint64_t)u * G) >> 32.  g_b[k] is how often group k was drawn, and sample i counts c_b[i] = g_b[group[i]] times; a sample whose id
 * lies outside [0, G) counts for nothing.  With group[i] = i and G = n this is dfd_boot_stats bit for bit.
 *
 * dfd_boot_stats_grouped: dfd_boot_stats' arguments plus group, G and max_size, and the same ten integers per (member, resample) with
 * the same definitions; the weighted sample count P + N of a resample now varies.  max_size is the caller's bound on the largest
 * group: no group may have more members.  (uint64_t)G * max_size must not exceed DFD_BOOT_GROUPED_MAX_WEIGHT = 2^31 - 1, which keeps
 * P, N and the int32 scans exact and two_u below 2^62; scores must be finite.  1 <= G <= n and 1 <= max_size <= n.
 * The counts have G entries, so the tier boundary is on G: G <= DFD_BOOT_LDS_MAX_N runs the LDS tier for any n; above, the
 * workspace is uint32 [R][G] and the zero and draw launches run over G.  The sweep gathers counts[group[perm[i]]].
 * dfd_boot_ws_grouped(n, G, B): the bytes for R = B in the global tier, 0 in the LDS tier or for arguments out of range.
 * dfd_boot_plan_grouped: plan[4] as dfd_boot_plan's, for G counts.  Arguments out of range, a NULL pointer, G * max_size above the
 * bound, or a global-tier ws too small for one resample: DFD_EINVAL, nothing is launched. */
#define DFD_BOOT_GROUPED_MAX_WEIGHT 2147483647
size_t dfd_boot_ws_grouped(int n, int G, int B);
int dfd_boot_plan_grouped(int n, int G, int max_size, int B, int M, size_t ws_bytes, int* plan);
int dfd_boot_stats_grouped(const float* const* score_ptrs, const int* const* perm_ptrs, int M, const unsigned char* is_positive,
                           const unsigned char* hit, const double* cuts, const int* group, int n, int G, int max_size, int B,
                           uint64_t seed, void* ws, size_t ws_bytes, int64_t* stats, dfd_stream stream);

/* Group pooling (csrc/dfd_group.hip, ABI 154): the rows of a group (the frames of a video) become one row.  probs f32 [n][J],
 * group int32 [n] in sample order (any order of ids, 0 <= id < G), targets int64 [n]; 1 <= G <= n <= DFD_GROUP_MAX_N,
 * 1 <= J <= DFD_GROUP_MAX_J, 0 <= positive < J.
 *   out_probs f32 [G][J], out_preds int64 [G] (the first arg max of the stored f32 row), out_targets int64 [G], sizes int32 [G],
 *   info int64 [4] = {invalid rows, ids out of range, groups with mixed targets, empty groups}
 * A row is invalid when a probability is not in [0, 1] (a NaN included; -0.0 is in) or its target is outside [0, J): it is skipped
 * and counted in info[0].  A valid row whose id is outside [0, G) is skipped and counted in info[1].  sizes counts the rows that
 * remain.  A group's target is its smallest member target; a group whose members disagree is counted in info[2].  An empty group
 * gets a row of zeros, pred 0, target -1, size 0 and is counted in info[3].
 *   DFD_GROUP_MEAN  each probability becomes q = llrint((double)p * 4294967296.0), the q are summed per (group, class) in uint64
 *                   (at most 2^24 2^32), and the stored value is (float)((double)sum / ((double)size * 4294967296.0))
 *   DFD_GROUP_VOTE  the same cells; a row adds 2^32 to the cell of its own first arg max: the share of rows voting for each class
 *   DFD_GROUP_MAX   a copy of the member row with the largest probs[i][positive] (-0.0 equals 0.0), the lowest i on ties: a 64-bit
 *                   maximum of the float's bits above 0xffffffff - i, then a gather
 * Only integer adds and maxima are atomic: the outputs do not depend on arrival order, tier or launch geometry.
 * Launches: zero (ws and info), accumulate, finish (one thread per group).  Two accumulate tiers; dfd_group_plan tells which runs.
 * dfd_group_ws(n, G, J) <= DFD_GROUP_LDS_BYTES: every workgroup accumulates into a private copy of the cells in LDS and adds its
 * nonzero cells to ws with one global atomic each.  Above: a wave takes 64 consecutive rows, merges each run of equal ids with a
 * segmented scan over its lanes, and issues one global atomic per cell and run.
 * ws: dfd_group_ws(n, G, J) = G (8 J + 12) bytes, 8-byte aligned, no initial contents required (0 for arguments out of range).
 * dfd_group_plan: plan[4] = {tier (DFD_GROUP_TIER_LDS / _GLOBAL), accumulate workgroups, LDS bytes, finish workgroups}.
 * Arguments out of range, a NULL pointer or a ws too small: DFD_EINVAL, nothing is launched. */
#define DFD_GROUP_MEAN 0
#define DFD_GROUP_VOTE 1
#define DFD_GROUP_MAX 2
#define DFD_GROUP_MAX_N (1 << 24)
#define DFD_GROUP_MAX_J 1024
#define DFD_GROUP_LDS_BYTES 65536
#define DFD_GROUP_LDS_MAX_BLOCKS 256
#define DFD_GROUP_GLOBAL_MAX_BLOCKS 2048
#define DFD_GROUP_TIER_LDS 0
#define DFD_GROUP_TIER_GLOBAL 1
size_t dfd_group_ws(int n, int G, int J);
int dfd_group_plan(int n, int G, int J, int* plan);
int dfd_group_pool(const float* probs, const int* group, const int64_t* targets, int n, int G, int J, int mode, int positive, void* ws,
                   size_t ws_bytes, float* out_probs, int64_t* out_preds, int64_t* out_targets, int* sizes, int64_t* info,
                   dfd_stream stream);

/* Input tail on the device (trainers/efficientnet.py:111-234): a uint8 NHWC
 * batch [N][H][W][3] -> RandomHorizontalFlip -> ToTensor (/255) -> Normalize((x-mean)/std) ->
 * RandomErasing(value 0) -> f32 NHWC, which is the stem kernel's input layout.  The random decisions
 * are made by the caller: flip[n] != 0 mirrors image n; erase[4n..] = {top, left, height, width},
 * height 0 = none; either pointer may be NULL.  mean3 / std3 are HOST arrays of 3 floats.      */
int dfd_image_prep(const unsigned char* src, float* dst, int N, int H, int W, const float* mean3,
                   const float* std3, const unsigned char* flip, const int* erase, dfd_stream stream);
/* torch.optim.AdamW step over a chunk table: int64 rows {param, grad, exp_avg,
 * exp_avg_sq, count}; hp = {lr, beta1, beta2, eps, weight_decay, 1-beta1^t,
 * 1-beta2^t, grad_scale} in device memory (so a captured graph sees new values).   */
#define DFD_ADAMW_TABLE_COLS 5
#define DFD_ADAMW_HP_LEN 8
int dfd_adamw_step(const int64_t* table, int nchunks, const float* hp, dfd_stream stream);
/* Gradient clipping in front of the AdamW step (torch.nn.utils.clip_grad_norm_ / clip_grad_value_), three enqueue-only,
 * capturable launches over the same chunk table; every buffer is the caller's.  NULL pointer or nchunks < 1: DFD_EINVAL before
 * any launch.
 *   dfd_grad_sumsq        one workgroup per table row (only the grad and count columns are read) writes partials[row], a double:
 *                         the sum of the squares of the chunk's f32 gradients, squared and added in f64.  No atomics; the order
 *                         is fixed (elements 4q..4q+3 belong to thread q % 256, a thread adds in rising order, then a wave
 *                         butterfly and (w0 + w1) + (w2 + w3)) and is the same on the 16-byte path and the scalar path, so
 *                         equal chunk contents give equal bits at any alignment and in every run.
 *   dfd_grad_clip_finish  one workgroup adds partials[0 .. nchunks) in f64 (thread t takes t, t + 256, ..., then the same
 *                         tree); one thread then computes in f32
 *                           total = (float)sqrt(sum) * hp[7]           hp: the AdamW record, hp[7] = grad_scale
 *                           coef  = fminf(cfg[0] / (total + 1e-6f), 1) cfg = {limit, mode} in device memory; 1 in value mode
 *                           skip  = !isfinite(total)
 *                         and updates state, DFD_CLIP_STATE_LEN f32 in device memory.  The counters and the norm sum / maximum
 *                         accumulate over calls until the host zeroes the record; a skipped step counts as seen and as
 *                         skipped only.
 *   dfd_adamw_step_clip   dfd_adamw_step reading cfg and state: returns at once, leaving param, exp_avg and exp_avg_sq
 *                         untouched, when state[DFD_CLIP_SKIP] is set; else the gradient is (g * grad_scale) * coef in
 *                         DFD_CLIP_MODE_NORM and fminf(fmaxf(g * grad_scale, -limit), limit) in DFD_CLIP_MODE_VALUE, and
 *                         the rest of the step is dfd_adamw_step's.                                                      */
#define DFD_CLIP_MODE_NORM 0
#define DFD_CLIP_MODE_VALUE 1
#define DFD_CLIP_CFG_LEN 2
#define DFD_CLIP_STATE_LEN 8
#define DFD_CLIP_NORM 0      /* total norm of the last call                 */
#define DFD_CLIP_COEF 1      /* coefficient of the last call                */
#define DFD_CLIP_SKIP 2      /* 1 when the last call's norm was not finite  */
#define DFD_CLIP_STEPS 3     /* calls seen                                  */
#define DFD_CLIP_CLIPPED 4   /* of these: finite norm and coef < 1          */
#define DFD_CLIP_SKIPPED 5   /* of these: norm not finite                   */
#define DFD_CLIP_NORM_SUM 6  /* sum of the finite norms                     */
#define DFD_CLIP_NORM_MAX 7  /* largest finite norm                         */
int dfd_grad_sumsq(const int64_t* table, int nchunks, double* partials, dfd_stream stream);
int dfd_grad_clip_finish(const double* partials, int nchunks, const float* hp, const float* cfg, float* state, dfd_stream stream);
int dfd_adamw_step_clip(const int64_t* table, int nchunks, const float* hp, const float* cfg, const float* state, dfd_stream stream);
/* Exponential moving average of the weights over a chunk table: int64 rows {src, dst, count, kind}, count <= 4096.
 * kind DFD_EMA_LERP: f32 dst = dst + w * (src - dst), rounded as d = src - dst, t = w * d, dst + t (no FMA);
 * kind DFD_EMA_COPY: count 8-byte words copied from src to dst (integer buffers).  w: one f32 in device memory
 * (so a captured graph sees each step's weight).  NULL table / w or nchunks < 1: DFD_EINVAL before any launch.  */
#define DFD_EMA_TABLE_COLS 4
#define DFD_EMA_LERP 0
#define DFD_EMA_COPY 1
int dfd_ema_update(const int64_t* table, int nchunks, const float* w, dfd_stream stream);
/* Mixup / CutMix of an f32 image batch [N][3][H][W] in place (layout: DFD_MIX_NHWC = channels_last memory, DFD_MIX_NCHW =
 * contiguous) and its soft targets y, f32 [N][J].  The partner of sample i is N - 1 - i.  jobs: one row of DFD_MIX_JOB_WORDS
 * 32-bit words per sample in device memory, {mode, w0, w1, y0, y1, x0, x1, 0}; w0 and w1 are f32 bit patterns.
 *   DFD_MIX_KEEP    picture untouched, y[i] = onehot(labels[i])
 *   DFD_MIX_MIXUP   x[i] = x[i] * w0 + x[N-1-i] * w1, rounded as a = x_i * w0, b = x_j * w1, a + b (no FMA)
 *   DFD_MIX_CUTMIX  pixels with y0 <= row < y1 and x0 <= col < x1 take the partner's value, all channels
 * with x_i, x_j the values before the launch; the two jobs of a pair may differ.  Targets of the two mixing modes: zeros,
 * y[i][labels[i]] = w0, then y[i][labels[N-1-i]] += w1.  The middle sample of an odd N is always kept.  Boxes are clamped to
 * the picture and a label outside [0, J) matches no class.  NULL pointer, N < 1, J < 1, H < 1, W < 1 or an unknown layout:
 * DFD_EINVAL before any launch.                                                      */
#define DFD_MIX_JOB_WORDS 8
#define DFD_MIX_KEEP 0
#define DFD_MIX_MIXUP 1
#define DFD_MIX_CUTMIX 2
#define DFD_MIX_NHWC 0
#define DFD_MIX_NCHW 1
int dfd_mix_batch(float* x, const int64_t* labels, const int32_t* jobs, float* y, int N, int H, int W, int J, int layout,
                  dfd_stream stream);

/* ------------------------------------------------------------ token mixers ---
 * What the EfficientFormerV2 (timm 1.0.20 efficientformer_v2.py: Attention2d, Attention2dDownsample,
 * LocalGlobalQuery, Downsample, Stem4) and FasterViT (fastervit 1.0.0 faster_vit.py: WindowAttention,
 * HAT, ConvBlock, PatchEmbed, LayerNorm) modules need beyond the MBConv kernels.  Reference call sites:
 * trainers/efficientformer_v2.py:244,215,369 and trainers/fastervit.py:271,235 (`model(inputs)`).       */

/* out = a[c]*dz + b[c]*y + c[c]  (BatchNorm input gradient, materialised)                                */
int dfd_affine2_apply(int dtype, const void* dz, const void* y, const float* coef, void* out, long rows,
                      int C, dfd_stream stream);
/* out = act(scale*y + shift + other); bnstate == NULL: y as is; other == NULL: no addend                 */
int dfd_bn_add_act(int dtype, const void* y, const float* bnstate, const void* other, int act, void* out,
                   long rows, int C, dfd_stream stream);
/* d = g * act'(scale*y + shift + other); partials (optional, needs bnstate): sums of (d, d*xhat)          */
int dfd_bn_add_act_bwd(int dtype, const void* g, const void* y, const float* bnstate, const void* other,
                       int act, void* d, long rows, int C, float* partials, int pcap, int* nparts,
                       dfd_stream stream);
/* per-channel (sum, sumsq) partial slabs [nparts][2][C] of a plain [rows][C] tensor                        */
int dfd_channel_stats(int dtype, const void* x, long rows, int C, float* partials, int pcap, int* nparts,
                      dfd_stream stream);
/* out[i] (+)= sum_p partials[p][i], fixed order; `partials` needs room for P + ceil(P/32) rows of L floats  */
int dfd_sum_rows(float* partials, int P, long L, float* out, int accumulate, dfd_stream stream);
/* dfd_sum_rows whose launch may be left to an open dfd_sum_batch_begin / _end (results nobody reads inside the batch:
 * parameter gradients summed straight into their destination)                                                    */
int dfd_sum_rows_deferred(float* partials, int P, long L, float* out, int accumulate, dfd_stream stream);
/* out [N][2h][2w][C] = act(bilinear_x2(s [N][h][w][C])), align_corners = False (nn.Upsample in Attention2d) */
int dfd_up2_act_fwd(int dtype, const void* s, int act, void* out, int N, int h, int w, int C, dfd_stream stream);
/* ws (optional): scratch of the size and type of g; with it the activation derivative is evaluated once per output
 * element (two launches) instead of once per interpolation tap                                                 */
int dfd_up2_act_bwd(int dtype, const void* g, const void* s, int act, void* ds, int N, int h, int w, int C,
                    void* ws, dfd_stream stream);
/* LocalGlobalQuery: out[n,i,j,:] = a[n,i,j,:] + bias[:] + x[n, i*stride, j*stride, :]  (AvgPool2d(1, stride))
 * and its gradient into x: dx[n, i*stride, j*stride, :] += g[n,i,j,:]                                        */
int dfd_subsample_add(int dtype, const void* a, const float* bias, const void* x, void* out, int N, int H,
                      int W, int stride, int C, dfd_stream stream);
int dfd_subsample_add_bwd(int dtype, const void* g, void* dx, int N, int H, int W, int stride, int C,
                          dfd_stream stream);

/* Small strided batched GEMM  C[b,h,m,n] = alpha * sum_k A[b,h,m,k] * B[b,h,k,n] (+ bias[h,m,n]).
 * Element (b, h, r, c) of an operand is at base + b*sb + h*sh + r*sr + c*sc (element units), so q / k / v
 * are read in place from the NHWC projection outputs and the result lands in NHWC.  dt_*: DFD_F32 / DFD_BF16.
 * round_a / round_b: round that operand to bf16 after loading (an f32 intermediate standing in for a tensor
 * a bf16 pipeline would have stored).  (M*(K+1) + K*N) * 4 bytes must fit in 150 KiB of LDS.               */
typedef struct { long sb, sh, sr, sc; } dfd_mat;
int dfd_bgemm(int dt_a, const void* A, const dfd_mat* sa, int dt_b, const void* B, const dfd_mat* sb,
              int dt_c, void* C, const dfd_mat* sc, const float* bias, float alpha, int nb, int nh, int M,
              int N, int K, int round_a, int round_b, dfd_stream stream);
/* Which kernel dfd_bgemm runs for (M, N, K) and the rounding flags (ABI 148; host code, the decision dfd_bgemm itself takes):
 * 0 = the LDS-panel kernel with 4 x 4 register tiles, 1 = the chunked long-K kernel (M, N <= 16 and panels beyond 48 KiB),
 * 2 = the K-parallel kernel (M, N <= 8, K >= 512), DFD_EUNSUPPORTED = panels beyond 150 KiB that neither of the two takes.  */
int dfd_bgemm_plan(int M, int N, int K, int round_a, int round_b);
/* Attention rows on S [B][H][Nq][Nk] f32:  [T1 = W1*S + b1 over heads ->] P = softmax_k(T1) [-> T2 = W2*P + b2]
 * th_w1 == NULL: no talking heads (T2 unused).  H <= 16, Nk <= 256.                                          */
int dfd_attn_softmax_fwd(const float* S, const float* th_w1, const float* th_b1, const float* th_w2,
                         const float* th_b2, float* P, float* T2, int B, int H, int Nq, int Nk,
                         dfd_stream stream);
/* dT2 -> dS (and dT1, the gradient at the softmax input, when talking heads are on)                           */
int dfd_attn_softmax_bwd(const float* dT2, const float* P, const float* th_w1, const float* th_w2,
                         float* dT1, float* dS, int B, int H, int Nq, int Nk, dfd_stream stream);
/* The launch shape of both for (H, Nk) (ABI 148; host code): *R = (b, query) rows per workgroup, *team = threads that share the
 * maximum and the sums of one (head, row) pair.  Returns DFD_OK or the error the launchers return; R / team may be NULL.     */
int dfd_attn_softmax_plan(int H, int Nk, int* R, int* team);
/* learned attention bias table [H][T] <-> full [H][L] through idx [L] (int32)                                 */
int dfd_bias_gather(const float* table, const int* idx, float* full, int H, int T, long L, dfd_stream stream);
int dfd_bias_scatter(const float* dfull, const int* idx, float* dtable, int H, int T, long L, int accumulate,
                     dfd_stream stream);

/* Dense k x k convolution, forward, as an implicit GEMM: the NT GEMM kernel gathers its A operand from the NHWC image
 * (row = output pixel, column = (tap, input channel)), applying the producer's BN + activation to the gathered values
 * (zero padding in the activated domain); nothing is materialised.  w_nk [Cout][k*k*C] in the activation dtype, column
 * (kh*k + kw)*C + c (dfd_conv_weight_perm + dfd_pw_prep_weights).  C % 8 == 0, Cout % 8 == 0.  Output, partials and
 * nparts as dfd_pwconv_fwd.  Reference call sites: the 3x3 convolutions of timm's EfficientFormerV2 stem and of
 * NVlabs FasterViT's PatchEmbed / ConvBlock / Downsample, reached from trainers/<model>.py `model(x)`.                  */
int dfd_conv_fwd(int dtype, const void* x, const dfd_dwconv_shape* s, const float* in_bnstate, int in_act,
                 const void* w_nk, int Cout, void* y, float* partials, int pcap, int* nparts, dfd_stream stream);

/* Weight gradient of the same convolution: dw[Cout][k*k*C] (f32, GEMM column order) = sum over output pixels of
 * P(p)[m][co] * im2col(act(bn(x)))[m][(tap, c)], the im2col operand gathered inside the TN kernel.  p / pro_p as for
 * dfd_pwconv_wgrad (DFD_PRO_NONE or the BN-backward map DFD_PRO_AFFINE2); ws: dfd_conv_wgrad_ws() bytes.            */
size_t dfd_conv_wgrad_ws(const dfd_dwconv_shape* s, int Cout);
int dfd_conv_wgrad(int dtype, const void* p, const dfd_prologue* pro_p, int Cout, const void* x,
                   const dfd_dwconv_shape* s, const float* in_bnstate, int in_act, float* dw, int accumulate,
                   float* ws, size_t ws_bytes, dfd_stream stream);

/* Dense k x k convolution = im2col + the 1x1 GEMM entry points (data gradient; forward: dfd_conv_fwd).  Shapes use dfd_dwconv_shape (C = input
 * channels).  col [N*Ho*Wo][k*k*C] with column index (kh*k + kw)*C + c; zero padding in the activated domain. */
int dfd_im2col(int dtype, const void* x, const float* in_bnstate, int in_act, void* col,
               const dfd_dwconv_shape* s, dfd_stream stream);
int dfd_col2im(int dtype, const void* dcol, void* dx, const dfd_dwconv_shape* s, dfd_stream stream);
/* torch's [O][I][k][k] f32 <-> the GEMM's [O][(kh,kw,i)]; to_gemm = 0 maps a weight gradient back; to_gemm = 2 writes
 * [I][(flipped tap, o)]: with it the data gradient of a stride-1 convolution is dfd_conv_fwd on the output gradient   */
int dfd_conv_weight_perm(const float* src, float* dst, int O, int I, int k, int to_gemm, int accumulate,
                         dfd_stream stream);

/* LayerNorm over C of [rows][C]; stats [rows][2] = (mean, rstd).  Backward partials [nparts][2][C]
 * (row 0: dgamma, row 1: dbeta), summed by dfd_sum_rows.                                                      */
int dfd_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* y,
                      float* stats, long rows, int C, dfd_stream stream);
int dfd_layernorm_bwd(int dtype, const void* g, const void* x, const float* gamma, const float* stats,
                      const void* residual, void* dx, float* partials, int pcap, int* nparts, long rows, int C,
                      dfd_stream stream);

/* Token bookkeeping of windowed attention (fastervit faster_vit.py window_partition / window_reverse /
 * ct_dewindow / ct_window / cat / split): dst[didx[r]] = src[sidx[r]], r < n, rows of C elements; a NULL index
 * array is the identity.  For the one-to-one maps above the backward pass is the same call with the arrays swapped. */
int dfd_copy_rows(int dtype, const void* src, const int* sidx, void* dst, const int* didx, long n, int C,
                  dfd_stream stream);
/* PosEmbMLPSwinv1D: out[r] = x[r] + table[r % T] (table f32 [T][C]); dtable[t] = sum_w g[w*T + t]              */
int dfd_add_rowtable(int dtype, const void* x, const float* table, void* out, long rows, int T, int C,
                     dfd_stream stream);
size_t dfd_rowtable_grad_ws(int T, int C);       /* bytes of scratch for dfd_rowtable_grad (no initial contents required) */
int dfd_rowtable_grad(int dtype, const void* g, float* dtable, long rows, int T, int C, int accumulate,
                      float* ws, size_t ws_bytes, dfd_stream stream);
/* The launch shape of dfd_rowtable_grad for the same (dtype, rows, T, C) (ABI 149; host code, the decision dfd_rowtable_grad itself
 * takes): *splits = slices of the rows / T windows summed apart (grid z), *w_per = windows per slice (the last one may hold fewer),
 * *rpb = row lanes of a workgroup.  Any of the three may be NULL.  DFD_EINVAL where dfd_rowtable_grad rejects the shape. */
int dfd_rowtable_grad_plan(int dtype, long rows, int T, int C, int* splits, long* w_per, int* rpb);
/* nn.AvgPool2d(k, stride) without padding on NHWC (TokenInitializer) and its gradient (dx [N][H][W][C])         */
int dfd_avgpool_fwd(int dtype, const void* x, void* out, int N, int H, int W, int k, int stride, int C,
                    dfd_stream stream);
int dfd_avgpool_bwd(int dtype, const void* g, void* dx, int N, int H, int W, int k, int stride, int C,
                    dfd_stream stream);
/* PosEmbMLPSwinv2D: full [H][S][S], S = n_local + n_global: 16*sigmoid(table[idx[i*n_local+j]][h]) in the local
 * block, zeros in the first n_global rows / columns; table f32 [T][H]; backward through the sigmoid into dtable  */
int dfd_relpos_bias_fwd(const float* table, const int* idx, float* full, int H, int n_local, int n_global,
                        dfd_stream stream);
int dfd_relpos_bias_bwd(const float* dfull, const float* table, const int* idx, float* dtable, int H, int T,
                        int n_local, int n_global, dfd_stream stream);

/* ---------------------------------------------------------------- bookkeeping ---
 * Small kernels that keep ATen off the model path (drop-connect / dropout randoms, counters, scaling).        */
/* out = (a_dev ? a*a_dev[0] : a) * x + b * y   (y may be NULL), f32                                           */
int dfd_axpby(const float* x, const float* y, float a, float b, const float* a_dev, float* out, long n,
              dfd_stream stream);
/* out = a + b, n elements of `dtype`, n % 8 == 0                                                               */
int dfd_add(int dtype, const void* a, const void* b, void* out, long n, dfd_stream stream);
/* Philox4x32-10 uniforms.  rng_state (device): {seed, offset}; counter = (offset, stream_id, index/4).
 * keep <= 0: out = U[0,1);  keep in (0,1]: out = floor(keep + u) / keep  (per-sample drop-path scale)          */
int dfd_rand(const uint64_t* rng_state, uint32_t stream_id, float keep, float* out, long n, dfd_stream stream);
/* once per forward pass: *counter_ptrs[i] += 1 (BatchNorm num_batches_tracked, int64) and rng offset += 1.
 * counter_ptrs is a DEVICE array of ncounters addresses.                                                       */
int dfd_step_tick(const int64_t* counter_ptrs, int ncounters, uint64_t* rng_state, dfd_stream stream);

/* ------------------------------------------------------- MX fp8 (FasterViT fp8 weights) ---
 * BASELINE config 5 ("FasterViT-0 bf16/fp8 weights ... on CDNA4 fp8 MFMA"); carries the Linear layers (qkv / proj /
 * fc1 / fc2) of the third-party module's forward at trainers/fastervit.py:271 (training), :235 (evaluate) and
 * orchestration/orchestrator.py:529,590 (inference) when `fp8_weights` is switched on.
 * Format: OCP microscaling FP8 — e4m3fn elements, one E8M0 scale byte (2^(b-127)) per 32 consecutive K elements:
 *   e = clamp(floor(log2(max|v|)) - 8, -127, 127);  q = e4m3_rne_sat(v * 2^-e);  scale byte = e + 127.
 * The GEMM is v_mfma_scale_f32_16x16x128_f8f6f4 (the one fp8 form above the bf16 MFMA rate); it takes BOTH operands in this
 * format, so activations are quantised the same way (dfd_mx_quant_rows) right before the product.  K % 128 == 0.          */
typedef struct dfd_mx_job {
    const float* src;      /* f32 master weight [N][K]                                                       */
    uint8_t* q;            /* e4m3fn [N][K]                                                                  */
    uint8_t* scale;        /* e8m0 [N][K/32]                                                                 */
    void* kn;              /* optional: DEQUANTISED weight, transposed [K][N], element type kn_dtype
                              (what the bf16 data-gradient GEMM multiplies by)                               */
    int N, K;
    int kn_dtype;
    int _pad;
} dfd_mx_job;
/* all fp8 weights of a network in one call (32 jobs per launch); `jobs` is a HOST array */
int dfd_mx_quant_weights_multi(const dfd_mx_job* jobs, int njobs, dfd_stream stream);
/* a [M][K] (dtype) [-> act(coef[0][k]*a + coef[1][k]) rounded to dtype: prologue modes DFD_PRO_NONE / DFD_PRO_BN_ACT]
 * -> q e4m3fn [M][K], scale e8m0 [M][K/32]                                                                              */
int dfd_mx_quant_rows(int dtype, const void* a, const dfd_prologue* pro, uint8_t* q, uint8_t* scale, long M, int K,
                      dfd_stream stream);
/* out[M][N] (dtype_out) = dequant(aq, ascale) . dequant(wq, wscale)^T, f32 accumulation; wq [N][K], N % 4 == 0       */
int dfd_mx_gemm(const uint8_t* aq, const uint8_t* ascale, const uint8_t* wq, const uint8_t* wscale, int dtype_out,
                void* out, long M, int K, int N, dfd_stream stream);

/* ------------------------------------------------ fused window attention (FasterViT) ---
 * WindowAttention of the third-party module (forward at trainers/fastervit.py:271, backward at :274), bf16, head_dim 32,
 * T <= 64 tokens per window:  o = softmax_k(scale * q k^T + bias[h]) v  with q / k / v read in place from the qkv projection
 * output [n][T][3*H*32] and o written as [n][T][H*32].  One wave per (window, head) on v_mfma_f32_16x16x32_bf16; S and P stay
 * in registers.  L [n][H][T] f32 = row max + log(row sum) (saved for the backward, which recomputes P).  bias f32 [H][T][T]
 * or NULL.  Backward writes dqkv [n][T][3*H*32] and, when dbias_parts != NULL, dfd_wattn_parts(n) rows of [H][T][T] f32
 * (sum over 4 windows each) for dfd_sum_rows.  DFD_EUNSUPPORTED for other head dimensions / longer windows (callers then
 * use dfd_bgemm + dfd_attn_softmax_*).                                                                                  */
int dfd_wattn_parts(int n);
int dfd_wattn_fwd(const void* qkv, const float* bias, void* out, float* L, int n, int T, int H, int hd, float scale,
                  dfd_stream stream);
int dfd_wattn_bwd(const void* qkv, const void* dout, const float* L, const float* bias, void* dqkv, float* dbias_parts,
                  int n, int T, int H, int hd, float scale, dfd_stream stream);

/* ------------------------------------------------ attention GEMMs of Attention2d (EfficientFormerV2) ---
 * timm's Attention2d (forward at trainers/efficientformer_v2.py:244) mixes the heads of a (query, key) pair before and after the
 * softmax ("talking heads"), so S / P / T2 stay f32 [B][H][Nq][Nk] tensors for dfd_attn_softmax_*; the six batched products
 * around them run here on v_mfma_f32_16x16x32_bf16, one wave per (image, head), instead of on dfd_bgemm:
 *   dfd_attn_scores  out[b][h][i][j] = alpha * sum_d x[b][i][h*D + d] * y[b][j][h*D + d] (+ bias[h][i][j])
 *                    x [n][Tx][H*D], y [n][Ty][H*D] bf16; out f32 [n][H][Tx][Ty]; bias f32 [H][Tx][Ty] or NULL         (S, dT2)
 *   dfd_attn_apply   out[b][i][h*D + d] = alpha * sum_t f[b][h][i][t] * x[b][t][h*D + d]      (f_trans = 0, f [n][H][To][Tc])
 *                                       = alpha * sum_t f[b][h][t][i] * x[b][t][h*D + d]      (f_trans = 1, f [n][H][Tc][To])
 *                    f f32 (rounded to bf16 for the product, f32 accumulation); x [n][Tc][H*D], out [n][To][H*D] bf16  (O, dQ | dV, dK)
 * Token counts <= 256 (walked in blocks of 64), D % 8 == 0, D <= 128; anything else: DFD_EUNSUPPORTED (callers keep dfd_bgemm).     */
int dfd_attn_scores(const void* x, const void* y, float* out, const float* bias, float alpha, int n, int H, int Tx, int Ty,
                    int D, dfd_stream stream);
int dfd_attn_apply(const float* f, int f_trans, const void* x, void* out, float alpha, int n, int H, int To, int Tc, int D,
                   dfd_stream stream);

/* -------------------------------------------- batched coordinate MLPs (FasterViT) ---
 * PosEmbMLPSwinv1D / PosEmbMLPSwinv2D of the third-party module:  table[t][:] = W2 . relu(W0 . coords[t] + b0), f32,
 * coords [T][2] constant, W0 [Hd][2], b0 [Hd], W2 [D][Hd] (Hd = 512).  They depend on parameters only, so a whole level's
 * tables are computed by one call before its first block and differentiated by one call after its last
 * (2 + 2 launches instead of ~280 per step).  `jobs` are HOST arrays (copied into kernel arguments, 24 per launch).
 * forward reads coords / w0 / b0 / w2 and writes table [T][D]; backward reads dtable [T][D] too and writes the non-NULL ones
 * of dw0 [Hd][2], db0 [Hd], dw2 [D][Hd] (overwriting).  T <= 176, Hd <= 1024, Hd % 4 == 0.                               */
typedef struct dfd_cmlp_job {
    const float *coords, *w0, *b0, *w2;
    float* table;
    const float* dtable;
    float *dw0, *db0, *dw2;
    int T, D, Hd, _pad;
} dfd_cmlp_job;
int dfd_coord_mlp_fwd_multi(const dfd_cmlp_job* jobs, int njobs, dfd_stream stream);
int dfd_coord_mlp_bwd_multi(const dfd_cmlp_job* jobs, int njobs, dfd_stream stream);
/* dfd_relpos_bias_fwd / _bwd for every attention layer of a level at once: table [T][H], idx int32 [n_local^2],
 * full / dfull [H][S][S] with S = n_local + n_global, dtable [T][H].                                                     */
typedef struct dfd_relpos_job {
    const float* table;
    const int* idx;
    float* full;
    const float* dfull;
    float* dtable;
    int H, T, n_local, n_global;
} dfd_relpos_job;
int dfd_relpos_bias_fwd_multi(const dfd_relpos_job* jobs, int njobs, dfd_stream stream);
int dfd_relpos_bias_bwd_multi(const dfd_relpos_job* jobs, int njobs, dfd_stream stream);

/* ---------------------------------------------------------------- Grad-CAM ---
 * Reference call site web_ui.py:275-282:
 *     with GradCAM(model=..., target_layers=[target]) as cam:
 *         grayscale = cam(input_tensor=batch, targets=[ClassifierOutputTarget(cls_idx)])[0]
 *     overlay = show_cam_on_image(_tensor_to_rgb(tensor), grayscale, use_rgb=True)
 * pytorch_grad_cam's GradCAM with one target layer and show_cam_on_image with image_weight 0.5, for a whole batch
 * (csrc/dfd_cam.hip spells the arithmetic out; tests/_cam_ref.py restates it in numpy f32, operation by operation).
 *
 * dfd_gradcam_map: act, grad NHWC [N*HW][C] of `dtype` (the target layer's output and its gradient) -> cam_out f32 [N][HW]
 *   = max(0, sum_c mean_p(grad[n,p,c]) * act[n,p,c]).  1 <= C <= 16384, any C; one launch, fixed summation order.     */
int dfd_gradcam_map(const void* act, const void* grad, int dtype, int N, int HW, int C, float* cam_out, dfd_stream stream);
/* dfd_cam_render: cam f32 [N][h][w] (dfd_gradcam_map's output) -> heat_out f32 [N][H][W], min-max scaled, cv2 INTER_LINEAR
 *   resized, ReLU'd and min-max scaled again; and, unless overlay_out is NULL, overlay_out uint8 [N][H][W][3] =
 *   uint8(255 * o / max(o)) with o = (1 - image_weight) * lut[uint8(255 heat)] / 255 + image_weight * clamp(x * std + mean, 0, 1).
 *   image: the normalised model input, f32 NCHW [N][3][H][W]; mean_std f32 [6] (mean[3], std[3]) and lut uint8 [256][3] (RGB)
 *   in device memory.  image, mean_std and lut may be NULL when overlay_out is.  One launch; the workspace holds the
 *   horizontal pass (dfd_cam_render_ws bytes, DFD_EWORKSPACE when smaller).                                                */
int dfd_cam_render(const float* cam, int N, int h, int w, int H, int W, const float* image, const float* mean_std,
                   const unsigned char* lut, double image_weight, float* heat_out, unsigned char* overlay_out,
                   void* workspace, size_t ws_bytes, dfd_stream stream);
size_t dfd_cam_render_ws(int N, int h, int w, int H, int W);

#ifdef __cplusplus
}
#endif
#endif /* DFD_HIP_H */
