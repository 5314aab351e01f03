/* resunet_hip.h -- C-ABI of libresunet_hip.so, the MI355X (gfx950) implementation of the ResUNet hot path
 * of lachinov/brats2019.
 *
 * The reference has no FFI of its own: the path is stock torch.nn calls inside model.py / loss.py.  This
 * header is therefore the boundary a maintainer binds with ctypes; each entry point
 * names the reference call site (file:line into the reference repo) whose arithmetic it replaces.
 *
 * Conventions:
 *   - all tensors are contiguous NCDHW float32 DEVICE pointers owned by the caller (PyTorch-ROCm
 *     `tensor.data_ptr()`); the library never allocates user-visible memory -- scratch comes from the
 *     caller-provided workspace (`ws`, `ws_bytes`; sizes from the *_workspace_bytes queries);
 *   - every function enqueues on `stream` (a hipStream_t passed as void*; 0 = default stream), performs no
 *     device synchronisation and no hipMalloc: calls are graph-capturable;
 *   - return 0 on success, a negative RU_E* code on error; `ru_last_error()` returns the thread-local
 *     message; nothing throws across the ABI.
 */
#ifndef RESUNET_HIP_H_
#define RESUNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RU_OK 0
#define RU_EINVAL (-1)    /* bad argument / unsupported shape */
#define RU_ENOMEM (-2)    /* workspace too small */
#define RU_EHIP (-3)      /* HIP runtime error (launch failed ...) */
#define RU_ESTATE (-4)    /* call order violated (backward without forward ...) */

/* arithmetic of the 3x3x3 convolutions (everything else is always float32):
 *   RU_PREC_F32    exact float32 products on v_mfma_f32_16x16x4_f32 (bit-for-bit an fmaf chain)
 *   RU_PREC_BF16X3 split-bf16: v = hi + lo (2 x bf16), products hi*hi + lo*hi + hi*lo on v_mfma_f32_16x16x32_bf16 with
 *                  float32 accumulation; ~2^-16 relative per product, |dp| ~ 5e-5 on the whole network (bar: 1e-3).
 *                  Needs W % 4 == 0, otherwise the f32 kernel runs.  HBM tensors stay float32 in both modes. */
#define RU_PREC_F32 0
#define RU_PREC_BF16X3 1
#define RU_PREC_BF16 2        /* gradient precision only (ru_unet_set_grad_precision): plain bf16 operands, one MFMA product, fp32 accumulate */

typedef void* ru_stream_t;                /* hipStream_t */
typedef struct ru_unet* ru_unet_t;        /* opaque engine handle */

const char* ru_last_error(void);
int ru_version(void);                     /* 100*major + minor */
/* 1 if a HIP device is usable by this process, 0 otherwise (never throws) */
int ru_device_ok(void);

/* ---------------------------------------------------------------- convolutions
 * nn.Conv3d as the reference constructs it: (k=3,stride=1,pad=1) model.py:72-73,336,348;
 * (k=2,stride=2,pad=0) model.py:361-363; (k=1,stride=1,pad=0) model.py:393,401.  Cross-correlation,
 * zero padding, weight layout [Cout][Cin][k][k][k].  D,H,W are the INPUT extents; for k=2 they must be even.
 * `bias` may be NULL.  Exact-f32 arithmetic (v_mfma_f32_16x16x4_f32 / v_fmac_f32).
 * ru_conv3d_workspace_bytes is the largest of the dry walks (the entry's own carve, run on the host without launches) it covers, plus 4096:
 * ru_conv3d_fwd / _bwd_data / _bwd_weight and their _p forms at both precisions, db included; for k = 3 also ru_conv3d_bwd_weight_l and
 * ru_conv3d_fwd_l / ru_conv3_l for every `flags` (bits 0-7) without bits 2 and 6 (those two take more: ru_conv3_l_workspace_bytes).  */
size_t ru_conv3d_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int k);
int ru_conv3d_fwd(const float* x, const float* w, const float* bias, float* y,
                  int N, int Cin, int Cout, int D, int H, int W, int k,
                  void* ws, size_t ws_bytes, ru_stream_t stream);
/* same as ru_conv3d_fwd / ru_conv3d_bwd_data with an explicit RU_PREC_* for k=3 (k=1,2 are always float32) */
int ru_conv3d_fwd_p(const float* x, const float* w, const float* bias, float* y,
                    int N, int Cin, int Cout, int D, int H, int W, int k, int precision,
                    void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_conv3d_bwd_data_p(const float* dy, const float* w, float* dx,
                         int N, int Cin, int Cout, int D, int H, int W, int k, int precision,
                         void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_conv3d_bwd_weight_p(const float* x, const float* dy, float* dw, float* db,
                           int N, int Cin, int Cout, int D, int H, int W, int k, int precision,
                           void* ws, size_t ws_bytes, ru_stream_t stream);
/* dx = d(loss)/dx given dy (autograd of the calls above) */
int ru_conv3d_bwd_data(const float* dy, const float* w, float* dx,
                       int N, int Cin, int Cout, int D, int H, int W, int k,
                       void* ws, size_t ws_bytes, ru_stream_t stream);
/* dw [Cout][Cin][k][k][k] and (if db != NULL) db[Cout] */
int ru_conv3d_bwd_weight(const float* x, const float* dy, float* dw, float* db,
                         int N, int Cin, int Cout, int D, int H, int W, int k,
                         void* ws, size_t ws_bytes, ru_stream_t stream);
/* The split-K form of the exact-f32 k = 3 forward, as the engine runs its small exact-f32 shapes: `ksplit` partial output tensors, each the sum over its
 * slice of the 8-channel input chunks, added in slice order.  ksplit = 0: the factor the engine would take for the shape (the high half of
 * ru_conv3_f32_inst); 1, given or chosen: the plain launch.  Refused: a factor that does not divide the chunks, a bias beside a split.
 * ru_conv3d_fwd_splitk_workspace_bytes: the dry walk of the entry (packed weight and partial tensors), plus 4096. */
size_t ru_conv3d_fwd_splitk_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int ksplit);
int ru_conv3d_fwd_splitk(const float* x, const float* w, const float* bias, float* y,
                         int N, int Cin, int Cout, int D, int H, int W, int ksplit,
                         void* ws, size_t ws_bytes, ru_stream_t stream);
/* What a launch of the NCDHW family chooses -- host-only queries of the functions the launchers switch on (no launch, no workspace):
 * ru_conv3_f32_inst: conv3_f32_kernel<TZ, TY, KC, NT> of an exact-f32 k = 3 convolution (forward, or the data gradient with Cin / Cout exchanged) and the
 *   engine's split factor: TZ | TY << 4 | KC << 8 | NT << 12 | ksplit << 16; negative: bad shape.
 * ru_wgrad3_inst: the k = 3 weight gradient; flags 1: x voxel-major, 2: dy voxel-major.  out7 = kernel (0 wgrad3_f32_kernel, 1 wgrad3_sb_kernel, 2 the
 *   transpose-read kernel: the rest 0, see ru_wgrad3_l), OT, CT, X16, DY16, nbx (workgroups per channel group), ntile (tiles they walk).
 * ru_conv1_inst: the pointwise launch behind k = 1 (V = D*H*W) and k = 2 (forward: Cin * 8 channels at V / 8 voxels; data gradient: Cout -> Cin * 8):
 *   0 conv1_mfma_kernel, 1 conv1_kernel<1, 4>, 2 conv1_kernel<4, 16>.
 * ru_wgrad1_inst: the k = 1 / k = 2 weight gradient on NCDHW tensors: out3 = OT | CT << 4 (as ru_wgrad1_l reports), nbx, nchunk (chunks of 256 voxels per sample). */
int ru_conv3_f32_inst(int N, int Cin, int Cout, int D, int H, int W);
int ru_wgrad3_inst(int N, int Cin, int Cout, int D, int H, int W, int precision, int flags, int* out7);
int ru_conv1_inst(int N, int Cin, int Cout, size_t V);
int ru_wgrad1_inst(int N, int Cin, int Cout, size_t V, int* out3);

/* ---------------------------------------------------------------- GroupNorm (+ fused LeakyReLU / residual)
 * nn.GroupNorm(G, C), eps, affine (model.py:95-96,338) followed by LeakyReLU(slope) (model.py:93-94; pass
 * slope = 1 for "no activation", as after norm_input, model.py:413) and, if residual != NULL, the Residual
 * skip add `x + out` (model.py:115).  V = D*H*W.  mean/rstd: [N*G] outputs (saved for backward).
 * ru_groupnorm_workspace_bytes: the larger of the dry walks of ru_groupnorm_fwd and ru_groupnorm_bwd, plus 4096.  */
size_t ru_groupnorm_workspace_bytes(int N, int C, size_t V);
int ru_groupnorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                     float* mean, float* rstd, int N, int C, size_t V, int G, float eps, float slope,
                     void* ws, size_t ws_bytes, ru_stream_t stream);
/* backward of y = lrelu(GN(x)): dy is d/d(activated output); the LeakyReLU mask is recomputed from the sign
 * of the normalised value (== sign of the in-place output the reference keeps).
 * dgamma/dbeta are OVERWRITTEN.  */
int ru_groupnorm_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                     const float* dy, float* dx, float* dgamma, float* dbeta,
                     int N, int C, size_t V, int G, float slope,
                     void* ws, size_t ws_bytes, ru_stream_t stream);

/* ---------------------------------------------------------------- LeakyReLU (model.py:352,422) */
int ru_leaky_relu_fwd(const float* x, float* y, size_t n, float slope, ru_stream_t stream);
int ru_leaky_relu_bwd(const float* y, const float* dy, float* dx, size_t n, float slope, ru_stream_t stream);

/* ---------------------------------------------------------------- trilinear x2 (model.py:12-14)
 * F.interpolate(scale_factor=2, mode='trilinear'), align_corners=False.  D,H,W = INPUT extents.  */
int ru_upsample2x_trilinear_fwd(const float* x, float* y, int N, int C, int D, int H, int W, ru_stream_t stream);
int ru_upsample2x_trilinear_bwd(const float* dy, float* dx, int N, int C, int D, int H, int W, ru_stream_t stream);

/* ---------------------------------------------------------------- sigmoid (model.py:351,431) */
int ru_sigmoid_fwd(const float* x, float* y, size_t n, ru_stream_t stream);

/* ---------------------------------------------------------------- criterion (loss.py:64-79,98-122; train.py:203-205)
 * Phase 1: per-class partial sums over THIS rank's shard, float64:
 *     sums[0..C)  = sum_{n,v} p*g          (Dice intersection, no epsilon)
 *     sums[C..2C) = sum_{n,v} (p*p + g)    (Dice union, no epsilon)
 *     sums[2C]    = sum g*log(p+1e-6) + bg_weight*(1-g)*log((1+1e-6)-p)
 * (all-reduce `sums` across data-parallel ranks between the phases).
 * Phase 2: dp = w_dice * dDice/dp + w_bce * dBCE/dp with the GLOBAL sums and GLOBAL element count
 * (`count` = N_global*C*V).  The reference's training criterion is w_dice = w_bce = 0.5, bg_weight 1e-2,
 * priority 1 (main.py:126-128).  loss value: see ru_criterion_value().  */
size_t ru_criterion_workspace_bytes(int N, int C, size_t V);
int ru_criterion_sums(const float* p, const float* g, double* sums, int N, int C, size_t V, float bg_weight,
                      void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_criterion_grad(const float* p, const float* g, const double* sums, double count,
                      float w_dice, float w_bce, float bg_weight, float priority,
                      float* dp, int N, int C, size_t V, ru_stream_t stream);
/* host helper: (dice, bce) from global sums (host pointer) */
int ru_criterion_value(const double* sums_host, int C, double count, double priority, double* dice, double* bce);
/* the same on the device, one launch, no host sync: out[0] = w_dice*dice + w_bce*bce (train.py:203-205 with w = 1/2), out[1] = dice
 * (loss.py:114-122), out[2] = bce (loss.py:79) as float64, from the (all-reduced) device sums */
int ru_criterion_value_device(const double* sums, int C, double count, double priority, double w_dice, double w_bce,
                              double* out3, ru_stream_t stream);

/* ---------------------------------------------------------------- criterion lists (loss.py:15-195; train.py:203-205)
 * Every criterion of the reference's loss.py that applies to the [N, C, D, H, W] probabilities is a closed form in per-row moments
 * (row = one (n, c), V voxels), and its gradient is dL/dp = a*g + b*p + c + d*g/(p+1e-6) + e*(1-g)/((1+1e-6)-p), a..e per row.
 *   ru_crit_moments : moments[(n*C + c)*RU_CRIT_MOMENTS + m], float64, one streaming pass (float per 8192-voxel chunk, double across).
 *                     `mask` (bits 1 << RU_CRIT_M_*): the two log moments are computed only when one of their bits is set, else 0;
 *                     the other moments are always written.  ws: ru_crit_moments_workspace_bytes(N, C, V) bytes.  Any V.
 *   ru_crit_reduce  : out[c*RU_CRIT_MOMENTS + m] = sum over the N samples of moments[n, c, m]; out[C*RU_CRIT_MOMENTS] = sum over n and
 *                     c >= 1 of Dice_loss_separate's (2 sum pg + 1) / (sum (p^2 + g) + 1).  C*RU_CRIT_MOMENTS + 1 doubles: the
 *                     buffer to all-reduce (SUM) across data-parallel ranks, and nothing else crosses ranks.
 *   ru_crit_eval    : one launch, no host sync.  terms: HOST array of `nterms` (1..RU_CRIT_MAX_TERMS), copied into the kernel argument.
 *                     From the all-reduced `totals` and this shard's `moments` [N, C, M]: values[0] = sum_t weight_t * L_t, values[1+t] =
 *                     L_t (float64); coef[(n*C + c)*5 + {a,b,c,d,e}] (float32) = sum_t weight_t * (coefficients of dL_t/dp).  count =
 *                     N_global*C*V, n_global = the global batch.  Reference quirks kept: GDL_joint and Dice_loss_separate skip channel 0,
 *                     sens_loss_joint does not; Dice_loss_separate ignores its priority; a class absent from the global batch gives
 *                     GDL_joint w_c = inf, so its value and gradient are NaN, as in torch.
 *   ru_crit_grad    : dp = f(p, g, coef[row]) * (*scale when scale != NULL; a float32 DEVICE scalar).  with_logs = 0 skips the d and e
 *                     terms (pass 1 whenever a CE or BCE term is in the list).
 * p, g and dp need only float alignment: the moments and apply passes move 16 bytes at a time when V % 4 == 0 and the pointers they read or
 * write are 16-byte aligned, and one element at a time otherwise (the same arithmetic per element; the moments' order of summation differs).  */
#define RU_CRIT_DICE_JOINT 0      /* Dice_loss_joint(index, priority)     loss.py:98-122 */
#define RU_CRIT_BCE 1             /* BCE_Loss(index, bg_weight)           loss.py:64-79 */
#define RU_CRIT_MSE 2             /* MSE_Loss(index, priority)            loss.py:15-29 */
#define RU_CRIT_CE 3              /* CE_Loss(index)                       loss.py:52-61 */
#define RU_CRIT_DICE1D 4          /* Dice1D(label_index)                  loss.py:81-96 */
#define RU_CRIT_GDL_JOINT 5       /* GDL_joint(index, priority)           loss.py:125-150 */
#define RU_CRIT_SENS_JOINT 6      /* sens_loss_joint(index, priority)     loss.py:153-174 */
#define RU_CRIT_DICE_SEPARATE 7   /* Dice_loss_separate(index, priority)  loss.py:176-195 */
#define RU_CRIT_NUM_KINDS 8
#define RU_CRIT_MAX_TERMS 8
#define RU_CRIT_M_PG 0            /* sum p*g */
#define RU_CRIT_M_PP 1            /* sum p*p */
#define RU_CRIT_M_P 2             /* sum p */
#define RU_CRIT_M_G 3             /* sum g */
#define RU_CRIT_M_GLOGP 4         /* sum g*log(p + 1e-6) */
#define RU_CRIT_M_QLOGQ 5         /* sum (1-g)*log((1+1e-6) - p) */
#define RU_CRIT_M_D2 6            /* sum (p-g)^2 */
#define RU_CRIT_MOMENTS 7
#define RU_CRIT_MASK_ALL 0x7fu
typedef struct {
    int kind;                     /* RU_CRIT_* */
    double weight;                /* weight in the total (train.py:203-205: 1 / len(list)) */
    double priority;              /* the module's priority (1 where it has none) */
    double bg_weight;             /* BCE_Loss only */
} ru_crit_term_t;
size_t ru_crit_moments_workspace_bytes(int N, int C, size_t V);
int ru_crit_moments(const float* p, const float* g, int N, int C, size_t V, unsigned mask, double* moments,
                    void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_crit_reduce(const double* moments, int N, int C, double* out, ru_stream_t stream);
int ru_crit_eval(const double* totals, const double* moments, int N, int C, double count, double n_global,
                 const ru_crit_term_t* terms, int nterms, double* values, float* coef, ru_stream_t stream);
int ru_crit_grad(const float* p, const float* g, const float* coef, const float* scale, int N, int C, size_t V, int with_logs,
                 float* dp, ru_stream_t stream);

/* ---------------------------------------------------------------- criteria for hard voxels and small regions (csrc/hardcrit.hip)
 * Beside the reference's list: focal loss, Tversky / focal-Tversky and top-k cross entropy on the same float32 probabilities p and targets
 * g in [0, 1] (soft labels allowed), n = N*C*V elements taken flat.  p + 1e-6 and (1 + 1e-6) - p are float32 expressions, as in BCE_Loss.
 * No float atomics, no host synchronisation; two calls give identical bytes.
 *   ru_focal_sum    : *sum_out (float64) = sum over this shard of f = -(a1 g (1-p)^gamma log(p+1e-6) + a0w (1-g) p^gamma log((1+1e-6)-p)),
 *                     a0w = a0 * bg_weight.  gamma == 0 or gamma >= 1.  One streaming pass, one float64 partial per workgroup, added in a
 *                     fixed order.  The loss is the (all-reduced) sum / count.  ws: ru_focal_workspace_bytes(n).
 *   ru_focal_grad   : dp = df/dp / count * (*scale when scale != NULL; a float32 DEVICE scalar); count = n * world.
 *   ru_tversky_eval : from ru_crit_reduce's (all-reduced) totals: *value = priority * mean_c (1 - TI_c)^(1/gamma), TI_c = (TP + s) /
 *                     (TP + alpha FP + beta FN + s), TP = sum pg, FP = sum p - TP, FN = sum g - TP over batch and space; coef[N*C*5] in
 *                     ru_crit_grad's layout (a and c non-zero): the backward is ru_crit_grad(..., with_logs = 0).
 *   ru_topk_select  : the K largest l = -(g log(p+1e-6) + bg_weight (1-g) log((1+1e-6)-p)) of this shard, exactly.  l is formed once and
 *                     stored in keys[n] as a 32-bit key in l's order (-0 as +0, NaN above all); the K-th largest key is found by a radix
 *                     select of 11 / 11 / 10 bits (integer histograms).  out2[0] = (sum of l > t + (K - n_gt) t) / K, out2[1] = t;
 *                     state[4] = {the key of t, K - n_gt, n_gt, n_eq}.  n < 2^32.  ws: ru_topk_workspace_bytes(n).
 *   ru_topk_grad    : dp = dl/dp / (K * world) where l > t, dl/dp (K - n_gt) / (n_eq K world) where l == t, else 0, times *scale; reads
 *                     the keys and the state ru_topk_select left, so both see the same bits of l. */
size_t ru_focal_workspace_bytes(size_t n);
int ru_focal_sum(const float* p, const float* g, size_t n, float gamma, float a1, float a0w, double* sum_out, void* ws, size_t ws_bytes,
                 ru_stream_t stream);
int ru_focal_grad(const float* p, const float* g, size_t n, float gamma, float a1, float a0w, double count, const float* scale, float* dp,
                  ru_stream_t stream);
int ru_tversky_eval(const double* totals, int N, int C, double alpha, double beta, double gamma, double smooth, double priority,
                    double* value, float* coef, ru_stream_t stream);
size_t ru_topk_workspace_bytes(size_t n);
int ru_topk_select(const float* p, const float* g, size_t n, unsigned long long K, float bg_weight, unsigned* keys, unsigned long long* state,
                   double* out2, void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_topk_grad(const float* p, const float* g, const unsigned* keys, const unsigned long long* state, size_t n, unsigned long long K,
                 float bg_weight, double world, const float* scale, float* dp, ru_stream_t stream);

/* ---------------------------------------------------------------- boundary and Hausdorff distance-transform losses (csrc/boundary.hip)
 * Criteria on exact Euclidean distance maps made on the device (definitions: INTEGRATION.md).  Unit isotropic spacing, every axis in
 * [1, 512] (larger: RU_EINVAL).  No float atomics, no host synchronisation; two calls give identical bytes.
 *   ru_signed_sqdist : x: float32 [items][D][H][W], one mask M = x > 0.5f per item (an item is a (sample, channel) pair).  out: int32
 *                      [items][D][H][W] = s_M: + the squared distance to the nearest voxel of M at a voxel outside M, - the squared
 *                      distance to the nearest voxel not in M at a voxel inside it, both exact integers of at least 1; 0 everywhere when M
 *                      is empty or the whole grid (decided on the device).  The W, H and D passes of csrc/edt_exact.hpp; every voxel is
 *                      written once.  items <= 32767.  ws: ru_signed_sqdist_workspace_bytes(items, D, H, W) (8 bytes per voxel and item).
 *   With F = sqrt(|s|) and phi = F where s > 0, -(F - 1) where s < 0, 0 where s == 0, both formed in float32 from the integer:
 *   ru_boundary_sum  : *sum_out (float64) = sum over this shard of p * phi_G (each product exact in float64).  One streaming pass, one
 *                      float64 partial per workgroup, added in a fixed order.  ws: ru_boundary_workspace_bytes(n).
 *   ru_boundary_grad : dp = coef * phi_G * (*scale when scale != NULL; a float32 DEVICE scalar); coef = priority / (n * world).
 *   ru_hddt_sum      : *sum_out = sum of (p - g)^2 (F_P^alpha + F_G^alpha); the weight in float32 (alpha == 2: the integers themselves,
 *                      alpha == 1: sqrtf, else powf(|s|, alpha / 2)), the difference and the products in float64.  alpha > 0, finite.
 *                      ws: ru_boundary_workspace_bytes(n).
 *   ru_hddt_grad     : dp = coef * 2 (p - g) (F_P^alpha + F_G^alpha) * (*scale); the maps are constants under differentiation. */
size_t ru_signed_sqdist_workspace_bytes(int items, int D, int H, int W);
int ru_signed_sqdist(const float* x, int items, int D, int H, int W, int* out, void* ws, size_t ws_bytes, ru_stream_t stream);
size_t ru_boundary_workspace_bytes(size_t n);
int ru_boundary_sum(const float* p, const int* s_g, size_t n, double* sum_out, void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_boundary_grad(const int* s_g, size_t n, float coef, const float* scale, float* dp, ru_stream_t stream);
int ru_hddt_sum(const float* p, const float* g, const int* s_p, const int* s_g, size_t n, float alpha, double* sum_out, void* ws,
                size_t ws_bytes, ru_stream_t stream);
int ru_hddt_grad(const float* p, const float* g, const int* s_p, const int* s_g, size_t n, float alpha, float coef, const float* scale,
                 float* dp, ru_stream_t stream);

/* ---------------------------------------------------------------- lesion-wise Dice loss (csrc/lesion_loss.hip)
 * The blob loss (Kofler et al. 2022) on Dice_loss_joint's Dice: the training-side counterpart of ru_lesion_metrics (definition and
 * degenerate cases: INTEGRATION.md).  p, g: float32 [N][C][D][H][W], finite values in [0, 1]; every extent in [1, 512], D * H * W < 2^31,
 * N * C <= 65535.  Per (n, c): G = g > 0.5f; Z = G dilated `dilation` times by the 18-neighbour structure; the lesions T_i = G & Z_i, Z_i
 * the 26-connected components of Z (ru_lesion_metrics' grouping), vol_i = |T_i|; kept: vol_i > min_volume, L of them.  The domain of
 * lesion i is the background (not G; Z \ G included) and T_i.  Per voxel qI = llrint(p g 2^35), qU = llrint(p p 2^35) + llrint(g 2^35)
 * from exact float64 products; I_i, U_i = the 64-bit integer sums over the domain times 2^-35; Dice_i = 2 (I_i + 1e-6) / (U_i + 2e-6),
 * a_i = 2 / (U_i + 2e-6), b_i = 4 (I_i + 1e-6) / (U_i + 2e-6)^2 in float64; pair loss l_nc = 1 - (sum over kept Dice_i) / L where L >= 1.
 * Loss = priority * (sum of l_nc over the pairs with L >= 1) / M, M = their number in the GLOBAL batch; 0 when M = 0.
 *   ru_lesion_loss_forward: labels_out int32 [N][C][V]: -1 outside G, else the root of the voxel's component of Z = the smallest linear
 *                     index of that component (the root itself may lie in Z \ G and then holds -1).  state_out: ru_lesion_loss_state_bytes
 *                     bytes, 16-byte aligned, five slices at the byte offsets the call reports: [0] per pair 64 bytes {A = sum kept a_i,
 *                     B = sum kept b_i, l_nc (float64); L, lesions (int64); the background's integer sums qI0, qU0 (uint64); 0};
 *                     [1] vol int32 [N*C][V], [2] qI and [3] qU uint64 [N*C][V]: a lesion's own sums at its root, 0 elsewhere;
 *                     [4] (a_i, b_i) float64 pairs [N*C][V], written AT ROOTS ONLY (zeros for a dropped lesion), undefined elsewhere.
 *                     totals_out float64 [2] = {sum of l_nc over THIS call's pairs with L >= 1, their number}: all that crosses ranks.
 *                     stats_out int64 [N][C][2] = {lesions, L}.  The number of lesions is not limited.  Integer atomics only; the
 *                     float64 sums run in an order fixed by the shape: two calls give identical bytes.  No host synchronisation.
 *                     ws: ru_lesion_loss_workspace_bytes(N, C, D, H, W) (0 for a bad shape).
 *   ru_lesion_loss_grad: dp = s (b p - a g), s = priority * (*scale when scale != NULL; a float32 DEVICE scalar) / (M * L), M =
 *                     totals_global[1] read on the device (the all-reduced totals); (a, b) = (a_i, b_i) in a kept lesion, (0, 0) in a
 *                     dropped one (exact zeros), (A, B) on the background; zeros for a pair with L = 0 and everywhere when M = 0.
 *                     Float64 arithmetic, rounded once to float32.  One streaming pass, no atomics.
 *   ru_lesion_loss_forward_upto: the forward cut short after `passes` of its four passes (1: clears, pack, dilation; 2: + labelling;
 *                     3: + sum; 4: + evaluate = ru_lesion_loss_forward): what tools/lesion_loss_time.py times pass by pass.  The outputs
 *                     are complete only with passes = 4. */
size_t ru_lesion_loss_workspace_bytes(int N, int C, int D, int H, int W);
size_t ru_lesion_loss_state_bytes(int N, int C, int D, int H, int W, size_t* offsets5);
int ru_lesion_loss_forward(const float* p, const float* g, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                           int* labels_out, void* state_out, double* totals_out, long long* stats_out, void* ws, size_t ws_bytes,
                           ru_stream_t stream);
int ru_lesion_loss_forward_upto(const float* p, const float* g, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                                int* labels_out, void* state_out, double* totals_out, long long* stats_out, void* ws, size_t ws_bytes,
                                int passes, ru_stream_t stream);
int ru_lesion_loss_grad(const float* p, const float* g, const int* labels, const void* state, const double* totals_global, double priority,
                        const float* scale, float* dp, int N, int C, int D, int H, int W, ru_stream_t stream);

/* ---------------------------------------------------------------- optimizer (main.py:133-142)
 * torch.optim.Adam(amsgrad=True) with L2 weight decay added to the gradient; `step` is 1-based.  */
int ru_adam_amsgrad_step(float* w, const float* g, float* m, float* v, float* vmax, size_t n,
                         float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         ru_stream_t stream);
/* the same with amsgrad optional: vmax_or_null == NULL is torch.optim.Adam(amsgrad=False).  What brats2019_amd.optim.Adam.step() -- the
 * optimizer class Trainer.train instantiates in place of torch.optim.Adam (main.py:134, train.py:82-83) -- calls once per contiguous run
 * of parameters of the flat buffer.  */
int ru_adam_step(float* w, const float* g, float* m, float* v, float* vmax_or_null, size_t n,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                 ru_stream_t stream);

/* ---------------------------------------------------------------- the rest of the recipe (optim.hip; brats2019_amd.optim)
 * Streaming kernels over runs of the flat parameter / gradient bucket.  A run may start at any ELEMENT offset: a lane owns 4 consecutive
 * floats and moves them as 16 bytes, the elements before the first 16-byte boundary and after the last whole quad go one by one (all
 * of a call's pointers must sit at the same offset from a 16-byte boundary for that, as runs of buffers laid out alike do; otherwise the
 * whole run goes one float per lane).  Grids are capped and stride.  Nothing waits for the host, and there are no float atomics.
 *
 * Global L2 norm of any number of runs, in float64 (squares and sums: 1e20 does not overflow, 1e-30 does not vanish).  A partial call
 * on n elements writes ru_gradnorm_slots(n) float64 partial sums into ws[first_slot ...], one per workgroup; give every run its own
 * slots.  ru_gradnorm_workspace_bytes(n_total, n_runs) covers any split of n_total elements into n_runs runs.  The finalize is ONE
 * workgroup that adds slots [0, n_slots) in a fixed order (a lane adds its contiguous share in index order, lane 0 the 256 shares in
 * lane order): the same bytes in give the same bytes out.  It writes norm_out[0] = sqrt(sum) (float64, device) and
 * coef_out[0] = (float) min(1, max_norm / (norm + 1e-6)) (device), torch.nn.utils.clip_grad_norm_'s coefficient with its clamp, formed
 * in float64.  A non-finite norm gives a non-finite coefficient (error_if_nonfinite=False); there is no skip policy.  */
size_t ru_gradnorm_slots(size_t n);
size_t ru_gradnorm_workspace_bytes(size_t n_total, size_t n_runs);
int ru_gradnorm_partial(const float* g, size_t n, size_t first_slot, double* ws, size_t ws_bytes, ru_stream_t stream);
int ru_gradnorm_finalize(const double* ws, size_t n_slots, double max_norm, double* norm_out, float* coef_out, ru_stream_t stream);
/* g[i] = coef[0] * g[i] in place, coef on the device: clipping for optimizers that are not this library's.  */
int ru_scale_by(float* g, size_t n, const float* coef, ru_stream_t stream);
/* torch.optim.SGD's update with the device coefficient folded in (coef_or_null == NULL: gc = g):
 *   gc = coef[0] * g;  d = gc + weight_decay * w;  buf = first ? d : momentum * buf + (1 - dampening) * d;
 *   u = nesterov ? d + momentum * buf : buf;  w -= lr * u.
 * momentum == 0 takes no buffer (buf_or_null == NULL, u = d); `first` is torch's "momentum_buffer is None" (buf is written, not read).
 * coef * g is rounded on its own, so a coefficient of exactly 1 gives the bytes of the call without one.  */
int ru_sgd_step(float* w, const float* g, float* buf_or_null, size_t n, float lr, float momentum, float dampening, float weight_decay,
                int nesterov, int first, const float* coef_or_null, ru_stream_t stream);
/* decoupled != 0: torch.optim.AdamW (w *= 1 - lr * weight_decay first, the gradient is not decayed).  decoupled == 0: the arithmetic of
 * ru_adam_step, line for line, on coef[0] * g (equal bytes when coef_or_null == NULL).  `step` is 1-based.  */
int ru_adamw_step(float* w, const float* g, float* m, float* v, float* vmax_or_null, size_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, int step,
                  const float* coef_or_null, ru_stream_t stream);
/* ema[i] = fmaf(decay, ema[i], (1 - decay) * w[i]), decay in [0, 1].  */
int ru_ema_update(float* ema, const float* w, size_t n, float decay, ru_stream_t stream);
/* exchanges a[0..n) and b[0..n) in place (they must not overlap).  */
int ru_swap_f32(float* a, float* b, size_t n, ru_stream_t stream);

/* ---------------------------------------------------------------- whole-network engine
 * model.UNet(depth, encoder_layers, decoder_layers, number_of_channels, number_of_outputs) (model.py:309)
 * with block=Residual and 4 input channels (model.py:336).  Parameters live in ONE flat float buffer in
 * reference state_dict() order (ru_unet_param_* describe it); gradients are written to a flat buffer of
 * the same layout (dead parameters -- decoder_convs.{depth-1}.*, decoder_convs1x1.{depth-1} -- get zeros,
 * model.py:420: they are constructed but never executed).  */
ru_unet_t ru_unet_create(int depth, const int* encoder_layers, const int* decoder_layers,
                         const int* number_of_channels, int number_of_outputs);
void ru_unet_destroy(ru_unet_t h);
/* RU_PREC_* used by the 3x3x3 convolutions (forward, data gradient, weight gradient) of subsequent forward/backward calls;
 * default RU_PREC_F32.  Change it only between steps (not between a forward and its backward).  */
int ru_unet_set_precision(ru_unet_t h, int precision);
/* Inference with constant weights: frozen != 0 promises that the values behind `params` and the workspace `ws` are not modified between
 * ru_unet_forward calls; the weight packs the forward builds at the head of `ws` are then built once and reused while the same
 * (params pointer, ws pointer, precision) come back (they are rebuilt otherwise).  Training must leave it off (0, the default): the
 * reference's optimizer changes the weights every step (train.py:220).  */
int ru_unet_freeze_params(ru_unet_t h, int frozen);
int ru_unet_get_precision(ru_unet_t h);
/* Arithmetic of the 3x3x3 DATA and WEIGHT gradients of subsequent ru_unet_backward calls when the forward precision is RU_PREC_BF16X3
 * (ignored otherwise).  RU_PREC_BF16X3 (default): three split-bf16 products like the forward, gradients within ~1e-5 relative of float32.
 * RU_PREC_BF16: the operands of the gradient convolutions are rounded to bf16 (hi*hi only, fp32 accumulate) -- BASELINE configs[2]
 * ("bf16 forward+backward") taken literally for the backward; the forward, and with it the probabilities (bar 1e-3, train.py:201-205 /
 * model.py:407-433), is untouched.  One third of the matrix work and half of the operand staging in those kernels; parameter gradients
 * then carry bf16 rounding noise (relative L2 error ~3e-3 per tensor against the float32 reference, tests/test_hip_unet.py).  The
 * persistent voxel-major kernels honour it (every level of the shipped configuration at training sizes); the small-shape fallbacks and
 * the 4-channel stem / head data paths keep three products. */
int ru_unet_set_grad_precision(ru_unet_t h, int precision);
int ru_unet_get_grad_precision(ru_unet_t h);
/* Backward-pass fusions of the voxel-major split-bf16 engine (on by default unless noted; same arithmetic either way up to summation order --
 * the separate passes stay available so that tests can hold the fused kernels to them):
 *   RU_FUSE_GN_BWD_STATS  the GroupNorm-backward sums are taken in the epilogue of the data-gradient conv that produces the incoming
 *                         gradient (no reduce pass over (y, d));
 *   RU_FUSE_GN_BWD_APPLY  16-channel level: the GroupNorm-backward apply is computed in the weight gradient's dy staging (no apply pass). */
#define RU_FUSE_GN_BWD_STATS 1
#define RU_FUSE_GN_BWD_APPLY 2
/*   RU_FUSE_SIDE_STREAM   the 3x3x3 weight gradients below the 16-channel level run on a second (library-owned, lower-priority) HIP stream,
 *                         event-ordered behind the kernel that produces their dy and joined before ru_unet_backward returns: same kernels,
 *                         same arithmetic, bit-identical gradients; the memory-bound passes of the chain run in their shadow.  */
#define RU_FUSE_SIDE_STREAM 4
/*   RU_FUSE_BATCH_WREDUCE the per-workgroup partials of every weight gradient of a backward pass are summed by ONE launch behind the last
 *                         weight-gradient kernel (nobody reads a weight gradient before the optimizer) instead of one small launch each:
 *                         same summation order, bit-identical gradients.
 *   RU_FUSE_TAIL_FINALIZE the GroupNorm statistics (forward) and the GroupNorm-backward coefficients are finalized by the LAST workgroup of
 *                         the kernel that produces their partial sums (one integer ticket per launch, reset by the finisher; partials
 *                         published with agent-scope stores and read back in the same fixed order: deterministic, no float atomics)
 *                         instead of by a finalize launch behind it.  OFF by default: built, verified and measured (round 4) -- the
 *                         serial tail (ticket + reading the partials back through the fabric) costs what the finalize launch and its
 *                         boundary cost.  */
#define RU_FUSE_BATCH_WREDUCE 8
#define RU_FUSE_TAIL_FINALIZE 16
/*   RU_FUSE_PW_DGRAD      decoder 1x1x1 conv over the (never materialised) concat, Cout <= 32: its weight-gradient kernel also forms the data
 *                         gradient of both halves from the dy tile it has staged (LeakyReLU backward of the up-sampled half included) --
 *                         one pass over (dy, skip, up) instead of two.  */
#define RU_FUSE_PW_DGRAD 32
int ru_unet_set_fusion(ru_unet_t h, unsigned mask);
/* In-situ timing of the dominant kernel (bench.py's roofline line): while enabled, every forward brackets its launches of
 * the 3x3x3 convolution 16 -> 16 at the input resolution (voxel-major split-bf16 engine; the forward of the shipped net has four) with a
 * HIP event pair on the stream the kernels run on.  ru_unet_probe_read waits for the recorded events, returns the summed duration and
 * the number of launches since the last read, and clears the record.  Off by default; costs two event records per probed launch. */
int ru_unet_probe(ru_unet_t h, int enable);
int ru_unet_probe_read(ru_unet_t h, double* total_ms, int* launches);
/* ru_unet_probe(h, 2): EVERY launch of ru_unet_forward / ru_unet_backward is bracketed and booked to one of RU_PROBE_FAMILIES kernel
 * families (bench.py's `roofline_families`): 0 3x3x3 conv fwd + data gradient at the 16-channel level (stem and head included), 1 the
 * same at the deeper levels, 2 / 3 3x3x3 weight gradients likewise, 4 GroupNorm passes (apply, backward reduce / apply, finalizes),
 * 5 1x1 / 2x2x2 convolutions, their weight gradients and the trilinear kernels, 6 everything else (weight packing, fills, head
 * gradient, partial-sum reductions of the weight gradients).  ms[f] = summed duration, launches[f] = count since the last read.
 * The event records cost ~1 us per launch: use it in probe steps, not in a timed region.
 * nfam = RU_PROBE_FAMILIES + RU_PROBE_INSTANCES additionally returns, behind the families, the launches that are ONE kernel instantiation worth naming
 * (bench.py's `roofline_top`; each is booked to its family as well): 0 / 1 the 16 -> 16 voxel-major 3x3x3 convolution forward / data gradient, 2 / 3 the
 * 32..128-channel ones, 4 the 16-channel level's weight gradient with the GroupNorm-backward apply fused into its staging, 5 the one without, 6 the
 * 32..128-channel weight gradients. */
#define RU_PROBE_FAMILIES 7
#define RU_PROBE_INSTANCES 7
int ru_unet_probe_read_families(ru_unet_t h, double* ms, int* launches, int nfam);
int ru_unet_param_count(ru_unet_t h);
const char* ru_unet_param_name(ru_unet_t h, int i);          /* state_dict key */
int ru_unet_param_ndim(ru_unet_t h, int i);
int ru_unet_param_dim(ru_unet_t h, int i, int d);
size_t ru_unet_param_offset(ru_unet_t h, int i);             /* in floats, into the flat buffer */
size_t ru_unet_param_total(ru_unet_t h);                     /* floats */
int ru_unet_param_is_dead(ru_unet_t h, int i);
/* Bytes of device workspace `ws` a forward (training == 0: inference, block temporaries are recycled) or a forward + backward pair
 * (training != 0: every activation is kept) needs at this shape; 0 for extents the network cannot take.  `ws` must be 256-byte aligned
 * (any hipMalloc pointer is) and may be larger than asked for. */
size_t ru_unet_workspace_bytes(ru_unet_t h, int N, int D, int H, int W, int training);
/* UNet.forward (model.py:407-433): x [N,4,D,H,W] -> probs [N,n_out,D,H,W] (sigmoid).  D,H,W divisible by
 * 2^(depth-1).  training != 0 keeps activations in `ws` for ru_unet_backward; `x` and `probs` are then read again by
 * ru_unet_backward (weight gradient of conv_input; sigmoid backward) and must stay valid and unmodified until it has run.  */
int ru_unet_forward(ru_unet_t h, const float* params, const float* x, float* probs,
                    int N, int D, int H, int W, int training,
                    void* ws, size_t ws_bytes, ru_stream_t stream);
/* loss.backward() through the network (train.py:210): dprobs = d(loss)/d(probs) -> grads (flat, overwritten).
 * Must follow a training-mode ru_unet_forward with the same params/ws.  dx (may be NULL) = d/d(input).  */
int ru_unet_backward(ru_unet_t h, const float* params, const float* dprobs, float* grads, float* dx,
                     ru_stream_t stream);
/* The same with the criterion's gradient formed on the way (train.py:203-210: `loss = (Dice + BCE) / 2; loss.backward()`): dprobs is not an
 * operand but the second phase of the criterion -- ru_criterion_grad(probs, target, sums, count, w_dice, w_bce, bg_weight, priority) --
 * evaluated inside the head's sigmoid-backward pass from the probabilities the forward wrote to the caller's buffer, `target` and the
 * (all-reduced) `sums` of ru_criterion_sums: the gradient w.r.t. the probabilities is never written or read back (one pass instead of
 * three over the class tensors; the same float expressions, so the gradients agree with the two-call sequence to float rounding --
 * 1e-7 relative L2 measured, tests/test_hip_unet.py).  */
int ru_unet_backward_criterion(ru_unet_t h, const float* params, const float* target, const double* sums, double count,
                               float w_dice, float w_bce, float bg_weight, float priority, float* grads, float* dx,
                               ru_stream_t stream);
/* per-layer GroupNorm statistics of the last forward, for parity checks: copies mean/rstd [N*8] of the
 * idx-th executed GroupNorm (execution order) into DEVICE buffers.  Returns number of GN layers if idx<0. */
int ru_unet_gn_stats(ru_unet_t h, int idx, float* mean, float* rstd, ru_stream_t stream);

/* ---------------------------------------------------------------- data-parallel collectives (replaces nn.DataParallel, main.py:61)
 * One process per GPU, full replica each, minibatch sharded over the ranks.  Per step two SUM all-reduces keep the result
 * identical to the reference's global-batch step: the [2C+1] float64 criterion sums between ru_criterion_sums and ru_criterion_grad
 * (Dice_loss_joint sums over the GLOBAL batch, loss.py:114-115), and the live runs of the flat float32 gradient buffer after
 * ru_unet_backward (SUM, not mean).  ru_allreduce enqueues ncclAllReduce (RCCL over xGMI) on `stream` -- the stream of the kernels --
 * in place; no host synchronisation.  librccl is bound at run time: the library loads without it, these calls then fail with RU_EHIP.
 * Set-up: rank 0 calls ru_comm_unique_id and hands the RU_COMM_ID_BYTES bytes to every rank out of band (the host mirror broadcasts
 * them through torch.distributed or a file); every rank then calls ru_comm_init with its HIP device current.  */
typedef struct ru_comm* ru_comm_t;
#define RU_COMM_ID_BYTES 128
#define RU_DT_F32 0
#define RU_DT_F64 1
int ru_comm_unique_id(void* id_out /* RU_COMM_ID_BYTES host bytes */);
int ru_comm_init(ru_comm_t* out, const void* id, int rank, int world);
int ru_comm_destroy(ru_comm_t c);
int ru_comm_rank(ru_comm_t c);
int ru_comm_world(ru_comm_t c);
int ru_allreduce(ru_comm_t c, void* buf, size_t count, int dtype, ru_stream_t stream);
/* ncclGroupStart / ncclGroupEnd: the ru_allreduce calls between them are issued as ONE RCCL launch (the runs of the gradient bucket of
 * a step; replaces the per-parameter reduce_add loop inside nn.DataParallel's backward, main.py:61) */
int ru_comm_group_begin(void);
int ru_comm_group_end(void);

/* ---------------------------------------------------------------- inference post-processing (test.py:115-159)
 * ru_tta_merge: `probs` holds K predictions [K][C][D][H][W] of flipped copies of one volume; bits 3k..3k+2 of `flips` say
 * which axes (bit0 D, bit1 H, bit2 W) copy k was reversed along (test.py:117-120 uses {none, D, H, D+H}).  Each prediction
 * is un-flipped (test.py:134-136) and they are averaged as sum(outputs)/K in list order (test.py:138, float32).  Outputs:
 * mean_out [C][D][H][W] (may be NULL), mask [C][V] uint8 = mean > 0.5 (test.py:144), counts[C] = voxels set per channel.
 * It is ru_tta_merge_box on the box covering the volume, served by the merge family of csrc/ensemble.hip: 32-bit voxel indices, so
 * D*H*W >= INT_MAX is refused (RU_EINVAL, "volume too large for 32-bit voxel indices"), and C <= 65535.
 * ru_compose_labels: labels[v] = 2 where mask[0], then 1 where mask[1], then 4 where mask[2] if counts[2] > et_min
 * (test.py:153-159, et_min = 32).  counts is read on the device: no host synchronisation.  */
int ru_tta_merge(const float* probs, int K, unsigned flips, float* mean_out, unsigned char* mask, unsigned long long* counts,
                 int C, int D, int H, int W, ru_stream_t stream);
int ru_compose_labels(const unsigned char* mask, const unsigned long long* counts, unsigned long long et_min, unsigned char* labels,
                      size_t V, ru_stream_t stream);

/* ---------------------------------------------------------------- inference driver on the device (csrc/inference.hip)
 * Sliding window (loader_helper.py:34-97, train.py:158-174).  `origins` = T x 3 HOST ints, index_min of each tile (get_indices: centre
 * block position * centre - border; may be negative).  ru_tile_gather is loader_helper.copy for T tiles in one launch: tiles
 * [(t*N + n), C, td, th, tw] = data[n, :, origin + (z, y, x)], zero outside the volume (tw % 4 == 0).  ru_tile_scatter is
 * loader_helper.copy_back: the centre block [border, border + center) of every tile is pasted at origin + border, clipped at the end
 * of the volume.  Centre blocks of different tiles do not overlap, so the order of the tiles does not matter.  */
int ru_tile_gather(const float* data, float* tiles, int N, int C, int D, int H, int W, int T, const int* origins,
                   int td, int th, int tw, ru_stream_t stream);
int ru_tile_scatter(const float* tiles, float* out, int N, int C, int D, int H, int W, int T, const int* origins,
                    int td, int th, int tw, const int* border, const int* center, ru_stream_t stream);
/* Blended sliding window (csrc/blend.hip): overlapping tiles, every predicted voxel used, weighted by a window that falls off towards the
 * tile's edge.  Geometry: per axis a HOST list of tile starts, beginning at 0, strictly increasing, without gaps, the last tile reaching
 * the volume's end (a tile may stick out of the volume: ru_tile_gather reads zeros there, what is predicted there is dropped); the tiles
 * are the Cartesian product of the three lists, tile index = (iz*ny + iy)*nx + ix.  `profiles` = DEVICE float32 [td + th + tw], the window
 * profiles gz, gy, gx one behind the other.  Fixed float32 arithmetic, comparable bit for bit with numpy:
 *   weight of tile voxel (z, y, x)   w = fl32(fl32(gz[z] * gy[y]) * gx[x])
 *   per volume voxel and channel, over the tiles that cover it IN RISING TILE INDEX:  S <- fl32(S + fl32(w*p)),  Wn <- fl32(Wn + w), from 0
 *   result = fl32(S / Wn) by a true division; no fma contraction, no atomics: two calls give identical bytes.
 * ru_blend_accumulate: folds tiles [t0, t0 + T) -- `tiles` holds these T only, in ru_tile_gather's layout [(t*N + n), C, td, th, tw] -- into
 *   acc [N][C][D][H][W].  A gather over the volume voxels inside the bounding box of the launch's tiles, so overlapping tiles of one call do
 *   not race and the result does not depend on how the tiles are split into calls.  The calls of one volume must come in rising t0 and cover
 *   every tile once: a voxel whose smallest covering tile index is >= t0 is WRITTEN (S starts from 0, acc is not read -- no memset), every
 *   other one continues from acc.  tw % 4 == 0; tile rows are read 16 bytes at a time where (x - start_x) % 4 == 0, by dwords elsewhere.
 * ru_blend_finalize: out = acc / Wn with Wn recomputed from the start lists and the profiles (no second volume); out may alias acc.  */
int ru_blend_accumulate(const float* tiles, float* acc, const float* profiles, int N, int C, int D, int H, int W, int td, int th, int tw,
                        const int* starts_z, int nz, const int* starts_y, int ny, const int* starts_x, int nx, int t0, int T, ru_stream_t stream);
int ru_blend_finalize(const float* acc, float* out, const float* profiles, int N, int C, int D, int H, int W, int td, int th, int tw,
                      const int* starts_z, int nz, const int* starts_y, int ny, const int* starts_x, int nx, ru_stream_t stream);
/* Case preparation (test.py:47-49,85-120).  ru_case_bbox: box[c*6 .. c*6+5] (DEVICE ints) = {min z, y, x, max z, y, x} of the non-zero
 * voxels of modality c of image [C][D][H][W]; {INT_MAX x3, -1 x3} for an all-zero modality (the host applies test.py:47-49's union and
 * its rule for empty modalities).  ru_case_stats: per channel over the crop box [lo, lo + size): stats[c*3..] = count(x > 0), sum x,
 * sum x^2 (float64, DEVICE).  ru_case_prepare: batch [K][C][padded] = the K test-time flips (3 bits per copy, bit0 D, bit1 H, bit2 W,
 * as ru_tta_merge) of the crop zero-padded by pad_left to `padded` and z-scored with the moments in `stats` -- every voxel,
 * padding included, (x - mean) / std in float64 as the reference's numpy does (test.py:103-113).  lo / size / pad_left / padded: HOST.  */
int ru_case_bbox(const float* image, int* box, int C, int D, int H, int W, ru_stream_t stream);
size_t ru_case_workspace_bytes(int C, int D, int H, int W);
int ru_case_stats(const float* image, double* stats, int C, int D, int H, int W, const int* lo, const int* size,
                  void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_case_prepare(const float* image, const double* stats, float* batch, int C, int D, int H, int W, const int* lo, const int* size,
                    const int* pad_left, const int* padded, int K, unsigned flips, ru_stream_t stream);
/* ru_tta_merge restricted to the box [lo, lo + size) of the padded prediction (test.py:140-144 removes the padding before the masks are
 * counted): mean_out / mask are [C][size], counts[C] the voxels set inside the box.  It is ru_ens_accumulate_finalize(first = 1, M = 1)
 * and shares its kernel (csrc/ensemble.hip) and its refusals: D*H*W >= INT_MAX ("volume too large for 32-bit voxel indices"), and C > 65535
 * is RU_EINVAL ("bad argument") before any launch, where the launch itself used to fail.  */
int ru_tta_merge_box(const float* probs, int K, unsigned flips, float* mean_out, unsigned char* mask, unsigned long long* counts,
                     int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream);
/* Post-processing (test.py:51-62,162-164): 26-connected components of labels > 0 by union-find on the device, every component smaller
 * than ratio * (V - size of the most frequent label, background included) is zeroed in place.  Only component sizes enter the rule, so
 * the result equals skimage.morphology.label + reject_small_regions whatever the numbering.  ru_paste_labels (test.py:167-168):
 * full [D][H][W] = 0 outside the box, lab [size] inside: ru_paste_u8c with one channel (csrc/ensemble.hip, 32-bit voxel indices:
 * D*H*W >= INT_MAX is refused with "volume too large for 32-bit voxel indices").  */
size_t ru_cc_workspace_bytes(int D, int H, int W);
int ru_cc_reject(unsigned char* labels, int D, int H, int W, double ratio, void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_paste_labels(const unsigned char* lab, unsigned char* full, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream);

/* ---------------------------------------------------------------- region-wise post-processing (csrc/postprocess.hip)
 * Between ru_tta_merge_box / the ensemble finalize and ru_compose_labels.  Per region k of R_0 = WT, R_1 = TC, R_2 = ET on a grid [D][H][W]
 * (D * H * W < 2^31), in this order (INTEGRATION.md states the same with its reasons):
 *   1. the 26-connected components of R_k (scipy.ndimage.label with a 3 x 3 x 3 structure of ones; ru_cc_reject's connectivity);
 *   2. per component vol = its voxels and, with probabilities, conf = the sum over its voxels of q(p) = (uint32) floor(clamp(p, 0, 1) *
 *      65536.0f) -- an exact float32 product, truncated -- in 64-bit integers;
 *   3. a component is removed if vol < min_volume[k]; or if conf_thr[k] > 0 and conf < conf_thr[k] * vol (integers; conf_thr[k] = T_k =
 *      floor(min_confidence[k] * 65536.0) formed by the caller, <= 65536); or if bit k of keep_largest_bits is set and it is not the
 *      component of largest vol among the survivors of the two rules, ties to the one holding the smallest linear voxel index;
 *   4. bit k of fill_holes_bits: every 6-connected component of the background of the filtered mask that touches no face of the grid
 *      becomes foreground (scipy.ndimage.binary_fill_holes, default structure; an extent of 1 leaves no holes);
 *   5. nest != 0: R_1 &= R_0, then R_2 &= R_1.
 * kind RU_POSTPROCESS_MASKS:  in = uint8 [3][D][H][W], non-zero = foreground; probs = float32 [3][D][H][W] or NULL (then every conf_thr
 *                             must be 0); out = uint8 [3][D][H][W] of 0 / 1.
 * kind RU_POSTPROCESS_LABELS: in = uint8 [D][H][W] BraTS labels, regions as ru_surface_metrics (WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4};
 *                             above 4: background); probs NULL; out = uint8 [D][H][W]: 2 where WT, 1 where TC, 4 where ET, in that order.
 * counts [3] uint64 = the voxels of the three output regions (what ru_compose_labels takes).  stats [3][RU_POSTPROCESS_STATS] int64 =
 * {components found, removed by volume, removed by confidence only, removed by keep_largest, voxels filled, invalid label voxels
 * (kind LABELS: bytes above 4, the same in every row; 0 otherwise)}.  `in` is not written and must not be `out`.  Integer atomics only:
 * two calls give identical bytes.  The call only enqueues; ws: ru_postprocess_workspace_bytes(kind, D, H, W) bytes (0 for a bad kind or
 * shape).  min_volume, conf_thr: HOST arrays of 3. */
#define RU_POSTPROCESS_MASKS 0
#define RU_POSTPROCESS_LABELS 1
#define RU_POSTPROCESS_REGIONS 3
#define RU_POSTPROCESS_STATS 6
#define RU_POSTPROCESS_S_FOUND 0
#define RU_POSTPROCESS_S_VOLUME 1
#define RU_POSTPROCESS_S_CONFIDENCE 2
#define RU_POSTPROCESS_S_LARGEST 3
#define RU_POSTPROCESS_S_FILLED 4
#define RU_POSTPROCESS_S_INVALID 5
size_t ru_postprocess_workspace_bytes(int kind, int D, int H, int W);
int ru_postprocess_regions(const void* in, const float* probs, int kind, int D, int H, int W, const long long* min_volume,
                           const unsigned long long* conf_thr, unsigned keep_largest_bits, unsigned fill_holes_bits, int nest,
                           unsigned char* out, unsigned long long* counts, long long* stats, void* ws, size_t ws_bytes, ru_stream_t stream);

/* ---------------------------------------------------------------- ensemble inference and soft labels (csrc/ensemble.hip)
 * The reference's ensemble step (README.md:1-5; average_predicts.ipynb / emsemble_predicts.ipynb: `sum(data_files) / len(data_files)`,
 * argmax, 3 -> 4) with the models' predictions resident on the device.  Fixed float32 arithmetic, comparable bit for bit with numpy:
 *   per model  p_m = (((o0 + o1) + o2) + o3) / K, un-flipped, on the box [lo, lo + size) -- ru_tta_merge_box's mean (test.py:134-144);
 *   across models  S_1 = p_1, S_m = S_(m-1) + p_m in call order;  mean = S_M / (float)M by a true division.
 * ru_ens_accumulate: one pass per model over probs [K][C][D][H][W]; acc [C][size] takes S_m (first != 0: written, not read -- no memset).
 *   K = 1, flips = 0 and the box equal to the volume accumulates an already merged prediction (a saved file).
 * ru_ens_finalize: mean_out (may be NULL) = acc / M, mask = mean > 0.5 (test.py:144), counts[C] = exact voxels set per channel.
 * ru_ens_accumulate_finalize: the LAST model's accumulate and the finalize in one pass (acc is read, not written; NULL when first != 0,
 *   i.e. an ensemble of one, which is ru_tta_merge_box); identical results.
 * ru_ens_argmax: the notebooks' class rule on acc [C][V] of saved class maps: argmax over c of acc / M (first maximum wins, as np.argmax),
 *   class 3 written as 4, uint8.
 * ru_paste_probs: the soft labels in the case's own frame: full [C][D][H][W] = 0 outside the box, mean [C][size] inside (test.py:167-168). */
int ru_ens_accumulate(const float* probs, int K, unsigned flips, float* acc, int first, int C, int D, int H, int W, const int* lo, const int* size,
                      ru_stream_t stream);
int ru_ens_finalize(const float* acc, int M, float* mean_out, unsigned char* mask, unsigned long long* counts, int C, size_t Vbox, ru_stream_t stream);
int ru_ens_accumulate_finalize(const float* probs, int K, unsigned flips, const float* acc, int first, int M, float* mean_out, unsigned char* mask,
                               unsigned long long* counts, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream);
int ru_ens_argmax(const float* acc, int M, unsigned char* labels, int C, size_t V, ru_stream_t stream);
int ru_paste_probs(const float* mean, float* full, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream);

/* ---------------------------------------------------------------- uncertainty maps and the BraTS uncertainty score (csrc/uncertainty.hip)
 * BraTS 2019's third task: per case three uint8 maps (WT, TC, ET; 0 = certain .. 100 = uncertain) beside the label map.  The samples are
 * the M x K un-flipped predictions o[m][k] an ensemble forms anyway, on the box [lo, lo + size); `mean` is ru_ens_*'s float32 mean.
 *   second moment, float32, every product and sum rounded (no fma):  q_m = ((o0*o0 + o1*o1) + o2*o2) + o3*o3;  T_1 = q_1, T_m = T_(m-1) + q_m
 *   RU_UNC_STD      e2 = (double)T_M / (double)(M*K), mu = (double)mean, var = max(e2 - mu*mu, 0), u = floor(min(200*sqrt(var), 100) + 0.5):
 *                   IEEE + - * / sqrt only, no contraction -- equal to numpy exactly
 *   RU_UNC_ENTROPY  H = -(mu*log2(mu) + (1-mu)*log2(1-mu)), a term is 0 unless its argument lies inside (0, 1); u = floor(100*H + 0.5)
 *                   (the device's log2 may differ from numpy's in the last place)
 * ru_unc_accumulate: ru_ens_accumulate plus acc2 [C][size] <- T_m in the same pass over probs; acc is bit-identical to ru_ens_accumulate's.
 *   first != 0: both buffers are written, not read (no memset).
 * ru_unc_accumulate_finalize: the LAST model's accumulate and the finalize in one pass, as ru_ens_accumulate_finalize (same mean_out, mask,
 *   counts, bit for bit), plus unc [C][size] uint8.  acc / acc2 are read, not written; both may be NULL when first != 0, acc2 also with
 *   RU_UNC_ENTROPY.
 * ru_unc_finalize: the same from stored sums of M members-of-K (saved predictions: K = 1); acc2 may be NULL with RU_UNC_ENTROPY.
 * ru_unc_histogram: pred, target = uint8 label volumes [D][H][W] with values {0,1,2,3,4}, unc = uint8 [3][D][H][W] -> hist [3][101][4] =
 *   exact voxel counts per region (WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4}), map value and class {RU_UNC_TP, _FP, _FN, _TN}; invalid[0] = voxels
 *   with a label outside 0..4 or a map value above 100 (they are in no bin).  Both outputs are written, not accumulated.
 * ru_unc_score: from hist and T strictly rising thresholds (HOST array, values 0..100, T <= 101), filtering out the voxels whose map value
 *   exceeds the threshold t:  Dice_t = 2TP/(2TP+FP+FN) (1 for an empty denominator), FTP_t = (TP_100 - TP_t)/TP_100 (0 for TP_100 = 0), FTN_t
 *   likewise; AUC = trapezoid rule / (t_last - t_first) (T = 1: the curve's value); out [3][4] = {score = (AUC_Dice + (1 - AUC_FTP) +
 *   (1 - AUC_FTN)) / 3, AUC_Dice, AUC_FTP, AUC_FTN} in float64; acc [3][4] (may be NULL) += out: the running sum over the cases.  Neither
 *   the empty-denominator values nor any threshold list have been checked against the challenge's evaluator.
 * ru_paste_u8c: ru_paste_labels for C channels: full [C][D][H][W] = 0 outside the box, src [C][size] inside. */
#define RU_UNC_STD 0
#define RU_UNC_ENTROPY 1
#define RU_UNC_TP 0
#define RU_UNC_FP 1
#define RU_UNC_FN 2
#define RU_UNC_TN 3
int ru_unc_accumulate(const float* probs, int K, unsigned flips, float* acc, float* acc2, int first, int C, int D, int H, int W, const int* lo,
                      const int* size, ru_stream_t stream);
int ru_unc_accumulate_finalize(const float* probs, int K, unsigned flips, const float* acc, const float* acc2, int first, int M, int measure,
                               float* mean_out, unsigned char* mask, unsigned long long* counts, unsigned char* unc, int C, int D, int H, int W,
                               const int* lo, const int* size, ru_stream_t stream);
int ru_unc_finalize(const float* acc, const float* acc2, int M, int K, int measure, float* mean_out, unsigned char* mask, unsigned long long* counts,
                    unsigned char* unc, int C, size_t Vbox, ru_stream_t stream);
int ru_unc_histogram(const unsigned char* pred, const unsigned char* target, const unsigned char* unc, int D, int H, int W, unsigned long long* hist,
                     unsigned long long* invalid, ru_stream_t stream);
int ru_unc_score(const unsigned long long* hist, const int* thresholds, int T, double* out, double* acc, ru_stream_t stream);
int ru_paste_u8c(const unsigned char* src, unsigned char* full, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream);

/* ---------------------------------------------------------------- voxel-major working layout ("C16")
 * Between the first and the last convolution the split-bf16 engine keeps activations as [N][C/16][D][H][W][16]
 * (16 channels of a voxel contiguous; C % 16 == 0): a halo tile of a 3x3x3 convolution is then a few long contiguous
 * runs instead of 16 channel planes x short rows.  Nothing in that layout crosses the boundary of ru_unet_*; the
 * entry points below exist so the tests and probes can drive the layout-aware kernels one at a time.
 * flags: bit 0 = x (input) is C16, bit 1 = y (output) is C16, bit 2 = x is NCDHW with Cin <= 4 and goes through the 4-channel
 * tap-pair kernel (needs extra workspace: 16 bytes per input voxel); bit 3 = x is voxel-major in SPLIT form (hi / lo bf16 packets); bit 4 = exact-f32
 * arithmetic (v_mfma_f32_16x16x4_f32 on voxel-major tensors: the exact-f32 inference forward of the engine; not with bits 2 / 3); bit 5 = x is an
 * ACTIVATION tensor (a forward convolution, model.py:72-73): shapes that have the kernel (16 input channels, voxel-major both sides, a grid that fills the
 * chip) take the fp16 + MX-fp8 product scheme the engine's forward convolutions take (f16*f16 + two e4m3 cross terms, RU_MX=0: off); never set for gradients;
 * bit 6 = x (float32, voxel-major both sides, 16 -> 16 channels) is a GRADIENT: where the kernel takes the shape it is converted to the gradient-operand form (bf16 + two
 * e4m3 planes + one exponent byte per voxel) and convolved with bf16 main + MX-fp8 cross products, as the engine's 16-channel data-gradient convolutions are (RU_MXG=0:
 * off; needs 64 more workspace bytes per input voxel); ignored elsewhere; bit 7 = pack `w` as a training step packs it instead of in every form: the fragment
 * forms the RU_* switches of the process launch, and no direct fragments where a forward convolution of this shape and these layouts (bits 0, 1, 5; no fused
 * residual / bias operand) takes a Winograd-z or fp16 + MX-fp8 kernel.  The launch itself is unchanged; if its route reads a form that pack does not hold -- a
 * residual `add` keeps a launch of such a shape on the direct kernel -- it is refused with RU_EINVAL before anything of the convolution is launched.  k = 3.
 * ru_conv3d_fwd_l is ru_conv3_l (below) with weight_mode 0 and no fused operands or reports: ru_conv3_l_workspace_bytes(..., flags) sizes it for any flags,
 * ru_conv3d_workspace_bytes(..., 3) for flags without bits 2 and 6. */
int ru_layout_convert(const float* src, float* dst, int N, int C, size_t V, int to_c16, ru_stream_t stream);
int ru_conv3d_fwd_l(const float* x, const float* w, const float* bias, float* y,
                    int N, int Cin, int Cout, int D, int H, int W, int flags,
                    void* ws, size_t ws_bytes, ru_stream_t stream);
/* weight gradient; flags: bit 0 = x is C16, bit 1 = dy is C16.  ws: ru_conv3d_workspace_bytes(..., 3) */
int ru_conv3d_bwd_weight_l(const float* x, const float* dy, float* dw,
                           int N, int Cin, int Cout, int D, int H, int W, int flags,
                           void* ws, size_t ws_bytes, ru_stream_t stream);

/* The voxel-major pointwise family, one launch at a time (all tensors C16).
 * ru_conv1_l: y[v][o] = lrelu_out_slope( sum_c w[o][c] * cat(x0, x1)[v][c] ), then the LeakyReLU-backward mask (y * (mask > 0 ? 1 : mask_slope)), then + add.
 *   s2d = 0: w is [Cout][ldw] (ldw >= C0 + C1, a multiple of 4); x1 / C1 optional (a channel concat that is never made); y1 / Cout0 optional: output
 *            channels Cout0.. go to y1, and the mask then applies to (and is laid out like) y1 only.
 *   s2d = 1: the 2x2x2 stride-2 convolution read straight from the FINE tensor x0 (C0 / 8 channels, extents 2Dc x 2Hc x 2Wc), V = Dc*Hc*Wc coarse voxels;
 *            w is the reference's [Cout][C0/8][2][2][2] and is packed here (ldw is ignored).
 *   s2d = 2: its transpose written straight into the FINE tensor y (Cout / 8 channels); w is the reference's [C0][Cout/8][2][2][2] (ldw is ignored).
 *   bst_y / bst_k[N][3][C] (k1, k2, thr) / bst_slope (optional; plain and scatter modes): the GroupNorm-backward sums of the stored output d,
 *            u = bst_y*k1 + k2, dh = u > thr ? d : d*bst_slope, S1 = sum dh, S2' = sum dh*u, as partials [N][C][*nblk][2] in stat_partials (capacity stat_floats);
 *            *nblk = 0 where the shape has no fused form (the launch is then refused).
 *   *inst (optional): the kernel instantiation taken, COB | S2D << 4 | NSLOT << 8 | PAIR << 12.
 * ru_wgrad1_l: dw[o*ldw + c] = sum_{n,v} dy[n][v][o] * x[n][v][c]; c16 = 0: NCDHW operands.  x1 / C0: input channels C0.. live in x1.  s2d = 1: x is the FINE tensor
 *   of a stride-2 conv (Cin = 8 x its channels, channel tap*(Cin/8) + c at fine voxel (2z+i, 2y+j, 2x+k), tap = 4i + 2j + k); tap_split = Cin/8 writes
 *   dw[o*ldw + c*8 + tap], the reference's [Cout][Cin/8][2][2][2].  dg_w (optional, [Cout][dg_ldw], Cout <= 32): the data gradient in the same pass,
 *   dx[v][c] = sum_o dg_w[o][c] * dy[v][o], channels < C0 (or all) to dg_y0, the others to dg_y1 times (x1 > 0 ? 1 : dg_mask_slope).
 *   *inst (optional): OT | CT << 4 of wgrad1_f32_kernel<OT, CT>, bit 8 = the stride-2 kernel instead, bit 9 = fused data gradient.
 * ru_conv1_l_workspace_bytes / ru_wgrad1_l_workspace_bytes: the dry walk of ru_conv1_l (both packs of the 2x2x2 weight with s2d, nothing without) /
 *   of ru_wgrad1_l (the partials), plus 4096. */
size_t ru_conv1_l_workspace_bytes(int C0, int Cout, int s2d);
int ru_conv1_l(const float* x0, int C0, const float* x1, int C1, const float* w, int ldw, float* y, float* y1, int Cout0,
               const float* add, float out_slope, const float* mask, float mask_slope, int N, int Cout, size_t V,
               int s2d, int Dc, int Hc, int Wc, const float* bst_y, const float* bst_k, float bst_slope,
               float* stat_partials, size_t stat_floats, int* nblk, int* inst, void* ws, size_t ws_bytes, ru_stream_t stream);
/* The 3x3x3 family, one launch at a time with the operands the engine fuses into it (flags as ru_conv3d_fwd_l; x / y / add / bst_y / in_res / in_sum_out in the layouts the
 * flags name, in_res / in_sum_out always voxel-major like x):
 *   y = act( conv3( pad0( lrelu(x*in_scale[n][c] + in_shift[n][c], in_slope) + in_res ), w ) + bias + add ),  act = sigmoid or none; in_scale null: no transform.
 *   in_sum_out (with in_res): the staged sum before the padding, every voxel written once.
 *   stat_partials [N][Cout][*nblk][2] (capacity stat_floats): per-workgroup (sum, sumsq) of the value after `add` and before the sigmoid; with bst_y / bst_k[N][3][Cout] /
 *   bst_slope instead the GroupNorm-backward sums of that value d: u = bst_y*k1 + k2, dh = u > thr ? d : d*bst_slope, S1 = sum dh, S2' = sum dh*u.
 *   products: 0 / 3 = three split-bf16 products, 1 = one bf16 product (gradient precision), 2 = x is an activation tensor (same as flag bit 5).
 *   weight_mode 0: w = [Cout][Cin][3][3][3]; 1: w = [Cin][Cout][3][3][3] is the weight of the FORWARD convolution whose data gradient this launch computes
 *   (channels swapped, taps mirrored in the packing).
 *   *route (optional): the kernel taken -- family (1 one-stage sb, 2 persistent sb2, 3 sb2c4, 4 wz32, 5 wz32mx, 6 mx, 7 f32c; 8 wz16, the
 *   16x16 Winograd-z kernel, which only a build with the developer switch RU_SB2_DBG can route to) | TZ << 4 | TY << 8 | IN16 << 12 |
 *   OUT16 << 13 | MULTI << 14 | BST << 15 | ADD << 16 | HEAD << 17 | GRAD << 18 | products per operand pair << 20.
 *   fin (optional; needs stat_partials): the launch's LAST workgroup finalizes the partials it published (the engine's RU_FUSE_TAIL_FINALIZE), see ru_fin_desc.
 *   The ticket is a word of the workspace, zeroed on the stream before the launch.  Null: no tail.  Split-K is not reachable from here.
 * ru_conv3_l_workspace_bytes(..., flags): the dry walk of ru_conv3_l (and of ru_conv3d_fwd_l) for these flags with bias == NULL and weight_mode 0, under the
 * RU_* switches of the calling process, plus 4096 -- the weight fragments, the 4-channel copy and its fragments (bit 2), the gradient-operand tensor (bit 6,
 * where the shape and RU_MXG take it; a bias turns that form off and needs no more); bit 8 (the query's alone): a ru_fin_desc will be passed (the ticket). */
/* What a kernel's in-launch tail finalizes, and where to (fin_tail.hpp).  kind 1: (sum, sumsq) partials -> mean / rstd [N][G], scale / shift [N][C] and, optionally,
 * bst_k [N][3][C] -- what ru_gn_finalize_l writes.  kind 2: GroupNorm-backward sums -> coef [N][C][3], dgamma / dbeta [C] -- what ru_gn_bwd_finalize_l writes --
 * from the INPUTS mean / rstd [N][G]; s2_sign as there.  nblk / N / C: 0 = the launch's own; another value is handed to the launcher as it is (which refuses a
 * descriptor that does not match its grid).  keep_ticket: the workspace is the one a previous call of the same shape left, and its ticket word is NOT zeroed. */
typedef struct ru_fin_desc {
    int kind, G, s2_sign, keep_ticket;
    float eps;
    int nblk, N, C;
    const float* gamma;
    const float* beta;
    float* mean;
    float* rstd;
    float* scale;
    float* shift;
    float* bst_k;
    float* coef;
    float* dgamma;
    float* dbeta;
} ru_fin_desc;
size_t ru_conv3_l_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int flags);
int ru_conv3_l(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int flags, int weight_mode,
               const float* add, const float* in_scale, const float* in_shift, float in_slope, const float* in_res, float* in_sum_out,
               int sigmoid, int products, const float* bst_y, const float* bst_k, float bst_slope, float* stat_partials, size_t stat_floats,
               int* nblk, int* route, void* ws, size_t ws_bytes, ru_stream_t stream, const ru_fin_desc* fin);

/* The voxel-major GroupNorm chain, one link at a time (G groups, C % G == 0; x / res / dact / dx voxel-major [N][C/16][V][16]).
 * ru_gn_finalize_l: partials [N][C][nblk][2] -> mean / rstd [N][G], scale / shift [N][C] (y = x*scale + shift), bst_k [N][3][C] (optional) = (sign(gamma)*rstd,
 *   -sign(gamma)*mean*rstd, -beta/|gamma|; gamma == 0: -inf where beta > 0, else +inf).  centred = 0: (sum, sumsq) pairs; 1: the (sum, M2) pairs of the NCDHW statistics pass.
 * ru_gn_apply_l: y = res' + lrelu(x*scale[n][c] + shift[n][c], slope); res' = nothing (res null), res, or lrelu(res*res_scale + res_shift, res_slope).
 * ru_gn_bwd_finalize_l: partials [N][C][nblk][2] of (S1 = sum dh, S2 = sum dh*xhat; s2_sign = 1: S2 carries sign(gamma)) -> coef [N][C][3] (dx = cA*dh + cB*x + cC),
 *   dgamma / dbeta [C].
 * ru_gn_bwd_l: the chain of one GroupNorm backward -- the reduction over (x, dact), its finalize (flags bit 0: in the reduction's tail, else the separate launch),
 *   the apply to dx (bit 1: in split form; bit 2: no apply, dx may be null).  bit 3: the ticket word of the workspace is not zeroed (see ru_fin_desc).  coef_out
 *   [N][C][3] / partials_out [N][C][nblk][2], nblk = ru_gn_bwd_l_nblk(V) (optional): copies of what the chain left in the workspace.
 *   ru_gn_bwd_l_workspace_bytes: its dry walk (partials, coef, ticket) plus 4096. */
int ru_gn_finalize_l(const float* partials, int nblk, const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift, float* bst_k,
                     int N, int C, size_t V, int G, float eps, int centred, ru_stream_t stream);
int ru_gn_apply_l(const float* x, const float* scale, const float* shift, const float* res, const float* res_scale, const float* res_shift, float* y,
                  int N, int C, size_t V, float slope, float res_slope, ru_stream_t stream);
int ru_gn_bwd_finalize_l(const float* partials, int nblk, const float* gamma, const float* mean, const float* rstd, float* coef, float* dgamma, float* dbeta,
                         int N, int C, size_t V, int G, int s2_sign, ru_stream_t stream);
int ru_gn_bwd_l_nblk(size_t V);
size_t ru_gn_bwd_l_workspace_bytes(int N, int C, size_t V);
int ru_gn_bwd_l(const float* x, const float* dact, const float* gamma, const float* scale, const float* shift, const float* mean, const float* rstd, float slope,
                float* dx, float* dgamma, float* dbeta, float* coef_out, float* partials_out, int N, int C, size_t V, int G, int flags,
                void* ws, size_t ws_bytes, ru_stream_t stream);
/* The head of the backward pass, one route of ru_unet_backward at a time: p [N][C][V] (the probabilities) and the gradient w.r.t. them -> d = dp*p*(1-p)
 * (model.py:431) as d4 [N][V][4] (voxel-major, channels C..3 written as +0) and / or dlog [N][C][V], and db [C] = sum over n, v of d (model.py:348).
 *   route 0: the 4-channel pass (1..4 channels, V % 4 == 0); dlog (optional) by the flat sigmoid backward behind it.
 *   route 1: the same pass with dp = ru_criterion_grad(p, target, sums, count, w_dice, w_bce, bg_weight, priority) formed in registers (dp not read, dlog null).
 *   route 2: the flat sigmoid backward into dlog, then the bias gradient over it (any C and V; d4 not written, may be null).
 * ru_head_grad_l_workspace_bytes: its dry walk (the bias partials) plus 4096. */
size_t ru_head_grad_l_workspace_bytes(int N, int C, size_t V, int route);
int ru_head_grad_l(const float* p, const float* dp, const float* target, const double* sums, double count, float w_dice, float w_bce, float bg_weight,
                   float priority, float* d4, float* db, float* dlog, int N, int C, size_t V, int route, void* ws, size_t ws_bytes, ru_stream_t stream);
size_t ru_wgrad1_l_workspace_bytes(int N, int Cin, int Cout, size_t V);
int ru_wgrad1_l(const float* x, const float* x1, int C0, const float* dy, float* dw, int ldw, int N, int Cin, int Cout, size_t V,
                int c16, int s2d, int Dc, int Hc, int Wc, int tap_split, const float* dg_w, int dg_ldw, float* dg_y0, float* dg_y1,
                float dg_mask_slope, int* inst, void* ws, size_t ws_bytes, ru_stream_t stream);
/* The transpose-read 3x3x3 weight gradient (both operands voxel-major, Cin and Cout multiples of 16), one launch at a time with the operands the engine fuses into it:
 *   dw[o][c][tap] = sum_{n,v} dy[n][v][o] * pad0( lrelu(x*in_scale[n][c] + in_shift[n][c], in_slope) )[n][v + tap][c];  in_scale null: no transform.
 *   flags: 1 = dy is in split form (64 bytes per voxel and block: bf16 hi ch 0-7 | hi ch 8-15 | lo ch 0-7 | lo ch 8-15);
 *          2 = x is NCDHW with dw_cin <= 4 channels and stands for one 16-channel block (Cin = 16): the 4-channel copy is made in the workspace and its three
 *              dx taps are packed into the block's columns;  4 = dy is NCDHW with dw_cout <= 4 channels (Cout = 16), likewise copied;
 *          8 = swapped: x (with its halo) is the convolution's OUTPUT gradient and dy its input; dw is then [dw_cin][dw_cout][27] = the convolution's
 *              [Cout_conv][Cin_conv][27], taps mirrored by the reduction;
 *          16 = gb_out is published in the gradient-operand form (bf16 hi ch 0-7 | hi ch 8-15 | e4m3 lo / 2^(e-8), e4m3 value / 2^e ch 0-7 | the same ch 8-15)
 *              instead of the split form;  32 = the reduction of the partials runs deferred (queued, then flushed as one batch launch): same result.
 *   products: 0 / 3 = three split-bf16 products, 1 = one bf16 product where such a kernel exists.
 *   dw_cin / dw_cout (0 = Cin / Cout): the real channel counts dw is truncated to; dw is [dw_cout][dw_cin][27].
 *   gb_y (optional; dy may then be null): the dy operand is the GroupNorm-backward apply formed in the staging from the forward tensor gb_y and the gradient
 *   gb_d (voxel-major), gb_scale / gb_shift [N][Cout], gb_coef [N][Cout][3] and gb_slope,
 *       dy = cA * ((y*scale + shift) > 0 ? d : d*slope) + (cB*y + cC),
 *   and is written to gb_out (voxel-major, 64 bytes per voxel and block; may be null with flag 2 only) in the form flag 16 names.
 *   *inst (optional): the instantiation taken, OT | XS << 4 | DS << 8 | NP << 12 of wgrad3_tz_kernel<OT, XS, DS, NP>; negative: the launch is refused.
 * ru_wgrad3_l_workspace_bytes(..., flags): the dry walk of ru_wgrad3_l, plus 4096 -- the partials and one 4-channel copy each for flags 2 and 4 (the other
 *   flags take nothing). */
size_t ru_wgrad3_l_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int flags);
int ru_wgrad3_l(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int D, int H, int W, int flags, int products,
                const float* in_scale, const float* in_shift, float in_slope, int dw_cin, int dw_cout,
                const float* gb_y, const float* gb_d, const float* gb_scale, const float* gb_shift, const float* gb_coef, float gb_slope, float* gb_out,
                int* inst, void* ws, size_t ws_bytes, ru_stream_t stream);

/* trilinear x2 and its transpose on C16 tensors (C % 16 == 0; D,H,W = extents of the COARSE side, as in
 * ru_upsample2x_trilinear_*).  out_slope: LeakyReLU slope applied to the interpolated value (the decoder fuses model.py:401-402
 * into the up-sampling; 1 = none). */
int ru_upsample2x_trilinear_fwd_l(const float* x, float* y, int N, int C, int D, int H, int W, float out_slope, ru_stream_t stream);
int ru_upsample2x_trilinear_bwd_l(const float* dy, float* dx, int N, int C, int D, int H, int W, ru_stream_t stream);

/* ---------------------------------------------------------------- evaluation metric (metrics.py:108-133, `Dice.update`)
 * counts[(n*C + c)*2 + {0,1}] = { #(p > 0.5 and g > 0.5), #(p > 0.5) + #(g > 0.5) } over the V voxels of sample n, channel c.
 * The metric is 2*counts[0]/counts[1] per (n, c) (NaN -> 1), averaged over the batch (host side: brats2019_amd/metrics.py). */
int ru_dice_counts(const float* p, const float* g, unsigned long long* counts, int N, int C, size_t V, ru_stream_t stream);
/* The rest of `Dice.update` (metrics.py:124-130) on the device: acc[c] += mean over the N samples of r(n, c), r = 2*counts[0]/counts[1] formed
 * in float32 like the reference's numpy line (0/0 -> NaN -> 1), the mean and the accumulator in float64; c < nacc (= classes - 1 <= C). */
int ru_dice_accumulate(const unsigned long long* counts, double* acc, int N, int C, int nacc, ru_stream_t stream);

/* ---------------------------------------------------------------- evaluation metric (metrics.py:188-271, `Hausdorff_ITK` / `Hausdorff_ITKWT`)
 * Exact squared Euclidean distances between voxel centres (unit spacing on D, H, W), every extent in [1, 512] (larger: RU_EINVAL).
 * p, g: [N][C][D][H][W] float32.  mode 0: K = C masks per sample, x > 0.5 per channel; mode 1: K = 1 mask, argmax over C > 0 (the
 * first of equal maxima wins, so: max(x[1:]) > x[0]).
 * out[(n*K + k)*4 + {0,1,2,3}] = { max over P of d^2 to G, max over G of d^2 to P, #P, #G } as exact integers (a directed maximum is
 * meaningless when either count is 0).  ws: ru_hausdorff_workspace_bytes(N, C, D, H, W, mode) bytes (8 per voxel and mask). */
size_t ru_hausdorff_workspace_bytes(int N, int C, int D, int H, int W, int mode);
int ru_hausdorff_sq(const float* p, const float* g, int N, int C, int D, int H, int W, int mode, unsigned long long* out,
                    void* ws, size_t ws_bytes, ru_stream_t stream);
/* The rest of the metric's `update` on the device: result[n, i] for i < nacc (<= K) as the reference's loop fills it -- HD = sqrt of the
 * larger squared maximum in float64, 1e6 when one mask is empty (ITK raises, the reference stores 1e+6); mode 0 only: both masks of
 * channel i empty writes 0 to column i-1 (the reference's index slip, kept) and leaves column i at 0; mode 1: both empty -> 1e6 -- then
 * acc[i] += mean over the N samples (float64). */
int ru_hausdorff_accumulate(const unsigned long long* sq, double* acc, int N, int K, int nacc, int mode, ru_stream_t stream);

/* ---------------------------------------------------------------- evaluation metrics (metrics.py:22-185: `Dice1D`, `RMSE`, `DiceWT`, `Dice_ITK`;
 * validate.py).  Label overlaps come from one per-sample confusion matrix of exact integer counts.
 *   ru_label_confusion : conf[(n*L + a)*L + b] = #voxels of sample n with prediction label a and target label b (uint64), one pass that
 *                        reads each input once; any V >= 1.  kind RU_CONF_PROB: pred, target = [N][C][V] float32, L = C in
 *                        1..RU_OVERLAP_MAX_LABELS (more: RU_EINVAL), label = argmax over C with torch's rules (the first of equal maxima,
 *                        a NaN is the maximum and the first NaN wins); `invalid` may be NULL.  kind RU_CONF_LABEL: pred, target = [N][V]
 *                        uint8 label volumes, C = 1, L = 4, label 4 counts as 3 (validate.py:70); a voxel where either value is outside
 *                        0..4 goes into invalid[n] (required) and into no bin.  conf and invalid are cleared by a kernel of the same call.
 *   ru_overlap_accumulate : one launch from conf [N][L][L]; `out` (float64 [N][nacc]) receives the per-sample values when non-NULL.
 *     RU_OVERLAP_ITK (Dice_ITK): column i-1 for label i = 1..nacc (<= 64): J = I/(P+G-I), dice = 2J/(1+J) in float64 (ITK's
 *                        LabelOverlapMeasuresImageFilter: mean overlap from the union overlap of the one non-zero label of two binary
 *                        images).  A label absent from both images (both counts 0, or i >= L) gives RU_OVERLAP_BOTH_EMPTY = NaN.  That
 *                        value was NOT checked against SimpleITK, whose versions differ there.  acc[i-1] += batch mean.
 *     RU_OVERLAP_WT (DiceWT): nacc = 1, labels > 0 on both sides: r = 2*I / (S + 1e-6) in float32 (both empty: 0), acc[0] += batch mean.
 *     RU_OVERLAP_VALIDATE (validate.py): L = 4, nacc = 4, out required: per sample [d1, d2, d3, dWT], r = 2*num/den of the
 *                        float32-rounded counts in float32, NaN -> 1; acc[k] += the SUM over the N samples (a running sum over cases).
 *   ru_dice1d_accumulate : from ru_dice_counts' counts [N][C][2] = {I, |P|+|G|}: acc[c] += batch mean of 2*I / (S + 1e-6) formed in
 *                        float32, c < classes (<= C, <= 64) (metrics.py:41-50).
 *   ru_rmse_accumulate   : acc[0] += sqrt(sums[0] / sums[1]) in float64, sums = {sum (p-g)^2, count} on the device (metrics.py:66-71;
 *                        the sum is ru_crit_moments' RU_CRIT_M_D2 moment of the tensor taken as one row). */
#define RU_CONF_PROB 0
#define RU_CONF_LABEL 1
#define RU_OVERLAP_MAX_LABELS 8
#define RU_OVERLAP_ITK 0
#define RU_OVERLAP_WT 1
#define RU_OVERLAP_VALIDATE 2
int ru_label_confusion(const void* pred, const void* target, int kind, int N, int C, size_t V, unsigned long long* conf,
                       unsigned long long* invalid, ru_stream_t stream);
int ru_overlap_accumulate(const unsigned long long* conf, int N, int L, int mode, int nacc, double* acc, double* out, ru_stream_t stream);
int ru_dice1d_accumulate(const unsigned long long* counts, double* acc, int N, int C, int classes, ru_stream_t stream);
int ru_rmse_accumulate(const double* sums, double* acc, ru_stream_t stream);

/* ---------------------------------------------------------------- calibration scoring and the per-region threshold search (csrc/calibration.hip)
 * One integer pass over (probability, target) that bins the probability; the Dice / sensitivity / specificity curve at every threshold and
 * the calibration numbers are small functions of its tables.  Opt-in: nothing else calls these.  The conventions are this library's own and
 * were not checked against any other package.
 *   NB        fine bins: a power of two, RU_CALIB_MIN_NB <= NB <= RU_CALIB_MAX_NB.  p * NB is exact in float32 and b / NB is representable.
 *   valid     a probability p (float32) is valid iff 0 <= p <= 1; -0.0 is valid, NaN, negatives, values above 1 and infinities are not.
 *   k(p)      = ceil(p * NB) in 0..NB: NB + 1 bins, bin 0 holds exactly p == 0, and p > b / NB <=> k(p) > b; b = NB / 2 is the rule p > 0.5.
 *   r(p)      = floor(p * 2^24) in 0..2^24, the fixed-point confidence (the product is exact; r = p * 2^24 on [0.5, 1], truncated below).
 *   target    RU_CALIB_TARGET_REGIONS: float32 [N][C][V], y = g > 0.5, a NaN target is invalid.  RU_CALIB_TARGET_LABELS: uint8 [N][V] label
 *             volume, C = 3 regions WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4}; a label outside 0..4 is invalid for all three.
 *   A voxel that is invalid for a channel counts in invalid[n][c] and in no bin.
 * ru_calib_histogram: pred float32 [N][C][V], C <= RU_CALIB_MAX_C, 1 <= V <= 2^31, any 4-byte alignment -> per (n, c), all uint64, written (not
 *   accumulated) and cleared by a kernel of the call:  hist [N][C][NB+1][2] = voxels per (k, y);  conf [N][C][NB+1][2] = the sum of r;
 *   sq [N][C][2][2] = per y {sum of (r*r & 0xffffffff), sum of (r*r >> 32)}, so that S2 = sq[y][1] * 2^32 + sq[y][0] is the exact sum of r^2;
 *   invalid [N][C].  Integer atomics only: two calls give identical bytes.  The prediction and a float32 target are read once; a label volume
 *   is read once per region (1 byte a voxel beside the prediction's 4).
 * ru_calib_accumulate: one launch.  pool_hist [C][NB+1][2], pool_conf [C][NB+1][2] += the sums over the N samples; pool_sq [C][2][2] takes the
 *   samples' S2 and is kept carried (its low word < 2^32).  With the mask k > b for b = 0..NB:  TP_b = sum_{k>b} hist[k][1], FP_b = sum_{k>b} hist[k][0],
 *   FN_b = sum_{k<=b} hist[k][1], TN_b = sum_{k<=b} hist[k][0] (exact integers), and in float64, one division each,
 *   Dice_b = 2TP / (2TP + FP + FN), Sens_b = TP / (TP + FN), Spec_b = TN / (TN + FP), each 1 for a zero denominator.
 *   curve_acc [C][3][NB+1] (Dice, Sens, Spec) += ((v_0 + v_1) + ...) + v_(N-1), the samples in order; curves_out [N][C][3][NB+1] may be NULL.
 * ru_calib_summary: from the pooled tables, with M coarse bins (M divides NB), coarse bin m = (max(k, 1) - 1) / (NB / M):
 *   n_m = voxels, conf_m = (double)R_m / ((double)n_m * 2^24) with R_m the sum of r, freq_m = (double)n_m(y=1) / (double)n_m,
 *   ECE = sum over the non-empty bins in order of m of ((double)n_m / (double)n) * |freq_m - conf_m| (product rounded, then added),
 *   MCE = the largest |freq_m - conf_m|, Brier = T / ((double)n * 2^48) with the exact integer T = S2(y=0) + n(y=1) * 2^48 - 2^25 * R(y=1) + S2(y=1)
 *   converted as (double)(T >> 64) * 2^64 + (double)(T mod 2^64).  out [C][7] = {ECE, MCE, Brier, mean confidence = (double)R / ((double)n * 2^24),
 *   prevalence = (double)n(y=1) / (double)n, n, non-empty coarse bins}, table [C][M][3] = {n_m, conf_m, freq_m} (zeros for an empty bin), float64.
 *   An empty channel (n = 0) gives zeros.
 * ru_threshold_regions: probs float32 [C][V], thresholds = HOST float[C] (no NaN) -> mask uint8 [C][V] = p > t (a NaN p gives 0), counts [C] = exact
 *   voxels set.  At t = 0.5 the mask and counts are ru_ens_finalize's on the same mean, bit for bit. */
#define RU_CALIB_TARGET_REGIONS 0
#define RU_CALIB_TARGET_LABELS 1
#define RU_CALIB_MIN_NB 16
#define RU_CALIB_MAX_NB 1024
#define RU_CALIB_DEFAULT_NB 256
#define RU_CALIB_MAX_C 8
int ru_calib_histogram(const float* pred, const void* target, int kind, int N, int C, size_t V, int NB, unsigned long long* hist,
                       unsigned long long* conf, unsigned long long* sq, unsigned long long* invalid, ru_stream_t stream);
int ru_calib_accumulate(const unsigned long long* hist, const unsigned long long* conf, const unsigned long long* sq, int N, int C, int NB,
                        unsigned long long* pool_hist, unsigned long long* pool_conf, unsigned long long* pool_sq, double* curve_acc,
                        double* curves_out, ru_stream_t stream);
int ru_calib_summary(const unsigned long long* pool_hist, const unsigned long long* pool_conf, const unsigned long long* pool_sq, int C, int NB, int M,
                     double* out, double* table, ru_stream_t stream);
int ru_threshold_regions(const float* probs, int C, size_t V, const float* thresholds, unsigned char* mask, unsigned long long* counts,
                         ru_stream_t stream);

/* ---------------------------------------------------------------- BraTS challenge metrics: Dice, sensitivity, specificity, HD95
 * Per sample n and region k, P and G are binary masks on the D x H x W grid, every extent in [1, 512] (larger: RU_EINVAL).
 *   kind RU_SURFACE_PROB : pred, target = [N][C][D][H][W] float32, P = pred > 0.5 and G = target > 0.5 per channel, K = C regions.
 *   kind RU_SURFACE_LABEL: pred, target = [N][D][H][W] uint8 label volumes, C = 1, K = RU_SURFACE_REGIONS in the model's channel order:
 *                          WT = {1, 2, 3, 4}, TC = {1, 3, 4}, ET = {3, 4}; a voxel where either value is above 4 is in no region and
 *                          is counted in counts[.][RU_SURFACE_C_INVALID] (the caller reports it).
 * Surface dA = the voxels of A with a face neighbour (6-connectivity) outside A or outside the grid.  S = the multiset of the squared
 * distances from each voxel of dP to the nearest voxel of dG and from each voxel of dG to the nearest of dP (exact integers, voxel
 * centres, unit spacing); HD95 = numpy.percentile(sqrt(S), 95) with numpy's default linear method reproduced exactly (x = (n-1)*0.95,
 * i = floor(x), j = min(i+1, n-1), t = x - i, numpy's _lerp of sqrt(s_(i)) and sqrt(s_(j)) in float64).  HD95 = 0 when both masks are
 * empty and `empty_value` when exactly one is.  From the exact counts, in float64: Dice = 2TP/(|P|+|G|) (1 when both are empty),
 * sensitivity = TP/|G| (1 when |G| = 0), specificity = (V-|P|-|G|+TP)/(V-|G|) (1 when |G| = V).
 *   ru_surface_metrics   : values [N][K][4] float64 = {RU_SURFACE_DICE, _SENS, _SPEC, _HD95}; counts [N][K][RU_SURFACE_COUNTS] uint64 =
 *                          {|P|, |G|, TP, |dP|, |dG|, invalid voxels of sample n (kind RU_SURFACE_LABEL; 0 otherwise)}.  Both are written
 *                          by the call (cleared by a kernel).  ws: ru_surface_workspace_bytes(kind, N, C, D, H, W) bytes (0 for a bad
 *                          shape or kind): 8 B per voxel for two distance maps, the four bit masks, and one histogram of
 *                          (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 uint32 bins per (n, k).  RU_EINVAL for a bad kind, an extent outside
 *                          [1, 512], 2 * N * K > 65535 (the launch grids) or an undersized workspace.
 *   ru_surface_accumulate: acc[i] += mean over the N samples of values[n][i][column] in float64, i < nacc (<= K, <= 64).
 *   ru_surface_distances : ru_surface_metrics' passes in the same workspace, `values` and `counts` byte for byte the same, and one more
 *                          launch that rereads the histogram: extras [N][K][T + 2] float64 = {NSD_0 .. NSD_T-1, ASSD, HD} for T in
 *                          [0, RU_SURFACE_MAX_TOL] tolerances.  With n = |dP| + |dG| and h_b the number of distances whose square is b:
 *                            NSD_t = #{s in S : s <= tol_bins[t]} / n, an exact 64-bit count and one float64 division (the normalized
 *                                    surface Dice, "surface Dice at tolerance tau", in the voxel-surface form: every surface voxel counts
 *                                    once, no surface-element areas).  tol_bins is a HOST array of integer limits on the SQUARED distance:
 *                                    for a tolerance tau the caller passes the largest b with sqrt((double)b) <= tau, which makes the test
 *                                    sqrt(s) <= tau exact; a limit at or beyond the number of bins means every distance.  The limits
 *                                    travel as kernel arguments: nothing is uploaded and nothing waits.
 *                            ASSD  = sum_b h_b * sqrt((double)b) / n (the average symmetric surface distance), float64 without contraction:
 *                                    thread i of 1024 adds its ceil(bins / 1024) consecutive bins in ascending order, then a fixed tree
 *                                    (thread i += thread i + 512, + 256, ... + 1), one division.  No floating-point atomics: the same bytes
 *                                    for the same bytes.
 *                            HD    = sqrt((double)max S), the symmetric Hausdorff distance.
 *                          Empty rules (conventions of this library, not checked against any official evaluator): P and G both empty:
 *                          NSD = 1, ASSD = HD = 0; exactly one empty: NSD = 0, ASSD = HD = empty_value.  Unit spacing only; the overlap of
 *                          each direction on its own is not offered.  RU_EINVAL as ru_surface_metrics, and for T outside
 *                          [0, RU_SURFACE_MAX_TOL], tol_bins == NULL with T > 0, or extras == NULL.
 *   ru_surface_extras_accumulate: acc[i] += mean over the N samples of extras[n][i][column] in float64 for rows of `ncols` columns
 *                          (ncols = T + 2 for ru_surface_distances' extras, T + 1 for ru_lesion_distances' summary_ex), i < nacc. */
#define RU_SURFACE_PROB 0
#define RU_SURFACE_LABEL 1
#define RU_SURFACE_REGIONS 3
#define RU_SURFACE_DICE 0
#define RU_SURFACE_SENS 1
#define RU_SURFACE_SPEC 2
#define RU_SURFACE_HD95 3
#define RU_SURFACE_COUNTS 6
#define RU_SURFACE_C_INVALID 5
size_t ru_surface_workspace_bytes(int kind, int N, int C, int D, int H, int W);
int ru_surface_metrics(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, double empty_value,
                       double* values, unsigned long long* counts, void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_surface_accumulate(const double* values, double* acc, int N, int K, int nacc, int column, ru_stream_t stream);
#define RU_SURFACE_MAX_TOL 8
int ru_surface_distances(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, double empty_value,
                         const unsigned* tol_bins, int T, double* values, unsigned long long* counts, double* extras, void* ws,
                         size_t ws_bytes, ru_stream_t stream);
int ru_surface_extras_accumulate(const double* extras, double* acc, int N, int K, int nacc, int ncols, int column, ru_stream_t stream);

/* ---------------------------------------------------------------- lesion-wise Dice and HD95 (csrc/lesion.hip)
 * Per sample n and region k, P and G are the masks of ru_surface_metrics (same kinds, same regions, every extent in [1, 512], and
 * D * H * W < 2^31).  Parameters: dilation >= 0, min_volume >= 0, empty_value.
 *   1. Dil(A) = `dilation` iterations of the binary dilation by the voxel, its 6 face and its 12 edge neighbours
 *      (scipy.ndimage.binary_dilation(A, generate_binary_structure(3, 2), iterations=dilation)); outside the grid is background.
 *   2. Z_1..Z_n = the 26-connected components of Dil(G), numbered by ascending smallest linear voxel index (scipy.ndimage.label with a
 *      3 x 3 x 3 structure of ones).  Lesion L_i = G & Z_i (never empty), vol_i = |L_i|.
 *   3. Q_1..Q_m = the 26-connected components of P.
 *   4. M_i = the union of the Q_j that meet Z_i; one Q_j may belong to several M_i.  A Q_j that meets no Z_i is a false positive,
 *      whatever the volumes of the lesions; n_fp is their number.
 *   5. tp_i = |M_i & L_i| = |P & L_i|; Dice_i = 2 tp_i / (|M_i| + |L_i|) in float64; HD95_i = ru_surface_metrics' HD95 of the pair
 *      (M_i, L_i): `empty_value` when M_i is empty.
 *   6. Kept lesions: vol_i > min_volume; n_kept of them.  A dropped lesion leaves the sums; what it matched is still no false positive.
 *   7. den = n_kept + n_fp; LesionDice = sum_kept Dice_i / den; LesionHD95 = (sum_kept HD95_i + n_fp * empty_value) / den, float64 sums
 *      in ascending lesion order; den = 0: LesionDice = 1, LesionHD95 = 0.
 * ru_lesion_metrics: summary [N][K][2] float64 = {RU_LESION_DICE, RU_LESION_HD95}; counts [N][K][RU_LESION_COUNTS] uint64 = {n_gt, n_kept,
 *   n_tp (kept with M_i non-empty), n_fn (kept with M_i empty), n_fp, invalid voxels of sample n (kind RU_SURFACE_LABEL; 0 otherwise)};
 *   table, optional (NULL): [N][K][max_lesions][RU_LESION_COLUMNS] float64 = {vol_i, |M_i|, tp_i, Dice_i, HD95_i} for the n_gt lesions
 *   of (n, k), the dropped ones included; rows from n_gt on are not written.  More than max_lesions (1..65536) lesions in one (n, k):
 *   RU_EINVAL, nothing is truncated; the number of predicted components is not limited.
 *   The pairs (M_i, L_i) go through the surface passes of ru_surface_metrics as bit masks of the whole grid, RU_LESION_CHUNK at a time:
 *   the workspace holds one chunk, it does not grow with the number of lesions beyond 52 B per lesion of max_lesions and (n, k).  The call
 *   synchronises the stream ONCE, to read the lesion counts back (they size the chunk loop): it cannot be captured into a graph.
 *   ws: ru_lesion_workspace_bytes(kind, N, C, D, H, W, max_lesions) bytes (0 for a bad shape, kind or max_lesions).
 * ru_lesion_accumulate: acc[i] += mean over the N samples of summary[n][i][column] in float64, i < nacc (<= K, <= 64).
 * None of this was checked against the challenge's own evaluator: the penalty value (the public evaluator uses a constant near 374),
 * the absence of a size threshold on false positives and the 50-voxel default of the callers are open. */
#define RU_LESION_DICE 0
#define RU_LESION_HD95 1
#define RU_LESION_COUNTS 6
#define RU_LESION_C_INVALID 5
#define RU_LESION_COLUMNS 5
#define RU_LESION_CHUNK 8
size_t ru_lesion_workspace_bytes(int kind, int N, int C, int D, int H, int W, int max_lesions);
int ru_lesion_metrics(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                      double empty_value, double* summary, unsigned long long* counts, double* table, int max_lesions, void* ws,
                      size_t ws_bytes, ru_stream_t stream);
int ru_lesion_accumulate(const double* summary, double* acc, int N, int K, int nacc, int column, ru_stream_t stream);
/* ru_lesion_distances: ru_lesion_metrics' sequence with ru_surface_distances' finalize on every pair (M_i, L_i); `summary`, `counts` and
 *   `table` come out byte for byte as ru_lesion_metrics writes them.  Per lesion NSD_{i,t}, ASSD_i and HD_i follow ru_surface_distances
 *   (a missed lesion, M_i empty: NSD_i = 0, ASSD_i = HD_i = empty_value).  summary_ex [N][K][T + 1] float64, sums over the kept lesions
 *   in ascending lesion order without contraction, den = n_kept + n_fp:
 *     LesionNSD_t = sum_kept NSD_{i,t} / den (a false-positive component adds 0); 1 when den = 0;
 *     LesionASSD  = (sum_kept ASSD_i + n_fp * empty_value) / den; 0 when den = 0.
 *   table_ex, optional (NULL): [N][K][max_lesions][T + 2] float64 = {NSD_{i,0..T-1}, ASSD_i, HD_i} for the n_gt lesions, the dropped ones
 *   included; rows from n_gt on are not written.  tol_bins, T as ru_surface_distances.  Still one synchronisation, the lesion counts.
 *   ws: ru_lesion_distances_workspace_bytes(kind, N, C, D, H, W, max_lesions, T) = ru_lesion_workspace_bytes' plus 8 (T + 2) B per lesion
 *   of max_lesions and (n, k); 0 for a bad shape, kind, max_lesions or T.  Conventions of this library, not checked against any evaluator. */
size_t ru_lesion_distances_workspace_bytes(int kind, int N, int C, int D, int H, int W, int max_lesions, int T);
int ru_lesion_distances(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                        double empty_value, const unsigned* tol_bins, int T, double* summary, unsigned long long* counts, double* table,
                        double* summary_ex, double* table_ex, int max_lesions, void* ws, size_t ws_bytes, ru_stream_t stream);

/* ---------------------------------------------------------------- training input pipeline (dataloader.py:100-216, SimpleReader)
 * ru_zscore_stats: per channel stats[c] = { #(x > 0), sum x, sum x^2 } over all V voxels in float64 -- the three numbers the
 *   reference's normalisation is made of (dataloader.py:124-130: the count is over positive voxels, the sums over all).
 * ru_augment_patch: ONE pass from the resident raw case to a training patch (dataloader.py:147-205): crop [lo, lo + patch),
 *   z-score ((x - mean) * inv_std), zoom by `scale` per axis (scipy.ndimage.affine_transform with a diagonal matrix, order 1,
 *   mode 'reflect', applied to the modalities and to the one-hot label), flips (flags bit 0/1/2 = axes D/H/W), transpose of D
 *   and H (bit 3), per-channel gain and bias, WT/TC/ET soft targets.  data_out [C][Q0][Q1][P2], target_out [3][Q0][Q1][P2] with
 *   (Q0, Q1) = (P1, P0) when transposed.  The small parameter arrays are HOST pointers, read at launch.  C <= 8.
 *   Refused (RU_EINVAL, before any launch): a crop outside the volume, a scale that is not positive or not finite, and a scale with
 *   scale[i] * (patch[i] - 1) >= 2^30 (the source cell floor(scale * index) is held in 32 bits). */
size_t ru_zscore_workspace_bytes(int C, size_t V);
int ru_zscore_stats(const float* image, double* stats, int C, size_t V, void* ws, size_t ws_bytes, ru_stream_t stream);
int ru_augment_patch(const float* image, const unsigned char* label, const float* mean, const float* inv_std,
                     int C, int D, int H, int W, const int* crop_lo, const int* patch, const double* scale, int flags,
                     const float* gain, const float* bias, float* data_out, float* target_out, ru_stream_t stream);
/* ru_augment_patch_soft: the same pass for distillation.  soft [3][D][H][W] = a teacher's WT/TC/ET probabilities in the case's frame
 * (ru_paste_probs): the targets are affine_transform(soft, (1, sx, sy, sz), order=1, mode='reflect') of the crop -- the reference's call
 * at dataloader.py:179 on three float channels -- with the same flips and transpose; `label` is not read then (may be NULL).
 * soft = NULL: ru_augment_patch. */
int ru_augment_patch_soft(const float* image, const unsigned char* label, const float* soft, const float* mean, const float* inv_std,
                          int C, int D, int H, int W, const int* crop_lo, const int* patch, const double* scale, int flags,
                          const float* gain, const float* bias, float* data_out, float* target_out, ru_stream_t stream);

/* ---------------------------------------------------------------- rotation augmentation (csrc/rotate.hip).  Opt-in; ru_augment_patch is not touched.
 * ru_augment_patch_affine: ONE pass from the resident raw case to a rotated / zoomed / sheared training patch, in ru_augment_patch's slot.  Per image
 *   channel, per one-hot label class (soft = NULL) or per channel of soft [3][D][H][W] (label may then be NULL):
 *     scipy.ndimage.affine_transform(volume, matrix, offset, output_shape=patch, order=1, mode='grid-constant', cval=0)
 *   on the WHOLE volume: for output index q = (i, j, k) of the patch, before flips and transpose, the source coordinate is s = matrix q + offset in
 *   float64 (matrix row-major 3 x 3, whole-volume voxel coordinates; per axis ((m0 i + m1 j) + m2 k) + offset, every operation rounded on its own);
 *   f = floor(s), t = (float)(s - f); the eight corners f + {0,1}^3 are weighted by products of 1 - t and t.  A corner outside [0,D) x [0,H) x [0,W)
 *   contributes the fill: raw intensity 0 for the image (it z-scores to what real background gets), label 0, soft 0.  A coordinate that is not a
 *   number, below -2 or above the axis extent counts as -2 / the extent (both corners outside).  The crop need not lie inside the volume.
 *   Then ru_augment_patch's tail, expression for expression: ((acc - mean) * inv_std) * gain + bias, the class weights summed to WT / TC / ET, flips
 *   (flags bit 0/1/2), the D <-> H transpose (bit 3).  data_out [C][Q0][Q1][P2], target_out [3][Q0][Q1][P2], (Q0, Q1) = (P1, P0) when transposed.
 *   With matrix = diag(1) and an integer offset inside the volume the result is ru_augment_patch's at scale 1, bit for bit.
 *   mapping: RU_AFFINE_MAP_ROW (256 consecutive output voxels along W per workgroup), RU_AFFINE_MAP_BRICK (a 4 x 2 x 8 brick of output voxels per
 *   wavefront) or RU_AFFINE_MAP_DEFAULT; the bytes written do not depend on it.  The small parameter arrays are HOST pointers, read at launch.  No
 *   workspace, no atomics; the call only enqueues (graph-capturable).  Refused (RU_EINVAL, before any launch): a null pointer, C outside 1..8, a
 *   volume or patch extent <= 0, P0 P1 P2 >= 2^31 - 1, flags outside bits 0..3, an unknown mapping, a matrix or offset entry that is not finite,
 *   |det(matrix)| < 1e-6 (a collapsed patch). */
#define RU_AFFINE_MAP_DEFAULT 0
#define RU_AFFINE_MAP_ROW 1
#define RU_AFFINE_MAP_BRICK 2
int ru_augment_patch_affine(const float* image, const unsigned char* label, const float* soft, const float* mean, const float* inv_std,
                            int C, int D, int H, int W, const int* patch, const double* matrix, const double* offset, int flags,
                            const float* gain, const float* bias, int mapping, float* data_out, float* target_out, ru_stream_t stream);

/* ---------------------------------------------------------------- elastic deformation of a training patch (dataloader.py:24-48 elastic_transform,
 * the commented-out call sites :177 / :180 and the draws :166-168).  Opt-in; ru_augment_patch is not touched.  All three calls only enqueue.
 * ru_elastic_noise: noise_out [3][P0][P1][P2] float64, uniform in [-1, 1): a counter-based generator (two rounds of splitmix64's finalizer), a pure
 *   function of (seed, field, linear voxel index) -- the stand-in for `random_state.rand(*shape) * 2 - 1`; numpy's Mersenne Twister stream is not
 *   reproduced, which is why ru_elastic_field takes the noise as an INPUT.
 * ru_elastic_field: disp_out [3][P0][P1][P2] float64 = scipy.ndimage.gaussian_filter(noise[f], sigma, mode="constant", cval=0) times alpha, alpha,
 *   alpha / 2.5: radius int(4 sigma + 0.5), weights exp(-0.5 x^2 / sigma^2) / sum, three separable passes along axis 0, 1, 2, zero outside the
 *   volume, accumulated and stored in float64.  The radius may exceed an extent.  Refused (RU_EINVAL, before any launch): sigma <= 0 or not finite,
 *   radius > 256, P2 > 512, P0 > 21845, noise == disp_out.  ws: ru_elastic_workspace_bytes(P0, P1, P2).
 * ru_elastic_warp: every output voxel reads its source at (i + d0, j + d1, k + d2) in float64.  The C image channels take
 *   map_coordinates(order=1, mode='reflect'): linear interpolation on the half-sample-symmetric extension (d c b a | a b c d | d c b a), periodic
 *   beyond one reflection; the T target channels take order=0: the voxel at floor(c + 0.5) on the same extension.  The same pass applies what
 *   ru_augment_patch applies last: flips (flags bit 0/1/2 = axes D/H/W), the D <-> H transpose (bit 3), gain and bias on the image channels
 *   (dataloader.py:184-204).  data_out [C][Q0][Q1][P2], target_out [T][Q0][Q1][P2], (Q0, Q1) = (P1, P0) when transposed; not in place.  gain and
 *   bias are HOST pointers read at launch.  C, T in 0..8 (a count of 0 skips that group and its pointers). */
size_t ru_elastic_workspace_bytes(int P0, int P1, int P2);
int ru_elastic_noise(unsigned long long seed, int P0, int P1, int P2, double* noise_out, ru_stream_t stream);
int ru_elastic_field(const double* noise, double sigma, double alpha, int P0, int P1, int P2, double* disp_out, void* ws, size_t ws_bytes,
                     ru_stream_t stream);
int ru_elastic_warp(const float* data_in, int C, const float* target_in, int T, const double* disp, int P0, int P1, int P2, int flags,
                    const float* gain, const float* bias, float* data_out, float* target_out, ru_stream_t stream);

/* ---------------------------------------------------------------- intensity augmentation of a training patch (csrc/intensity.hip).  Opt-in, a stage of
 * its own behind ru_augment_patch / ru_elastic_warp; the call only enqueues.  in, out [C][P0][P1][P2] float32, C in 1..8, out may not overlap in.
 * `p` is a HOST pointer read at launch: per channel a mask of RU_INT_* bits and the parameters of the stages whose bit is set.  A channel with no
 * bit set is copied bit for bit.  Per channel the stages run in this order (dataloader.intensity_augment_host restates them in float64):
 *   RU_INT_BLUR        scipy.ndimage.gaussian_filter(x, blur_sigma, mode='reflect'): radius r = int(4 sigma + 0.5), weights exp(-0.5 d^2 / sigma^2) / sum,
 *                      three separable passes along axis 0, 1, 2 on the half-sample-symmetric extension (d c b a | a b c d | d c b a), periodic beyond
 *                      one reflection, so r may exceed an extent.  float32 weights, data and sums.
 *   RU_INT_LOWRES      per axis (extent P, z = lowres_zoom): n_c = max(1, floor(P z + 0.5)); coarse sample j = the source voxel
 *                      min(floor((j + 0.5) P / n_c), P - 1); output voxel i = linear interpolation of the coarse samples at
 *                      c = clamp((i + 0.5) n_c / P - 0.5, 0, n_c - 1).  Trilinear over 8 source voxels; indices in exact integer arithmetic.
 *                      (= zoom(zoom(x, n_c / P, order=0, mode='nearest', grid_mode=True), P / n_c, order=1, mode='nearest', grid_mode=True))
 *   RU_INT_NOISE       x + sqrt(noise_variance) * n(noise_seed, channel, v), v = the linear voxel index inside the channel.  With mix64 = splitmix64's
 *                      finalizer (ru_elastic_noise's) and G = 0x9E3779B97F4A7C15, all in 64-bit wrapping arithmetic:
 *                        key = mix64(noise_seed + (channel + 1) G),  z1 = mix64(key + (2 v + 1) G),  z2 = mix64(key + (2 v + 2) G),
 *                        u1 = ((z1 >> 11) + 1) / 2^53 in (0, 1],  u2 = (z2 >> 11) / 2^53 in [0, 1),  n = sqrt(-2 ln u1) cos(2 pi u2)   (Box-Muller)
 *                      The device evaluates ln, sqrt and cos in float32, ln u1 to a
 *                      RELATIVE error (logf(h) + (u1 - h) / h, h = float32(u1)): n is good to a few float32 roundings of itself.  A pure function of (seed, channel, v): no state, any launch shape.
 *   RU_INT_BRIGHTNESS  x * brightness
 *   RU_INT_CONTRAST    clip((x - mean) * contrast + mean, min, max) with mean, min, max of the channel as it enters this stage
 *   RU_INT_GAMMA       with min, range = max - min, mean, std (population) of the channel as it enters this stage, after the negation if
 *                      RU_INT_GAMMA_INVERT is set: y = ((x - min) / (range + 1e-7))^gamma * range + min; with RU_INT_GAMMA_RETAIN
 *                      y = (y - mean_y) * (std / (std_y >= 1e-8 ? std_y : 1e-8)) + mean; with RU_INT_GAMMA_INVERT the result is negated back.
 *                      t^gamma is formed as exp2(gamma log2 t).  The two modifier bits mean nothing without RU_INT_GAMMA.
 * Channel statistics: per-workgroup partials summed in float64 in a fixed order (as ru_zscore_stats): no float atomics, two calls give the same bytes,
 * min and max are exact.  Refused (RU_EINVAL, before any launch): C outside 1..8, overlapping in / out, unknown mask bits, blur_sigma <= 0 or not
 * finite or radius > 8 (sigma up to 2.0), lowres_zoom outside (0, 1], noise_variance < 0 or not finite, gamma <= 0 or not finite, brightness or
 * contrast not finite, ws smaller than ru_intensity_workspace_bytes(C, P0, P1, P2), P0 > 65535. */
#define RU_INT_BLUR 1
#define RU_INT_LOWRES 2
#define RU_INT_NOISE 4
#define RU_INT_BRIGHTNESS 8
#define RU_INT_CONTRAST 16
#define RU_INT_GAMMA 32
#define RU_INT_GAMMA_INVERT 64
#define RU_INT_GAMMA_RETAIN 128
typedef struct ru_intensity_params {      /* every array is indexed by channel; 8 = the pipeline's channel limit (ru_augment_patch) */
    int mask[8];
    double blur_sigma[8];
    double lowres_zoom[8];
    double noise_variance[8];
    unsigned long long noise_seed[8];
    double brightness[8];
    double contrast[8];
    double gamma[8];
} ru_intensity_params;
size_t ru_intensity_workspace_bytes(int C, int P0, int P1, int P2);
int ru_intensity_augment(const float* in, float* out, int C, int P0, int P1, int P2, const ru_intensity_params* p, void* ws, size_t ws_bytes,
                         ru_stream_t stream);

/* ---------------------------------------------------------------- the training set resident in HBM (csrc/resident.hip).  Opt-in; the entry points
 * above are not touched.
 * A PACKED case is the bounding box [box_lo, box_lo + box_size) of every voxel of image [C][D][H][W] float32, label [D][H][W] uint8 and (optional)
 * soft [3][D][H][W] float32 that is not zero: a voxel is inside if the BIT PATTERN of any image or soft channel is not that of +0.0f (so -0.0f and
 * NaN are inside) or its label is not 0.  Inside the box the image is stored as [C][b0][b1][b2] uint16 (RU_PACK_U16) or float32 (RU_PACK_F32), the
 * label as [b0][b1][b2] uint8, soft as [3][b0][b1][b2] float32.  Outside the box the case is +0.0f / label 0 bit for bit and inside it every value
 * is stored exactly, so ru_case_unpack(ru_case_pack(x)) == x byte for byte.
 * ru_case_probe: one pass; out8 (DEVICE, 8 ints) = box_lo[3], box_size[3], exact, 0.  exact = 1 if every image value x satisfies
 *   bits((float)(uint16)x) == bits(x) -- negative, fractional, above 65535, -0.0f and NaN values clear it; only then may the case be packed as
 *   RU_PACK_U16.  An all-zero case gets box_lo = (0,0,0), box_size = (1,1,1).  Integer min / max atomics only: two calls give the same bytes.
 * ru_case_pack: crops to the box (the caller passes what the probe wrote); kind RU_PACK_U16 on a case that is not exact is not detected here.
 * ru_case_unpack: the inverse, +0.0f / label 0 outside the box.  soft and soft_out are both NULL or both set.
 * All three only enqueue.  Refused (RU_EINVAL, before any launch): a null pointer, C outside 1..8, an extent <= 0, an unknown kind, a box that does
 * not lie inside the volume.
 *
 * ru_augment_batch_packed: ONE launch cuts N patches from N packed cases (the same case may appear more than once) straight into
 *   data_out [N][C][Q0][Q1][P2] and target_out [N][3][Q0][Q1][P2]; N = 1 is the single-patch entry.  Sample n is cases[n] + patches[n] (HOST arrays,
 *   read at launch: the descriptors travel as kernel arguments, at most RU_AUG_BATCH_MAX samples per launch, more are sent in chunks).  A sample of
 *   mode RU_AUG_ZOOM computes what ru_augment_patch / ru_augment_patch_soft compute on the unpacked case for (crop_lo, patch, scale, flags, gain,
 *   bias), one of mode RU_AUG_AFFINE what ru_augment_patch_affine computes for (patch, matrix, offset, flags, gain, bias, mapping), bit for bit:
 *   the kernels instantiate one per-voxel function (csrc/augment_voxel.hpp) on different sources.  A case with soft != NULL gets its targets from
 *   soft.  Every sample has the same channel count and the same patch; a transposed sample (flags bit 3) in a batch of more than one needs
 *   P0 == P1.  No workspace, no atomics, no synchronisation: the call only enqueues.  Refused (RU_EINVAL, before any launch): what the
 *   single-patch entry points refuse (crop outside the volume, scale <= 0, not finite or scale * (patch - 1) >= 2^30 for zoom; matrix or offset not finite, |det| < 1e-6, unknown
 *   mapping for affine; flags outside bits 0..3; C outside 1..8; patch extents <= 0 or P0 P1 P2 >= 2^31 - 1), N < 1, an unknown kind or mode, a
 *   box outside its volume, differing channel counts, a transposed sample with P0 != P1 and N > 1. */
#define RU_PACK_F32 0
#define RU_PACK_U16 1
#define RU_AUG_ZOOM 0
#define RU_AUG_AFFINE 1
#define RU_AUG_BATCH_MAX 8                /* samples per launch: 8 x 352 bytes of descriptors stay well under HIP's 4 KB of kernel arguments */
typedef struct ru_case_desc {
    const void* image;                    /* packed image, DEVICE: uint16 or float32 by `kind` */
    const unsigned char* label;           /* packed label, DEVICE */
    const float* soft;                    /* packed soft targets, DEVICE, or NULL */
    int kind;                             /* RU_PACK_F32 / RU_PACK_U16 */
    int C;
    int dims[3];                          /* D, H, W of the whole case */
    int box_lo[3], box_size[3];
    float mean[8], inv_std[8];            /* z-score constants per channel */
} ru_case_desc;
typedef struct ru_patch_desc {
    int mode;                             /* RU_AUG_ZOOM / RU_AUG_AFFINE */
    int flags;                            /* bit 0/1/2: flip D/H/W, bit 3: transpose D <-> H */
    int mapping;                          /* affine: RU_AFFINE_MAP_*; zoom: ignored */
    int crop_lo[3];                       /* zoom */
    double scale[3];                      /* zoom */
    double matrix[9], offset[3];          /* affine */
    float gain[8], bias[8];
} ru_patch_desc;
int ru_case_probe(const float* image, const unsigned char* label, const float* soft, int C, int D, int H, int W, int* out8, ru_stream_t stream);
int ru_case_pack(const float* image, const unsigned char* label, const float* soft, int C, int D, int H, int W, const int* box_lo,
                 const int* box_size, int kind, void* image_out, unsigned char* label_out, float* soft_out, ru_stream_t stream);
int ru_case_unpack(const void* image, const unsigned char* label, const float* soft, int kind, int C, int D, int H, int W, const int* box_lo,
                   const int* box_size, float* image_out, unsigned char* label_out, float* soft_out, ru_stream_t stream);
int ru_augment_batch_packed(const ru_case_desc* cases, const ru_patch_desc* patches, int N, const int* patch, float* data_out, float* target_out,
                            ru_stream_t stream);

/* ---------------------------------------------------------------- CarveMix: lesion-aware mixing of two patches (csrc/carvemix.hip).  Opt-in; the
 * entry points above are not touched.  Written from the paper (Zhang et al., MICCAI 2021); not checked against the authors' code.
 * A donor patch (Xa [C][D][H][W], Ya [3][D][H][W]) is carved into a receiver patch (Xb, Yb) of the same shape, float32, channel 0 of the target
 * being WT, for two host draws u in [0, 1) (float64) and side in {RU_CARVE_OUTER, RU_CARVE_INNER}:
 *   G = Ya[0] > 0.5f (the mask rule of ru_signed_sqdist), V = |G|, n = D H W;  s = ru_signed_sqdist(Ya[0]) (>= 1 outside G, <= -1 inside);
 *   R2 = the largest integer q with q^3 <= V^2 (64-bit integer search; floor(V^(2/3)), the squared form of the paper's lambda_u = V^(1/3));
 *   outer: T = floor((u u) R2);  inner: T = -ceil(((u u) R2) 0.25)  -- float64, plain IEEE multiplies, nothing fused;
 *   V == 0: T = INT32_MIN (nothing is carved);  V == n: T = INT32_MAX (the output is the donor);
 *   M = s <= T;  X = M ? Xa : Xb per channel, Y = M ? Ya : Yb: a select of 32-bit words, so NaN and -0.0f pass through bit for bit.
 * ru_carvemix_threshold: wt [K][n] float32 (the donors' WT channels, as handed to ru_signed_sqdist), u [K] and side [K] HOST arrays that travel as
 *   kernel arguments (RU_CARVE_BATCH_MAX donors per launch, more are sent in chunks).  V is counted exactly in integers (one partial per workgroup,
 *   added in a fixed order); T_out int32 [K] and V_out int64 [K] are DEVICE arrays.  n <= 2^27.  ws: ru_carvemix_workspace_bytes(K, n).
 * ru_carvemix_mix: ONE launch (per RU_CARVE_BATCH_MAX donors) for the batch: donor k (donor_data [K][C][n], donor_target [K][3][n], s [K][n], T [K]
 *   on the DEVICE) goes into receiver dst[k] of data [N][C][n] / target [N][3][n], IN PLACE; dst is a HOST array of K distinct indices.  Quads
 *   without a selected voxel are neither loaded nor stored.  mask_out (optional, uint8 [K][n]) receives M.  Tensors of a pair that do not share an
 *   offset from a 16-byte boundary (or n % 4 != 0) go one voxel at a time.
 * Both only enqueue: no float atomics, no synchronisation, two calls give identical bytes.  Refused (RU_EINVAL, before any launch): a null or
 * misaligned pointer, K < 1, K > N, C outside 1..8, an extent <= 0 or n > 2^27, u outside [0, 1), an unknown side, dst outside [0, N) or not
 * distinct, a donor tensor, the map, T or mask_out overlapping a receiver tensor, a workspace that is too small. */
#define RU_CARVE_OUTER 0
#define RU_CARVE_INNER 1
#define RU_CARVE_BATCH_MAX 8              /* donors per launch: 8 x 64 bytes of pointers and lanes travel as kernel arguments */
size_t ru_carvemix_workspace_bytes(int K, size_t n);
int ru_carvemix_threshold(const float* wt, int K, size_t n, const double* u, const int* side, int* T_out, long long* V_out, void* ws,
                          size_t ws_bytes, ru_stream_t stream);
int ru_carvemix_mix(const float* donor_data, const float* donor_target, const int* s, const int* T, int K, const int* dst, int N, int C, int D,
                    int H, int W, float* data, float* target, unsigned char* mask_out, ru_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RESUNET_HIP_H_ */
