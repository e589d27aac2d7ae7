/*
 * unet_hip.h — C ABI of libunet_hip.so: the MI355X (gfx950) kernels behind the
 * Our_UNet train step of Ulixes-8/UNet-Implementations.
 *
 * The reference has no FFI: its operator API for this path is the PyTorch module
 * surface.  Every entry point below replaces the ATen op(s) the
 * reference reaches through torch.nn at the cited file:line (paths relative to
 * the reference checkout).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every function returns 0 on success or a negative UNET_E_* code;
 *     unet_last_error() returns a thread-local message for the last failure.
 *   - all data pointers are DEVICE pointers owned by the caller (no ownership
 *     transfer, no hidden allocation) unless the parameter is marked UNET_HOST
 *     (see the macro below); workspaces are caller-provided and sized by the
 *     matching *_workspace_bytes() query.
 *   - the Python binding is derived from this file by a small parser
 *     (unet-implementations_amd/_header.py) that refuses what it does not know:
 *     keep to one declaration per export, the scalar types int / float / double /
 *     size_t / int64_t / uint64_t, plain pointers and `typedef struct` records.
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*).
 *   - activations are NHWC fp32 ("pixel-major": [N][H][W][C]); logits and the
 *     input image cross the module boundary as NCHW, exactly like the reference.
 *   - packed 3x3 weights, tap = ky*3+kx, the GEMM's reduction axis contiguous:
 *     wf[tap][co][ci] (forward: K = ci) and wd[tap][ci][co] (data gradient: K = co).
 */
#ifndef UNET_HIP_H_
#define UNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_ABI_VERSION 11

#define UNET_OK 0
#define UNET_E_INVALID (-1) /* bad argument / unsupported shape */
#define UNET_E_LAUNCH (-2)  /* HIP launch or runtime error */
#define UNET_E_WORKSPACE (-3) /* workspace too small */

typedef void* unet_stream_t; /* hipStream_t */

/* Where a pointer lives, for readers and for the Python binding, which parses this header; both
 * macros expand to nothing.
 *   UNET_HOST    A pointer to data (float*, void*, ...) is a device address unless marked so: then
 *                the library dereferences it on the host during the call, and the binding types
 *                `T* UNET_HOST p` as POINTER(T) instead of an address.  (The char buffer of
 *                unet_debug_recorded_launches is host memory too and stays an address.)
 *   UNET_DEVICE  A pointer to one of the records below (unet_act_src*, unet_bwd_stats*) is read
 *                on the host during the call unless marked so: then it is a table in device
 *                memory that the kernels read, an address to the binding. */
#define UNET_HOST
#define UNET_DEVICE

const char* unet_last_error(void);
int unet_abi_version(void);
/* number of HIP devices visible to the library (0 without a GPU); never fails */
int unet_device_count(void);

/* Test hook.  Operands are addressed through 2 GiB buffer descriptors; a batch whose tensor is
 * larger (the reference trains at bs 32: Our_UNet/src/train.py:748) is split over N inside the
 * convolution entry points.  This lowers the split threshold so the chunked path can be
 * exercised on small tensors; bytes <= 0 restores 2^31 - 1. */
int unet_debug_set_chunk_limit(int64_t bytes);

/* Test hook: a record of the kernels the library launches, so tests can assert which
 * instantiation a call selected.  unet_debug_record_launches clears the record and turns it on
 * (on != 0) or off; while off a launch costs one relaxed atomic load.  The record holds host
 * data only (harmless during graph capture).  unet_debug_recorded_launches writes the demangled
 * kernel names launched since the record was turned on, one per line in launch order (the
 * mangled name where the demangler gives up), NUL-terminated and truncated to cap - 1 bytes;
 * returns the length of the whole text (call with cap = 0 to size the buffer). */
int unet_debug_record_launches(int on);
size_t unet_debug_recorded_launches(char* buf, size_t cap);

/* ---- layout helpers ------------------------------------------------------ */

/* NCHW -> NHWC (module boundary for the input image, Our_UNet/models/unet.py:399) */
int unet_nchw_to_nhwc(const float* x_nchw, float* y_nhwc, int N, int C, int H, int W,
                      unet_stream_t stream);
/* NHWC -> NCHW (test helper / hooks that want the reference layout) */
int unet_nhwc_to_nchw(const float* x_nhwc, float* y_nchw, int N, int C, int H, int W,
                      unet_stream_t stream);

/* OIHW [Cout][Cin][3][3] (state_dict layout, Our_UNet/models/unet.py:106-115)
 * -> wf[9][Cout][Cin] and wd[9][Cin][Cout]; either output may be NULL. */
int unet_pack_conv3x3_weights(const float* w_oihw, float* wf, float* wd, int Cout, int Cin,
                              unet_stream_t stream);

/* ---- 3x3 convolution (pad 1, stride 1 or 2) ------------------------------ */

/* y[N][Ho][Wo][Cout] = conv3x3(cat(x0[.., C0], x1[.., C1])) + bias.
 * Replaces nn.Conv2d forward inside ConvBlock (Our_UNet/models/unet.py:106-115,
 * stride rule :103) and the torch.cat of UpBlock (:228) via the two-source
 * input (x1 may be NULL with C1 = 0).  H, W are the INPUT spatial sizes;
 * Ho = (H-1)/stride+1.  C0 == 3 (RGB stem) or C0, C1 multiples of 32;
 * Cout multiple of 32.
 */
int unet_conv3x3_fwd(const float* x0, int C0, const float* x1, int C1, const float* wf,
                     const float* bias, float* y, int N, int H, int W, int Cout, int stride,
                     unet_stream_t stream);

/* bf16 mixed-precision variants (BASELINE.json config 4; the reference's AMP path,
 * Our_UNet/src/train.py:638-652, is fp16 autocast): identical arguments and fp32 tensors; both
 * operands are rounded to bf16 while staged on chip and contracted on the bf16 matrix cores with
 * fp32 accumulation.  The RGB stem (C0 == 3) stays fp32. */
int unet_conv3x3_fwd_bf16(const float* x0, int C0, const float* x1, int C1, const float* wf,
                          const float* bias, float* y, int N, int H, int W, int Cout, int stride,
                          unet_stream_t stream);
int unet_conv3x3_bwd_data_bf16(const float* dy, const float* wd, int Cin_total, int ci_offset,
                               float* dx, int N, int H, int W, int Cout, int Ccols, int stride,
                               int accumulate, unet_stream_t stream);

/* dx[N][H][W][Ccols] (+)= conv3x3_transpose(dy[N][Ho][Wo][Cout], wd slice).
 * Replaces the data-gradient half of aten::convolution_backward reached from
 * loss.backward() (Our_UNet/src/train.py:663).  wd is the whole
 * wd[9][Cin_total][Cout]; the call produces input channels
 * [ci_offset, ci_offset + Ccols) into dx, whose channel count is Ccols (the two
 * halves of a concatenated input are two calls).  H, W are the spatial sizes of
 * dx (the conv INPUT).  accumulate != 0 adds into dx (skip tensors receive two
 * gradients). */
int unet_conv3x3_bwd_data(const float* dy, const float* wd, int Cin_total, int ci_offset,
                          float* dx, int N, int H, int W, int Cout, int Ccols, int stride,
                          int accumulate, unet_stream_t stream);

/* dw_oihw[Cout][Cin_total][3][3] (columns ci_offset .. ci_offset+Cx) =
 *   sum over pixels of x[.., Cx] (x) dy[.., Cout]; db[Cout] = sum dy if db != NULL.
 * Replaces the weight/bias-gradient half of aten::convolution_backward.
 * H, W are the spatial sizes of x (the conv input). */
size_t unet_conv3x3_bwd_weight_workspace_bytes(int N, int H, int W, int Cx, int Cout, int stride);
int unet_conv3x3_bwd_weight(const float* x, int Cx, const float* dy, float* dw_oihw,
                            int ci_offset, int Cin_total, float* db, void* workspace,
                            size_t workspace_bytes, int N, int H, int W, int Cout, int stride,
                            unet_stream_t stream);

/* bf16 mixed-precision weight gradient (config 4): same arguments; stride-1 layers run on the
 * bf16 matrix cores (operands rounded on chip, fp32 sums), the rest fall back to fp32. */
int unet_conv3x3_bwd_weight_bf16(const float* x, int Cx, const float* dy, float* dw_oihw,
                                 int ci_offset, int Cin_total, float* db, void* workspace,
                                 size_t workspace_bytes, int N, int H, int W, int Cout, int stride,
                                 unet_stream_t stream);

/* Split-bf16 ("bf16x3") operand mode: fp32 operands are split on chip into three bf16 terms
 * (x = h + m + l, residual <= 2^-26 |x|) and every product is evaluated as the six bf16 x bf16
 * terms of weight >= 2^-16 on the bf16 matrix cores with fp32 accumulation; the dropped terms
 * are below one fp32 rounding of the product, so results agree with the fp32-MFMA entry points
 * to fp32 accuracy (tests/test_kernels_gpu.py compares both with fp64).  Arguments as the
 * plain entry points plus the weights pre-split by unet_pack_conv3x3_weights_bf16x3:
 * wf3 = [3][9][Cout][Cin] and wd3 = [3][9][Cin][Cout] bf16 (bit patterns as uint16_t), either
 * may be NULL in the pack call.  The RGB stem and the stride-2 weight gradient run on the fp32
 * path, which is why the fp32 wf / wd are still passed. */
int unet_pack_conv3x3_weights_bf16x3(const float* w_oihw, uint16_t* wf3, uint16_t* wd3, int Cout,
                                     int Cin, unet_stream_t stream);

/* Every layer's packing in ONE launch (the per-layer form costs 22 small launches per step).
 * `table_device` is an array of n entries in DEVICE memory, built once by the caller; all
 * pointers are device pointers, any destination may be NULL; Cout must be a multiple of 32.
 * A workgroup packs one 32 (co) x 32 (ci) x 9 tile: entry k owns the tiles
 * [tile_begin, tile_begin + (Cout/32) * ceil(Cin/32)), total_tiles = their sum.  Layouts as above. */
typedef struct unet_pack_entry {
  const float* w;   /* OIHW source [Cout][Cin][3][3] */
  float* wf;        /* [9][Cout][Cin] */
  float* wd;        /* [9][Cin][Cout] */
  uint16_t* wf3;    /* [3][9][Cout][Cin] bf16 planes ([1][9][Cout][Cin] when planes == 1) */
  uint16_t* wd3;    /* [3][9][Cin][Cout] bf16 planes */
  int Cout, Cin;
  int tile_begin;
  int reserved;     /* planes: 0 or 3 = the three planes of the split-bf16 form; 1 = only plane 0,
                       the bf16-rounded weight (what the mixed-precision kernels stage) */
} unet_pack_entry;
int unet_pack_conv3x3_weights_batched(const unet_pack_entry* UNET_DEVICE table_device, int n,
                                      int total_tiles, unet_stream_t stream);
int unet_conv3x3_fwd_bf16x3(const float* x0, int C0, const float* x1, int C1, const float* wf,
                            const uint16_t* wf3, const float* bias, float* y, int N, int H, int W,
                            int Cout, int stride, unet_stream_t stream);
int unet_conv3x3_bwd_data_bf16x3(const float* dy, const float* wd, const uint16_t* wd3,
                                 int Cin_total, int ci_offset, float* dx, int N, int H, int W,
                                 int Cout, int Ccols, int stride, int accumulate,
                                 unet_stream_t stream);
int unet_conv3x3_bwd_weight_bf16x3(const float* x, int Cx, const float* dy, float* dw_oihw,
                                   int ci_offset, int Cin_total, float* db, void* workspace,
                                   size_t workspace_bytes, int N, int H, int W, int Cout,
                                   int stride, unet_stream_t stream);

/* ---- 1x1 convolution (CLIP fusion layer) ---------------------------------- */

/* y = conv1x1(cat(x0, x1)) + bias with w[Cout][C0+C1]; replaces clip_fusion_conv[0] =
 * nn.Conv2d(512 + clip_dim, 512, 1) and the torch.cat in front of it
 * (CLIP_UNet/models/unet.py:356-362, :477-478). */
int unet_conv1x1_fwd(const float* x0, int C0, const float* x1, int C1, const float* w,
                     const float* bias, float* y, int N, int H, int W, int Cout,
                     unet_stream_t stream);
/* dx[.., Ccols] (+)= dy . wT[ci_offset.., :] with wT[Cin_total][Cout] (unet_transpose2d of w) */
int unet_conv1x1_bwd_data(const float* dy, const float* wT, int Cin_total, int ci_offset,
                          float* dx, int N, int H, int W, int Cout, int Ccols, int accumulate,
                          unet_stream_t stream);
/* dw[Cout][Cin_total] (columns ci_offset .. ci_offset+Cx); workspace sized by
 * unet_conv3x3_bwd_weight_workspace_bytes(N, H, W, Cx, Cout, 1) */
int unet_conv1x1_bwd_weight(const float* x, int Cx, const float* dy, float* dw, int ci_offset,
                            int Cin_total, void* workspace, size_t workspace_bytes, int N, int H,
                            int W, int Cout, unet_stream_t stream);
/* dst[C][R] = src[R][C]^T */
int unet_transpose2d(const float* src, float* dst, int R, int C, unet_stream_t stream);

/* ---- InstanceNorm2d(eps, affine) + LeakyReLU + SpatialDropout2d ----------- */

/* Per-(n,c) statistics of y[N][HW][C] and the folded affine coefficients
 *   alpha[n][c] = gamma[c]*rstd, beta2[n][c] = beta[c] - mean*alpha.
 * Replaces aten::native_batch_norm statistics as lowered from
 * nn.InstanceNorm2d(eps=1e-5, affine=True) (Our_UNet/models/unet.py:118-119).
 * mean, rstd, alpha, beta2 are [N][C]. */
size_t unet_instnorm_workspace_bytes(int N, int HW, int C);
int unet_instnorm_stats(const float* y, const float* gamma, const float* beta, float eps,
                        float* mean, float* rstd, float* alpha, float* beta2, void* workspace,
                        size_t workspace_bytes, int N, int HW, int C, unet_stream_t stream);

/* a = leaky_relu(y*alpha + beta2, slope) * mask ; mask [N][C] may be NULL.
 * Replaces InstanceNorm apply + nn.LeakyReLU (unet.py:122-123) +
 * SpatialDropout2d.forward (unet.py:13-35; mask already scaled by 1/(1-p)). */
int unet_instnorm_lrelu_drop_fwd(const float* y, const float* alpha, const float* beta2,
                                 const float* mask, float slope, float* a, int N, int HW, int C,
                                 unet_stream_t stream);

/* Backward of the block above: from ga = dL/da produce dy = dL/dy (may alias ga),
 * dgamma[C], dbeta[C] and dbias[C] = the gradient of the conv bias in front of the norm (may be
 * NULL) = sum over pixels of dy, evaluated in closed form from the reduction sums: it is
 * identically zero under InstanceNorm (the reference's autograd value is rounding noise). */
int unet_instnorm_lrelu_drop_bwd(const float* ga, const float* y, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta,
                                 const float* mask, float slope, float* dy, float* dgamma,
                                 float* dbeta, float* dbias, void* workspace,
                                 size_t workspace_bytes, int N, int HW, int C,
                                 unet_stream_t stream);

/* ---- bilinear 2x upsample (align_corners=False) --------------------------- */

/* y[N][2h][2w][C] from x[N][h][w][C]; replaces F.interpolate in UpBlock.forward
 * (Our_UNet/models/unet.py:219-225) for the exact-2x case. */
int unet_upsample2x_fwd(const float* x, float* y, int N, int h, int w, int C,
                        unet_stream_t stream);
/* gx[N][h][w][C] (+)= transpose-stencil of gy[N][2h][2w][C] (gather form, no atomics) */
int unet_upsample2x_bwd(const float* gy, float* gx, int N, int h, int w, int C, int accumulate,
                        unet_stream_t stream);

/* ---- 1x1 segmentation head ------------------------------------------------ */

/* logits_nchw[N][K][HW] = a[N][HW][C] . w[K][C] + b[K]; replaces
 * segmentation_output = nn.Conv2d(32, 3, 1) (Our_UNet/models/unet.py:374-381,:430).
 * C == 32, K <= UNET_MAX_CLASSES.  K <= 4 is the vector-unit kernel of the 3-class network;
 * 5 <= K <= 32 runs on the fp32 matrix cores (one v_mfma_f32_32x32x2_f32 tile of 32 pixels x 32
 * zero-padded classes per wave), here and in every unet_head1x1_* entry point below.  For K > 4
 * the backward leaves no InstanceNorm-backward reductions (bs->tiles_out == 0) and
 * unet_head1x1_in_bwd_fold returns plain da. */
#define UNET_MAX_CLASSES 32
int unet_head1x1_fwd(const float* a, const float* w, const float* b, float* logits_nchw, int N,
                     int HW, int C, int K, unet_stream_t stream);
size_t unet_head1x1_bwd_workspace_bytes(int N, int HW, int C, int K);
int unet_head1x1_bwd(const float* a, const float* dlogits_nchw, const float* w, float* da,
                     float* dw, float* db, void* workspace, size_t workspace_bytes, int N, int HW,
                     int C, int K, unet_stream_t stream);

/* ---- deferred slab reductions of the weight gradients ----------------------------------------
 * Every *_bwd_weight* entry point ends with 2-3 small launches that sum its per-workgroup slabs
 * in a fixed order and scatter the result into the OIHW gradient (44 such launches per train
 * step).  Between unet_wgrad_defer_begin() and unet_wgrad_defer_end() (per calling thread) the
 * entry points only QUEUE those reductions; unet_wgrad_defer_flush() launches everything queued
 * so far as 2-3 batched launches (all layers side by side; the same arithmetic in the same
 * order: bit-identical gradients).  While a reduction is queued its `workspace` must stay
 * allocated and dw_oihw is NOT yet valid.  The stand-alone bias gradient (db != NULL) cannot be
 * deferred: such a call fails before it launches or queues anything.  No reference counterpart
 * (aten::convolution_backward returns finished gradients). */
int unet_wgrad_defer_begin(void);
int unet_wgrad_defer_pending(void);
int unet_wgrad_defer_flush(unet_stream_t stream);
int unet_wgrad_defer_end(unet_stream_t stream);

/* ---- SimpleLoss: dynamic-weighted CE + soft Dice, forward and gradient ----- */

/* loss_out[0] = w_ce*CE + w_dice*Dice, loss_out[1] = CE, loss_out[2] = Dice,
 * loss_out[3..5] = the class weights used; dlogits (NCHW, may be NULL) = dL/dlogits.
 * Replaces SimpleLoss.forward and its autograd backward
 * (Our_UNet/models/losses.py:24-62 class weights, :73-76 CE, :84-121 Dice).
 * class_weights: 3 floats on device used when dynamic_weights == 0 (NULL = unweighted).
 * N <= 1024 images per call, here and in the _grad / _shard_stats / _shard_apply forms
 * (UNET_E_INVALID beyond, before any launch).
 * global_counts (optional, may be NULL): when non-NULL the kernel pair is split
 * so the caller can all-reduce the 4 class/valid counts between the passes. */
size_t unet_dice_wce_loss_workspace_bytes(int N, int H, int W);
int unet_dice_wce_loss_fwd_bwd(const float* logits_nchw, const int64_t* target, float* loss_out,
                               float* dlogits_nchw, void* workspace, size_t workspace_bytes,
                               int N, int H, int W, float smooth, float w_dice, float w_ce,
                               int ignore_index, int dynamic_weights, const float* class_weights,
                               float grad_scale, unet_stream_t stream);

/* The gradient pass alone, for a caller that learns dL/d(loss) only later (autograd's
 * backward): run unet_dice_wce_loss_fwd_bwd / _shard_apply with dlogits == NULL, keep the SAME
 * workspace (it holds the class weights and Dice coefficients of that call) and call this with
 * `upstream` = a device float holding dL/d(loss) (NULL = 1).  dlogits = upstream * the gradient
 * the one-call form writes (bit-identical for upstream == 1).  Replaces the autograd backward
 * of SimpleLoss.forward (Our_UNet/models/losses.py:64-82) without an extra scaling pass. */
int unet_dice_wce_loss_grad(const float* logits_nchw, const int64_t* target,
                            const void* workspace, size_t workspace_bytes, const float* upstream,
                            float* dlogits_nchw, int N, int H, int W, int ignore_index,
                            unet_stream_t stream);

/* The same loss over a batch SHARDED across processes (data parallel, SURVEY.md 8e
 * "global-exact"): the value and gradient of SimpleLoss on the concatenated batch.
 * shard_stats leaves per-image sums in `workspace` and writes stats[10] (device, double) =
 * {class counts[3], per-class NLL sums[3], valid pixels, sum over images of Dice[3]}; the host
 * sums stats over the shards (one 80-byte all-reduce) and passes the result, with the global
 * image count, to shard_apply together with the SAME workspace.  loss_out is identical on every
 * shard; dlogits already carry the global normalisation, so parameter gradients are SUMMED
 * (not averaged) across shards. */
int unet_dice_wce_loss_shard_stats(const float* logits_nchw, const int64_t* target, double* stats,
                                   void* workspace, size_t workspace_bytes, int N, int H, int W,
                                   float smooth, int ignore_index, unet_stream_t stream);
int unet_dice_wce_loss_shard_apply(const float* logits_nchw, const int64_t* target,
                                   const double* global_stats, int N_global, float* loss_out,
                                   float* dlogits, void* workspace, size_t workspace_bytes, int N,
                                   int H, int W, float smooth, float w_dice, float w_ce,
                                   int ignore_index, int dynamic_weights,
                                   const float* class_weights, float grad_scale,
                                   unet_stream_t stream);

/* ---- validation metrics and input pipeline ------------------------- */

/* preds[N][H][W] (uint8, optional) = argmax over the class planes; counts[9] (uint64, device) =
 * per class {intersection, predicted, labelled} over the batch, ignore_index pixels excluded:
 * the integers behind the Dice scores of validate() (Our_UNet/src/train.py:556-577).
 * target == NULL and counts == NULL: prediction only (the argmax of src/evaluate.py:185-207). */
int unet_argmax_dice_counts(const float* logits_nchw, const int64_t* target, uint8_t* preds,
                            uint64_t* counts, int N, int H, int W, int ignore_index,
                            unet_stream_t stream);

/* uint8-target twins of the loss and metric entry points above: `target` is the dataset's uint8
 * mask [N,H,W] itself (1 byte per pixel instead of 8), raw or cleaned - the dataset's rule
 * v > 2 && v != 255 -> 0 (Our_UNet/src/train.py:300) is applied on load and is the identity on a
 * cleaned mask.  Arguments, outputs and workspace layout are those of the int64 forms, and so are
 * the results, bit for bit, on the cleaned mask widened to int64 (the kernels are the same
 * templates; the workspaces of the two forms are interchangeable).  ignore_index must lie in
 * 3..255: anything else is UNET_E_INVALID before a launch.  unet_argmax_dice_counts_u8 takes four
 * pixels per lane - one 4-byte label load, 16-byte logit loads - when H*W % 4 == 0 and the
 * tensors are 16- / 4-byte aligned; the loss kernels keep the int64 forms' one pixel per lane,
 * whose summation order and fused multiply-adds are the bits of the loss and of dlogits. */
int unet_dice_wce_loss_fwd_bwd_u8(const float* logits_nchw, const uint8_t* target, float* loss_out,
                                  float* dlogits_nchw, void* workspace, size_t workspace_bytes,
                                  int N, int H, int W, float smooth, float w_dice, float w_ce,
                                  int ignore_index, int dynamic_weights,
                                  const float* class_weights, float grad_scale,
                                  unet_stream_t stream);
int unet_dice_wce_loss_grad_u8(const float* logits_nchw, const uint8_t* target,
                               const void* workspace, size_t workspace_bytes,
                               const float* upstream, float* dlogits_nchw, int N, int H, int W,
                               int ignore_index, unet_stream_t stream);
int unet_dice_wce_loss_shard_stats_u8(const float* logits_nchw, const uint8_t* target,
                                      double* stats, void* workspace, size_t workspace_bytes,
                                      int N, int H, int W, float smooth, int ignore_index,
                                      unet_stream_t stream);
int unet_dice_wce_loss_shard_apply_u8(const float* logits_nchw, const uint8_t* target,
                                      const double* global_stats, int N_global, float* loss_out,
                                      float* dlogits, void* workspace, size_t workspace_bytes,
                                      int N, int H, int W, float smooth, float w_dice, float w_ce,
                                      int ignore_index, int dynamic_weights,
                                      const float* class_weights, float grad_scale,
                                      unet_stream_t stream);
int unet_argmax_dice_counts_u8(const float* logits_nchw, const uint8_t* target, uint8_t* preds,
                               uint64_t* counts, int N, int H, int W, int ignore_index,
                               unet_stream_t stream);

/* ---- test-set evaluation (Our_UNet/src/evaluate.py:150-268) -------------------------------- */

/* cm[B][3][3] (uint64, device; zeroed here) = per image, the confusion matrix
 * [target class][predicted class] of the argmax map (first maximum wins) and the mask, BOTH
 * resized with nearest-neighbour interpolation to that image's original size: the integers
 * behind every metric of evaluate_model (src/evaluate.py:189-211) and behind its
 * plot_confusion_matrix.  dims[B][2] = (orig_h, orig_w) is a DEVICE array (what the default
 * collate makes of the dataset's original_dims, src/train.py:314) and is never read on the host;
 * NULL = at network size.  The source index of output index d is ATen's, in fp32:
 * min((int)floorf((float)d * ((float)in / (float)out)), in - 1).  Pixels whose (resized) target
 * is ignore_index, or is not a class, are excluded.  An entry of dims outside 1..16384 gives
 * that image zero counts.  H * W <= 2^30; ignore_index must not be 0, 1 or 2. */
int unet_eval_confusion(const float* logits_nchw, const int64_t* target, const int64_t* dims,
                        uint64_t* cm, int B, int H, int W, int ignore_index,
                        unet_stream_t stream);

/* ---- K classes, 2 <= K <= UNET_MAX_CLASSES: loss, counts, confusion ---------------------------
 * The entry points above are the pet trimap's 3 classes and have no K argument; these carry it.
 * Definitions are the reference's with 3 replaced by K (Our_UNet/models/losses.py:24-121):
 * dynamic weights total / count (count 0 -> 1) renormalised to sum K, weighted CE over the valid
 * pixels, soft Dice averaged over the images and then over the K classes.
 * K == 3 IS the 3-class call: every entry point of this block then runs the kernels of its
 * counterpart above (loss_reduce / loss_finalize / loss_grad, argmax_counts_kernel with its
 * four-pixel form, eval_confusion_kernel with its vector form) and gives its bits, and the
 * entry points above are these at K == 3.  A workspace sized by either
 * unet_dice_wce_loss_workspace_bytes(N, H, W) or unet_dice_wce_lossk_workspace_bytes(N, 3, H, W)
 * (equal for the N both admit) serves both, the sharded pair included.  Any other K runs the
 * K-class kernels, instantiated for K padded to 4, 8, 16 or 32.
 * One difference between the two kernel sets is visible at K == 3, in the `_u8` forms: the
 * 3-class loaders clean a raw mask with the dataset's literal rule v > 2 && v != 255 -> 0, the
 * K-class loaders with v >= K && v != ignore_index -> 0.  The two agree for ignore_index == 255,
 * the value the Python surface passes with uint8 targets at 3 classes; for another ignore_index
 * in 3..254 the 3-class loaders read a byte equal to ignore_index as class 0 and a byte 255 as a
 * valid pixel of no class, where the K-class loaders ignore the former and read the latter as
 * class 0.
 *   loss_out     float[3 + K] = {loss, CE, Dice, w[0..K-1]}
 *   class_weights K floats on the device (dynamic_weights == 0; NULL = unweighted)
 *   workspace     unet_dice_wce_lossk_workspace_bytes(N, K, H, W); kept by the caller between
 *                 a dlogits == NULL call and unet_dice_wce_lossk_grad, whose dlogits are
 *                 upstream * those of the one-call form (bit-identical for upstream == 1)
 * Three launches (per-workgroup sums, one finalize workgroup in double, gradient), no float
 * atomics: results are bit-reproducible.  The `_u8` forms take the dataset's uint8 mask and clean
 * it on load with v >= K && v != ignore_index -> 0; they need ignore_index in K..255 and give the
 * int64 forms' bits on a cleaned mask.  An int64 label outside 0..K-1 that is not ignore_index
 * counts as a valid pixel of no class.
 * Limits, UNET_E_INVALID before any launch: K outside 2..32; N > 1024 images per call (the
 * finalize keeps its N (4K + 1) sums in the workspace, not in LDS, so the limit does not depend
 * on K); K * H * W >= 2^31. */
size_t unet_dice_wce_lossk_workspace_bytes(int N, int K, int H, int W);
int unet_dice_wce_lossk_fwd_bwd(const float* logits_nchw, const int64_t* target, float* loss_out,
                                float* dlogits_nchw, void* workspace, size_t workspace_bytes,
                                int N, int K, int H, int W, float smooth, float w_dice, float w_ce,
                                int ignore_index, int dynamic_weights, const float* class_weights,
                                float grad_scale, unet_stream_t stream);
int unet_dice_wce_lossk_fwd_bwd_u8(const float* logits_nchw, const uint8_t* target,
                                   float* loss_out, float* dlogits_nchw, void* workspace,
                                   size_t workspace_bytes, int N, int K, int H, int W,
                                   float smooth, float w_dice, float w_ce, int ignore_index,
                                   int dynamic_weights, const float* class_weights,
                                   float grad_scale, unet_stream_t stream);
int unet_dice_wce_lossk_grad(const float* logits_nchw, const int64_t* target,
                             const void* workspace, size_t workspace_bytes, const float* upstream,
                             float* dlogits_nchw, int N, int K, int H, int W, int ignore_index,
                             unet_stream_t stream);
int unet_dice_wce_lossk_grad_u8(const float* logits_nchw, const uint8_t* target,
                                const void* workspace, size_t workspace_bytes,
                                const float* upstream, float* dlogits_nchw, int N, int K, int H,
                                int W, int ignore_index, unet_stream_t stream);

/* preds[N][H][W] (uint8, optional) = argmax over the K class planes, first maximum wins;
 * counts[K][3] (uint64, device; zeroed here) = per class {intersection, predicted, labelled},
 * ignore_index pixels excluded.  target == NULL and counts == NULL: prediction only.
 * N <= 65535. */
int unet_argmax_countsk(const float* logits_nchw, const int64_t* target, uint8_t* preds,
                        uint64_t* counts, int N, int K, int H, int W, int ignore_index,
                        unet_stream_t stream);
int unet_argmax_countsk_u8(const float* logits_nchw, const uint8_t* target, uint8_t* preds,
                           uint64_t* counts, int N, int K, int H, int W, int ignore_index,
                           unet_stream_t stream);

/* unet_eval_confusion for K classes: cm[B][K][K] (uint64, device; zeroed here), the same dims
 * rule and limits; ignore_index must not be a class index 0..K-1. */
int unet_eval_confusionk(const float* logits_nchw, const int64_t* target, const int64_t* dims,
                         uint64_t* cm, int B, int K, int H, int W, int ignore_index,
                         unet_stream_t stream);

/* One read of the logits, any subset of (NULL skips an output):
 *   probs[B][3][H][W]  fp32 softmax over the classes (visualize_confidence_maps_batch,
 *                      utils/visualize.py:117-119)
 *   classes[B][H][W]   uint8 argmax
 *   errors[B][H][W]    uint8 category of create_error_visualization (utils/visualize.py:205-222),
 *                      255 in the mask read as background: 0 none, 1 true positive, 2 false
 *                      positive, 3 false negative, 4 wrong class.  Needs target. */
int unet_eval_maps(const float* logits_nchw, const int64_t* target, float* probs,
                   uint8_t* classes, uint8_t* errors, int B, int H, int W, unet_stream_t stream);

/* ---- mask post-processing (postprocess.hip): components, vote, hole fill ------------
 * All integers.  The input is a uint8 class map [B][H][W] on the device (what unet_eval_maps /
 * unet_argmax_countsk write) with K classes, 2 <= K <= UNET_MAX_CLASSES; a byte >= K reads as 0;
 * class 0 is background; images never interact.
 *
 * Components.  unet_cc_label_u8 writes labels[B][H][W] and areas[B][H][W] (uint32):
 *   mode UNET_CC_FOREGROUND  selects pixels != 0; neighbours join whatever their class
 *   mode UNET_CC_CLASS       selects pixels != 0; neighbours join only if their bytes are equal
 *   mode UNET_CC_BACKGROUND  selects pixels == 0
 *   connectivity             4 or 8
 *   labels  0 on unselected pixels, otherwise 1 + (y0 * W + x0) with (y0, x0) the component's
 *           first pixel in raster order within its image (ranking the distinct labels in
 *           increasing order gives the numbering of scipy.ndimage.label)
 *   areas   the component's pixel count at that first pixel, 0 everywhere else
 *
 * Cleanup.  unet_mask_cleanup_u8 applies, in this order, each step skipped when it is off:
 *   1. removal  (keep_largest != 0 or min_area > 0)  the foreground components (connectivity)
 *      with area < min_area become 0; with keep_largest every component but the largest becomes
 *      0, ties to the smaller label; the largest is chosen among ALL components, so an image
 *      whose largest component is below min_area ends up empty.
 *   2. vote  counts the surviving foreground pixels per class 1..K-1, ties to the lower class.
 *      UNET_VOTE_IMAGE: every foreground pixel of an image takes the image's winning class (an
 *      image without foreground is unchanged).  UNET_VOTE_COMPONENT: every foreground component
 *      (the same components as in step 1) takes its own winning class.
 *   3. holes  (fill_holes != 0)  the background of the current map is labelled with the DUAL
 *      connectivity (4 when the foreground uses 8, 8 when it uses 4).  A background component that
 *      touches no image edge and has area <= max_hole_area (0 = any area) is a hole and takes the
 *      class of the pixel immediately left of the hole's first raster pixel, read from the map as
 *      it stood before step 3.  That pixel exists and is foreground: the first pixel of a hole
 *      that touches no edge has x > 0, and a background left neighbour would belong to the same
 *      hole (left is a neighbour under both connectivities) and precede it in raster order.
 * With every step off the call copies the map, bytes >= K becoming 0.  classes_in == classes_out
 * is allowed.
 *
 * Nothing is read back on the host.  Every data-dependent loop in the kernels is bounded (H * W
 * steps suffice); on overrun a kernel sets the uint32 status word at offset 0 of the workspace
 * (zeroed by every call, 0 = all loops ended by themselves) and leaves; the caller reads the word
 * if and when it wants to.  Workspaces: 4 bytes a pixel for the labelling, 16 bytes a pixel for
 * the cleanup, plus O(B) words, independent of K; 0 is returned for a shape outside the limits.
 * UNET_E_INVALID before any launch: a null pointer; B outside 1..65535; K outside 2..32; H or W
 * outside 1..16384 or H * W > 2^30; connectivity not 4 or 8; an unknown mode or vote; a negative
 * area; a workspace that is too small. */
#define UNET_CC_FOREGROUND 0
#define UNET_CC_CLASS 1
#define UNET_CC_BACKGROUND 2
#define UNET_VOTE_NONE 0
#define UNET_VOTE_IMAGE 1
#define UNET_VOTE_COMPONENT 2
size_t unet_cc_workspace_bytes(int B, int H, int W);
int unet_cc_label_u8(const uint8_t* classes, uint32_t* labels, uint32_t* areas, void* workspace,
                     size_t workspace_bytes, int B, int K, int H, int W, int connectivity,
                     int mode, unet_stream_t stream);
size_t unet_mask_cleanup_workspace_bytes(int B, int K, int H, int W);
int unet_mask_cleanup_u8(const uint8_t* classes_in, uint8_t* classes_out, void* workspace,
                         size_t workspace_bytes, int B, int K, int H, int W, int connectivity,
                         int vote, int keep_largest, int min_area, int fill_holes,
                         int max_hole_area, unet_stream_t stream);

/* unet_eval_confusionk with the class map given instead of the logits: preds[B][H][W] uint8 (a
 * byte >= K reads as 0) takes the place of the argmax; the same dims rule, the same counts, the
 * same limits (H, W <= 16384 here); ignore_index must not be a class index 0..K-1. */
int unet_eval_confusion_classes(const uint8_t* preds, const int64_t* target, const int64_t* dims,
                                uint64_t* cm, int B, int K, int H, int W, int ignore_index,
                                unet_stream_t stream);

/* ---- evaluation pictures (render.hip) -------------------------------------------------------
 * The tiles of the reference's figure functions as uint8 RGB, on the device; titles, legends and
 * colour bars are not drawn. */

/* panel ids of unet_render_seg_panels */
#define UNET_RENDER_IMAGE 0  /* the input image as bytes */
#define UNET_RENDER_GT 1     /* colorize_mask(mask): 1 red, 2 green, anything else black */
#define UNET_RENDER_PRED 2   /* colorize_mask(argmax), first maximum wins */
#define UNET_RENDER_ERROR 3  /* create_error_visualization: (image + category colour) >> 1 */
#define UNET_RENDER_CONF0 4  /* confidence overlay of class 0 .. 2: (image + jet[idx(p)]) >> 1 */
#define UNET_RENDER_CONF1 5
#define UNET_RENDER_CONF2 6
#define UNET_RENDER_TARGET 7 /* (image + c) >> 1, c = (103,0,12) where mask == target_class, else
                                (255,245,240): the two ends of matplotlib's Reds */
#define UNET_RENDER_HEAT 8   /* Grad-CAM overlay: (image + jet[idx(heat)]) >> 1 */

/* out[B][H][P][W][3] (uint8) = the P requested panels of every image side by side - the same
 * memory as the picture [B * H][P * W][3] of the whole batch.  One launch.
 *   image   image_is_u8 == 0: fp32 [B][3][H][W] normalised with the ImageNet mean / std; a byte is
 *           trunc(clip(double(x) * std + mean, 0, 1) * 255), each operation rounded to double
 *           in that order (Our_UNet/utils/visualize.py:60-62, :277).  image_is_u8 != 0: uint8
 *           [B][H][W][3], the bytes themselves.
 *   logits  fp32 [B][3][H][W]; NULL allowed when no panel needs it (pred, error, conf0..2 do).
 *   mask    int64 [B][H][W], or uint8 with mask_is_u8 != 0; NULL allowed when no panel needs it
 *           (gt, error, target do).  In the error panel 255 reads as background.
 *   heat    fp32 [B][H][W]; NULL allowed without the heat panel.
 *   jet     uint8 [256][3], the colour table of the overlays; idx(v) = min((int)(v * 256), 255)
 *           of v clipped to [0, 1], NaN reading as 0 (matplotlib's rule).  The confidence p is
 *           the fp32 softmax of unet_eval_maps.
 *   panels  the ordered list, 4 bits per panel from bit 0: id + 1; the first zero nibble ends it;
 *           1 to 9 panels, an id may repeat.
 * All blends are the truncating half-sum per byte.  UNET_E_INVALID before the launch: a null
 * image / jet / out, a bad shape (B in 1..65535, H * W <= 2^30), an empty, too long or unknown
 * panel list, a panel whose operand is NULL. */
int unet_render_seg_panels(const void* image, int image_is_u8, const float* logits_nchw,
                           const void* mask, int mask_is_u8, const float* heat, const uint8_t* jet,
                           int target_class, uint64_t panels, uint8_t* out, int B, int H, int W,
                           unet_stream_t stream);

/* out[B][H][3][W][3] (uint8) = original | reconstruction | error map: create_comparison_image on
 * denormalize_image without mean / std (AE_pretrained/reconstruction/utils/visualize.py:16-95).
 *   original  fp32 [B][3][H][W] in [0, 1] - a byte is trunc(clamp(x, 0, 1) * 255) with an fp32
 *             multiply - or, with original_is_u8 != 0, uint8 [B][H][W][3].
 *   recon     fp32 [B][3][H][W], converted the same way.
 *   error map d = |original byte - reconstruction byte| per channel; m = the maximum of d over the
 *             whole image, PER IMAGE; e = trunc(d / m * 255), the division and then the product
 *             each rounded to fp32 (all zero if m = 0);
 *             gray = (4899 e_R + 9617 e_G + 1868 e_B + 8192) >> 14; colour = jet[gray], RGB.
 *   maxima    uint32 [B] scratch: cleared on the stream, then holds m.
 * Two launches (the integer maximum, then the picture). */
int unet_render_recon_panels(const void* original, int original_is_u8, const float* recon_nchw,
                             const uint8_t* jet, uint32_t* maxima, uint8_t* out, int B, int H,
                             int W, unet_stream_t stream);

/* ---- online batch augmentation (augment.hip; semantics defined by this project) -- */

/* Floats per sample record of unet_augment_u8 (24). */
int unet_augment_params_per_sample(void);

/* image [N][H][W][3] + mask [N][H][W] (uint8, mask nullable: then mask_out is not written) ->
 * an augmented pair of the same shape, one launch, grid (pixel tiles, N).  params [N][24] (fp32)
 * and rng [N][4] (uint32, nullable: then all noise is off) are DEVICE arrays read by the kernel
 * only, so a launch captured in a HIP graph follows new records on replay.  The outputs must not
 * overlap the inputs (the kernel gathers).  Record, levels 0..255 where a value is a pixel value:
 *    0-8   h0..h8  inverse homography, row-major: output pixel centre -> source coordinate
 *    9     alpha (contrast gain)        10-12  beta_c per channel (brightness 255 + RGB shift)
 *    13    gray flag (0 / 1)            14     sigma of the Gaussian noise (0 = off)
 *    15-18 hole x0, y0, x1, y1 in output pixels, half-open; empty if x1 <= x0 or y1 <= y0
 *    19    hole fill (image)   20  mask border fill   21  mask hole fill   22-23  reserved, 0
 * rng[n] = seed_lo, seed_hi, pepper_thr, salt_thr.
 * Every fp32 operation below is rounded on its own (no fused multiply-add).  Output pixel (i, j):
 *    xc = j + 0.5, yc = i + 0.5, den = (h6 xc + h7 yc) + h8,
 *    u = ((h0 xc + h1 yc) + h2) / den, v = ((h3 xc + h4 yc) + h5) / den.
 * Image: fx = u - 0.5, x0 = floor(fx), ax = fx - x0 (the same in y); taps (y0,x0), (y0,x0+1),
 * (y0+1,x0), (y0+1,x0+1), a tap outside the image contributes 0 (and a pixel none of whose taps
 * is inside is exactly 0); top = (1-ax) p00 + ax p01, bot = (1-ax) p10 + ax p11,
 * s = (1-ay) top + ay bot.  Mask: source (floor(v), floor(u)), the border fill outside.  A pixel
 * with !(den > 0) is outside for both.  All range tests are made in float before any conversion.
 * Inside the hole s_c is the hole fill and the mask the mask hole fill.  Then, in this order:
 *    a_c = clamp(alpha s_c + beta_c, 0, 255);  gray: a_c = (0.299 a_0 + 0.587 a_1) + 0.114 a_2;
 *    sigma > 0: a_c += sigma z_c;  q_c = clamp(rint(a_c), 0, 255);
 *    pepper (0, 0, 0) if the pixel's word < pepper_thr, else salt (255 x 3) if salt_thr != 0 and
 *    word >= 2^32 - salt_thr.
 * Random words: Philox4x32-10, key (seed_lo, seed_hi), counter (pixel index lo, hi, stream, 0)
 * with the pixel index i W + j inside the sample.  Stream 0: words w0..w3 give the normals by
 * Box-Muller on (w0, w1) and (w2, w3): u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24,
 * r = sqrt(-2 ln u1), z_0 = r cos(2 pi u2), z_1 = r sin(2 pi u2) of the first pair, z_2 the
 * cosine of the second.  Stream 1: word 0 is the salt / pepper word.
 * UNET_E_INVALID before any launch: null image / image_out / params, a mask without mask_out,
 * N, H or W <= 0 (or N > 65535, H or W > 32768, H W > 2^30), an output overlapping an input. */
int unet_augment_u8(const uint8_t* image, const uint8_t* mask, uint8_t* image_out,
                    uint8_t* mask_out, const float* params, const uint32_t* rng, int N, int H,
                    int W, unet_stream_t stream);

/* ---- elastic, grid and optical distortion: a per-pixel warp in front of the homography ------ */

/* Floats per sample record `warp` of unet_augment_warp_u8 / unet_elastic_field (64). */
int unet_augment_warp_params_per_sample(void);

/* unet_augment_u8 behind a warp stage (normative text).  The warp acts in the OUTPUT
 * frame, before the homography: output pixel (i, j) with centre xc = j + 0.5, yc = i + 0.5 goes
 * through the stage below to (xw, yw), and from there on everything of the unet_augment_u8 comment
 * holds with (xw, yw) in place of (xc, yc) in den, u and v.  The hole test stays on the integer
 * output pixel (i, j), the random counters on the output pixel index i W + j, and the mask is
 * sampled at (floor(v), floor(u)) of the same warped coordinates.  Every fp32 operation is rounded
 * on its own, in the order the parentheses give; range tests are made in float before any
 * conversion; !(den > 0) is outside.
 * warp [N][64] (fp32, DEVICE, read by the kernels only): value 0 is the mode, 1.. the mode's
 * numbers, every value a mode does not name is 0:
 *   mode 0, none:    (xw, yw) = (xc, yc): the bytes of unet_augment_u8 on the same params / rng.
 *                    Any mode value other than 1, 2, 3 is treated as 0.
 *   mode 1, elastic: 1-6 a0..a5, 7 alpha (pixels), 8 R (radius, 0..16), 9-25 g[0..16] (taps of the
 *                    Gaussian, g[t] = 0 for t > R).
 *                      xw = (((a0 xc) + (a1 yc)) + a2) + dx(i, j)
 *                      yw = (((a3 xc) + (a4 yc)) + a5) + dy(i, j)
 *                    (dx, dy) = field[n][i][j][0..1] as unet_elastic_field wrote it; 0 with a
 *                    null field.  alpha, R and g are read by unet_elastic_field only.
 *   mode 2, grid:    1 Kx, 2 invcell_x, 3 Ky, 4 invcell_y, 8-15 ax_k, 16-23 bx_k, 24-31 ay_k,
 *                    32-39 by_k (k < K; 1 <= K <= 8).  Per axis, independently:
 *                      k = min((int)floor(xc invcell_x), Kx - 1),  xw = (ax_k xc) + bx_k
 *                    and the same in y with yc.  (On the device the cell index is clamped to
 *                    0..7 in float first, so a record never indexes past its 64 floats.)
 *   mode 3, optical: 1 cx, 2 cy, 3 k, 4 iw = 1/W, 5 ih = 1/H (rounded to fp32 by the host).
 *                      ex = xc - cx, ey = yc - cy, xn = ex iw, yn = ey ih,
 *                      r2 = (xn xn) + (yn yn),  f = (1 + (k r2)) + ((k r2) r2),
 *                      xw = cx + (ex f),  yw = cy + (ey f).
 * field [N][H][W][2] (fp32, nullable, 8-byte aligned) is read for the samples of mode 1 only.
 * UNET_E_INVALID before any launch: as unet_augment_u8, and a null warp, a misaligned field, an
 * output overlapping warp or field. */
int unet_augment_warp_u8(const uint8_t* image, const uint8_t* mask, uint8_t* image_out,
                         uint8_t* mask_out, const float* params, const uint32_t* rng,
                         const float* warp, const float* field, int N, int H, int W,
                         unet_stream_t stream);

/* The displacement field of the elastic samples: field[n][i][j][0..1] = (dx, dy) in pixels
 * (fp32), written for the samples whose warp record has mode 1 ONLY - the workgroups of every
 * other sample return at once and leave their slice of `field` untouched, so the launch is the
 * same for every batch and a captured one follows new records.  Grid (32 x 32 tiles, N), 48 KB LDS.
 *   noise      n_c(i, j) = (2 u) - 1, u = (word_c >> 8) 2^-24, c = 0 (x), 1 (y): words 0 and 1 of
 *              Philox4x32-10 STREAM 2, key (seed_lo, seed_hi) of rng[n], counter (pixel index lo,
 *              hi, 2, 0) with the pixel index i W + j.  At a position outside the image the noise
 *              is exactly 0.  With rng == NULL all noise is 0 and so is the field.
 *   smoothing  separable Gaussian of radius R, one-sided taps g[0..R] from the record (the host
 *              computes them in fp64 - exp(-t^2 / (2 sigma^2)), normalised so that g[0] + 2 sum
 *              g[1..R] = 1 - and rounds them to fp32; the device evaluates no exp);
 *              R = min(ceil(3 sigma), 16).
 *   row pass   r_c(i, j) = sum over t = -R..R, ascending, from 0.f, of g[|t|] n_c(i, j + t): each
 *              product and each sum rounded on its own; rows outside the image give 0.
 *   column     d_c(i, j) = alpha * (the same sum over r_c(i + t, j)).
 * UNET_E_INVALID before any launch: null field / warp, a bad shape (as unet_augment_u8), a field
 * that is not 8-byte aligned or overlaps warp / rng. */
int unet_elastic_field(float* field, const float* warp, const uint32_t* rng, int N, int H, int W,
                       unet_stream_t stream);

/* ---- HSV shift, equalize / CLAHE and blur: a second stage behind the gather ------ */

/* Floats per sample record `post` of unet_augment_post_u8 (64). */
int unet_augment_post_params_per_sample(void);

/* Bytes of the workspace unet_augment_post_u8 needs for N samples: counts [N][3][256] uint32, then
 * LUTs [N][64][256] bytes.  0 for N <= 0. */
size_t unet_augment_post_workspace_bytes(int N);

/* image [N][H][W][3] (uint8) -> image_out of the same shape (normative text).  post
 * [N][64] (fp32) and rng [N][4] (uint32, nullable: then there is no salt / pepper) are DEVICE arrays
 * read by the kernels only, and the launch sequence (one memset of the counts, the histogram kernel,
 * the apply kernel) is the same for every batch, so a captured sequence follows new records on
 * replay.  image_out must not overlap image, post, rng or workspace.  Record; every value a mode
 * does not name is 0:
 *    0      HSV on: exactly 1; any other value is off
 *    1-3    dh, ds, dv: hue in half-degrees (h in [0, 180)), saturation and value in levels 0..255
 *    4      histogram op: 1 equalize, 2 CLAHE; any other value is none
 *    5      CLAHE clip_limit          6, 7   CLAHE tile grid ty, tx (integers in 1..8)
 *    8      blur: 1 separable, 2 dense; any other value is none
 *    9      radius R: clamped IN FLOAT to 1..4 (separable) or 1..3 (dense), then truncated
 *    10-14  one-sided separable taps g[0..4]
 *    15-63  dense weights w, row-major over (2R+1)^2 <= 49: index 15 + (dy+R)(2R+1) + (dx+R)
 * rng[n] = seed_lo, seed_hi, pepper_thr, salt_thr as for unet_augment_u8.
 * Every fp32 operation is rounded on its own (no fused multiply-add), in the order the parentheses
 * give; fmin / fmax return the other operand for a NaN; byte(x) = clamp(rint(x), 0, 255); all range
 * tests are made in float before any conversion to an index.  Per sample, in this order:
 *    input byte p_c -> HSV -> byte -> histogram op -> byte -> blur -> byte -> salt / pepper.
 * HSV (skipped entirely unless value 0 is 1), with r, g, b = (float)p_0..2:
 *    V = max(r, g, b), m = min(r, g, b), d = V - m, S = (V == 0) ? 0 : (255 d) / V;
 *    h = 0 if d == 0, else by the channel that is the maximum (ties: r, then g):
 *      r: 30 ((g - b) / d)     g: 60 + (30 ((b - r) / d))     b: 120 + (30 ((r - g) / d));
 *    h < 0: h = h + 180.
 *    h' = h + dh, h' = h' - (180 floor(h' / 180)), h' = fmin(fmax(h', 0), 180 - 2^-16) (the largest
 *    float below 180);  S' = fmin(fmax(S + ds, 0), 255);  V' = fmin(fmax(V + dv, 0), 255).
 *    c = (V' S') / 255, hp = h' / 30, k = fmin(fmax(floor(hp), 0), 5), f = hp - k,
 *    P = V' - c, Q = V' - (c f), T = V' - (c (1 - f));  (r, g, b)' by k = 0..5:
 *      (V',T,P) (Q,V',P) (P,V',T) (P,Q,V') (T,P,V') (V',P,Q);   q_c = byte(that).
 * Equalize (op 1), per channel over the whole sample of the q_c: hist the 256-bin histogram, i0 the
 *    first non-empty bin, total = H W.  hist[i0] == total: the channel is unchanged.  Otherwise
 *    scale = 255.f / (float)(total - hist[i0]), lut[i] = 0 for i <= i0, and for i > i0 with
 *    sum = hist[i0+1] + .. + hist[i]:  lut[i] = min(255, (int)rint((float)sum scale)).
 * CLAHE (op 2) on luma Y = (int)byte(((0.299 q_0) + (0.587 q_1)) + (0.114 q_2)).  The grid (ty, tx)
 *    must be two integers in 1..8 with H % ty == 0 and W % tx == 0; a record where it is not is
 *    treated as "no histogram op".  Tiles are th = H / ty by tw = W / tx, area = th tw.  Per tile,
 *    in integers: hist of Y;  t = fmax(floor((clip_limit (float)area) / 256.f), 1),
 *    climit = (t >= (float)area) ? area : (int)t;  excess = sum max(hist_i - climit, 0),
 *    hist_i = min(hist_i, climit);  batch = excess / 256, resid = excess - 256 batch,
 *    hist_i += batch;  if resid > 0: step = max(256 / resid, 1) and hist_i += 1 for the i with
 *    i % step == 0 and i / step < resid;  cdf the inclusive sum,
 *    L_i = min(255, (int)rint((float)cdf_i (255.f / (float)area))).
 *    Pixel (i, j): fx = ((float)j (1.f / (float)tw)) - 0.5, x1 = floor(fx), ax = fx - x1,
 *    x2 = x1 + 1, then x1 and x2 clamped to 0 .. tx - 1; the same in y with i, th, ty.
 *    top = ((1 - ax) L[y1][x1][Y]) + (ax L[y1][x2][Y]), bot the same with y2,
 *    s = ((1 - ay) top) + (ay bot), Y' = (int)byte(s), out_c = clamp(q_c + (Y' - Y), 0, 255).
 * Blur over the bytes B after the histogram op.  Borders reflect without repeating the edge
 *    (x < 0: -x; x > W - 1: 2 (W - 1) - x), the result then clamped to 0 .. W - 1; rows likewise.
 *    Separable (1): row(i, j) = sum over t = -R..R, ascending, from 0.f, of g[|t|] (float)B(i, j+t),
 *    each product and each sum rounded on its own, kept in fp32;  out = byte(the same sum over
 *    t of g[|t|] row(i+t, j)).  Dense (2): out = byte(sum over dy = -R..R, then dx = -R..R, both
 *    ascending, from 0.f, of w[dy][dx] (float)B(i+dy, j+dx)).
 * Salt / pepper last, with the rule and the Philox stream-1 word of the output pixel index i W + j
 * of unet_augment_u8.  A sample with nothing on is copied.
 * workspace: unet_augment_post_workspace_bytes(N) bytes, 16-byte aligned, scratch of this call.
 * UNET_E_INVALID before any launch: null image / image_out / post, a bad shape (as
 * unet_augment_u8), a null, too small or misaligned workspace, image_out overlapping an input or
 * the workspace, the workspace overlapping an input. */
int unet_augment_post_u8(const uint8_t* image, uint8_t* image_out, const float* post,
                         const uint32_t* rng, void* workspace, size_t workspace_bytes, int N, int H,
                         int W, unet_stream_t stream);

/* The two halves of unet_augment_post_u8, for a caller that measures or overlaps them: the
 * histogram half (the memset of the counts and the histogram kernel) fills the workspace the apply
 * half reads; hist followed by apply on one stream, with the same arguments, is
 * unet_augment_post_u8.  The same refusals. */
int unet_augment_post_hist(const uint8_t* image, const float* post, void* workspace,
                           size_t workspace_bytes, int N, int H, int W, unet_stream_t stream);
int unet_augment_post_apply(const uint8_t* image, uint8_t* image_out, const float* post,
                            const uint32_t* rng, void* workspace, size_t workspace_bytes, int N,
                            int H, int W, unet_stream_t stream);

/* ---- ISO noise, shadow, sun flare and fog: a third stage (augment_light.hip) ------- */

/* Floats per sample record `light` of unet_augment_light_u8 (272). */
int unet_augment_light_params_per_sample(void);

/* Bytes of the workspace unet_augment_light_u8 needs for N samples: sums [N][2] uint64.  0 for
 * N <= 0. */
size_t unet_augment_light_workspace_bytes(int N);

/* image [N][H][W][3] (uint8) -> image_out of the same shape (normative text).  light
 * [N][272] (fp32) and rng [N][4] (uint32, nullable: then ISO noise is off) are DEVICE arrays read
 * by the kernels only, and the launch sequence (one memset of the sums, the statistics kernel, the
 * apply kernel) is the same for every batch, so a captured sequence follows new records on replay.
 * image_out must not overlap image, light, rng or workspace.  Record; every value a mode does not
 * name is 0; x runs along W, y along H, in output pixels:
 *    0      ISO noise on: exactly 1; any other value is off
 *    1      sigma_h, the standard deviation of the hue noise in degrees      2   intensity
 *    3      mode: 1 shadow, 2 sun flare, 3 fog; any other value is none
 *    4      count: polygons (shadow), secondary circles (flare), points (fog).  Clamped IN FLOAT to
 *           0..2, 0..10 or 0..128 (a NaN is 0), then truncated; 0 polygons leave the sample as it is
 *    shadow 16 + 10 p + 2 v, + 1: vertex v = 0..4 of polygon p as (x, y)
 *    flare  5, 6 the source centre (x, y);  7 Rs;  8 T, clamped in float to 2..40 (a NaN is 2), then
 *           truncated;  16 + 7 c ..: circle c as cx, cy, r, a, colour_0..2
 *    fog    5 the common radius;  6 a = alpha_coef fog_coef;  7 the box size k, clamped in float to
 *           1..9 (a NaN is 1), then truncated (1: no box);  16 + 2 p, + 1: point p as (x, y)
 * A radius r is used as fmax(r, 0) (a NaN is 0) and only in arithmetic.  rng[n] = seed_lo, seed_hi
 * (the two thresholds are not read).
 * Every fp32 operation is rounded on its own (no fused multiply-add), in the order the parentheses
 * give; fmin / fmax return the other operand for a NaN; byte(x) = clamp(rint(x), 0, 255); all range
 * tests are made in float before any conversion to an index or a loop bound.  Per sample:
 *    input byte p_c -> ISO noise -> byte -> one of { shadow | sun flare | fog } -> byte.
 * HLS is carried in fp64, each operation rounded on its own, and a channel that comes out of it is
 * rounded to fp32 before byte: S and the hue's fraction are quotients, and only so does the way back
 * return exactly the value that went in (a shadowed pixel with s <= 255 is exactly byte(p / 2)).
 * HLS of a pixel, r, g, b = (double)p_0..2:  V = max, m = min, s = V + m, d = V - m;  L = s / 510;
 *    S = 0 if d == 0, else d / s for s <= 255, else d / (510 - s);  H = 0 if d == 0, else by the
 *    channel that is the maximum (ties: r, then g):  r: 60 ((g - b) / d)   g: 120 + (60 ((b - r) / d))
 *    b: 240 + (60 ((r - g) / d));  H < 0: H = H + 360.
 * Back from (H, L, S), in levels:  l2 = 510 L;  c = l2 S if l2 <= 255, else (510 - l2) S;
 *    hp = H / 60, k = fmin(fmax(floor(hp), 0), 5), f = hp - k;  x = c (1 - f) for odd k, c f for even;
 *    lo = 0.5 (l2 - c), hi = lo + c, mid = lo + x;  (r, g, b) by k = 0..5:
 *      (hi,mid,lo) (mid,hi,lo) (lo,hi,mid) (lo,mid,hi) (mid,lo,hi) (hi,lo,mid);
 *    q_c = byte((float)that).
 * ISO noise (value 0 is 1 and rng is not null).  S1 = sum of s and S2 = sum of s^2 over the
 *    sample's input pixels, exact integers.  In fp64, each operation rounded on its own:  n = H W,
 *    mean = S1 / n, var = fmax((S2 / n) - (mean mean), 0), sd = sqrt(var) / 510,
 *    lambda = (float)fmin(fmax((intensity 255) sd, 0), 64).  The table, in fp32:  t_0 = 1,
 *    t_k = (t_{k-1} lambda) / k and t_k = 0 where that is below FLT_MIN;  c_k = c_{k-1} + t_k from
 *    c_0 = t_0, k = 1..255;  T = c_255.  Pixel with index i W + j: words w0..w3 of Philox4x32-10
 *    STREAM 3, key (seed_lo, seed_hi), counter (pixel index lo, hi, 3, 0).  z = the first Box-Muller
 *    normal of (w0, w1) as unet_augment_u8 forms it;  u = (w2 >> 8) 2^-24;  kp = the number of
 *    c_j <= (u T), at most 255.  In fp64, with sigma_h, z and kp converted:
 *    H' = H + (sigma_h z), H' = H' - (360 floor(H' / 360)),
 *    H' = fmin(fmax(H', 0), 360 - 2^-44) (the largest double below 360);
 *    L' = fmin(L + ((kp / 255) (1 - L)), 1);  back from (H', L', S).
 * Shadow: pixel (i, j) has the centre xc = j + 0.5, yc = i + 0.5.  Edge e of a polygon runs from
 *    vertex e = (x1, y1) to vertex (e + 1) mod 5 = (x2, y2); it is crossed where
 *    (y1 <= yc) != (y2 <= yc) (half-open in y, so a centre level with a vertex is decided once) and
 *    xc < x1 + (((yc - y1) / (y2 - y1)) (x2 - x1)).  A centre with an odd number of crossed edges is
 *    inside the polygon.  m = the number of polygons the centre is inside: m == 0 keeps the bytes;
 *    else back from (H, 0.5 L, S) for m == 1 and from (H, 0.25 L, S) for m == 2.
 * Circles (flare, fog): pixel (i, j) is inside (cx, cy, r) where
 *    (((float)j - cx)^2 + ((float)i - cy)^2) <= (fmax(r, 0) fmax(r, 0)), each square and the sum
 *    rounded; a NaN makes it outside.
 * Sun flare, per channel: ov = o = the byte.  Circle c = 0..count-1 in order: inside: ov = colour_c;
 *    then o = byte((a ov) + ((1 - a) o)).  Then i = 0..T-1:  r_i = 1 + (((Rs - 1) (float)i) /
 *    (float)(T - 1)); inside (source centre, r_i): ov = 255;  q = (float)(T - 1 - i) / (float)(T - 1),
 *    a_i = (q q) q;  o = byte((a_i ov) + ((1 - a_i) o)).
 * Fog, per channel: for point p = 0..count-1 in order, inside (point, radius):
 *    o = byte((a 255) + ((1 - a) o)).  Then for k >= 2 the k x k box mean over the fogged bytes B:
 *    offsets -(k / 2) .. k - 1 - (k / 2) per axis (integer division), borders reflect without
 *    repeating the edge (x < 0: -x; x > W - 1: 2 (W - 1) - x), the result then clamped to
 *    0 .. W - 1, rows likewise;  out = byte((sum over dy, then dx, both ascending, from 0.f, of
 *    (float)B(i + dy, j + dx)) / (float)(k k)).  A halo pixel's B is the value of the whole chain
 *    at that pixel, ISO noise included (its words depend on the pixel index only).
 * A sample with nothing on is copied.
 * workspace: unet_augment_light_workspace_bytes(N) bytes, 16-byte aligned, scratch of this call.
 * UNET_E_INVALID before any launch: null image / image_out / light, a bad shape (as
 * unet_augment_u8), a null, too small or misaligned workspace, image_out overlapping an input or
 * the workspace, the workspace overlapping an input. */
int unet_augment_light_u8(const uint8_t* image, uint8_t* image_out, const float* light,
                          const uint32_t* rng, void* workspace, size_t workspace_bytes, int N,
                          int H, int W, unet_stream_t stream);

/* The two halves of unet_augment_light_u8, for a caller that measures or overlaps them: the
 * statistics half (the memset of the sums and the statistics kernel) fills the workspace the apply
 * half reads; stats followed by apply on one stream, with the same arguments, is
 * unet_augment_light_u8.  The same refusals. */
int unet_augment_light_stats(const uint8_t* image, const float* light, void* workspace,
                             size_t workspace_bytes, int N, int H, int W, unet_stream_t stream);
int unet_augment_light_apply(const uint8_t* image, uint8_t* image_out, const float* light,
                             const uint32_t* rng, void* workspace, size_t workspace_bytes, int N,
                             int H, int W, unet_stream_t stream);

/* uint8 HWC image (+ uint8 mask) -> ((v/255) - mean)/std NHWC fp32 (+ int64 target with values
 * > 2 other than 255 mapped to 0): PetSegmentationDataset.__getitem__, src/train.py:300-311.
 * mean3 / std3 are HOST pointers to 3 floats. */
int unet_preprocess_u8(const uint8_t* image_hwc, const uint8_t* mask, float* out_nhwc,
                       int64_t* target, int N, int H, int W, const float* UNET_HOST mean3,
                       const float* UNET_HOST std3, unet_stream_t stream);

/* ---- SGD with Nesterov momentum over a flat arena -------------------------- */

/* g' = g*grad_scale + wd*p; buf = first_step ? g' : mu*buf + g'; p -= lr*(g' + mu*buf).
 * Replaces optim.SGD(lr, momentum, nesterov=True, weight_decay).step()
 * (Our_UNet/src/train.py:445-451,:664). */
int unet_sgd_nesterov_step(float* params, const float* grads, float* momentum, int64_t n,
                           float lr, float mu, float weight_decay, int first_step,
                           float grad_scale, unet_stream_t stream);

/* The same with the hyper-parameters read from DEVICE memory, hyper = {lr, mu, weight_decay,
 * grad_scale}: a train step captured in a HIP graph keeps following the learning-rate schedule
 * (the reference steps it per epoch, Our_UNet/src/train.py:940) without being re-captured. */
int unet_sgd_nesterov_step_dev(float* params, const float* grads, float* momentum, int64_t n,
                               const float* hyper, int first_step, unet_stream_t stream);

/* ---- fused layer pipeline -------------------------------------------------- */
/*
 * One ConvBlock unit of the reference is conv -> InstanceNorm2d -> LeakyReLU -> SpatialDropout2d
 * (Our_UNet/models/unet.py:101-134).  The stand-alone entry points above run it as four passes
 * over the layer tensor (conv, statistics, apply, next conv).  The fused pipeline keeps only
 * the RAW convolution output y_l of every layer in HBM:
 *   - the convolution that produces y_l emits the InstanceNorm statistics of y_l from its
 *     epilogue (per-tile (mean, M2) summaries, merged by a tiny finalize launch), and
 *   - every consumer of the activated tensor a_l = dropout(lrelu(IN(y_l))) -- the next
 *     convolution, the weight gradient of the next convolution, the bilinear up-sampling, the
 *     1x1 head -- applies  a = lrelu(y * alpha[n][c] + beta[n][c], slope)  to the operand while
 *     it stages it on chip (zero padding is applied after the activation).
 * alpha / beta are the folded coefficients the statistics finalize writes:
 *   alpha[n][c] = gamma[c] * rstd[n][c] * mask[n][c],
 *   beta [n][c] = (beta[c] - mean[n][c] * gamma[c] * rstd[n][c]) * mask[n][c]
 * (mask = the SpatialDropout2d factor 0 or 1/(1-p), folded in because lrelu(z)*m == lrelu(z*m)
 * for m >= 0).  a_l itself is never written.
 */
typedef struct unet_act_src {
  const float* x;     /* [N][H][W][C] raw convolution output, or a plain tensor (alpha == NULL) */
  int C;              /* channels: 3 (RGB image, plain only) or a multiple of 32 */
  const float* alpha; /* [N][C] folded InstanceNorm scale x dropout mask; NULL = use x as stored */
  const float* beta;  /* [N][C] folded shift; ignored when alpha == NULL */
} unet_act_src;

/* y[N][Ho][Wo][Cout] = conv_kxk(cat(act(s0), act(s1))) + bias  (ksize 3: pad 1, stride 1|2,
 * w = wf[9][Cout][Cin]; ksize 1: stride 1, w = [Cout][Cin]; s1 may be NULL).  The epilogue leaves
 * per-tile (mean, M2) summaries of y in `workspace`; *stats_px_out (HOST int) receives the pixels
 * per summary tile, or 0 when this shape has no statistics epilogue (tiny or ragged maps).
 * Replaces Conv2d (+ the previous unit's InstanceNorm apply / LeakyReLU / dropout) of ConvBlock
 * (Our_UNet/models/unet.py:101-134) and the torch.cat of UpBlock (:228).  H, W = input size. */
size_t unet_conv_in_fwd_workspace_bytes(int N, int H, int W, int Cout, int stride);
int unet_conv_in_fwd(const unet_act_src* s0, const unet_act_src* s1, float slope, const float* w,
                     const float* bias, int ksize, int stride, float* y, void* workspace,
                     size_t workspace_bytes, int* UNET_HOST stats_px_out, int N, int H, int W,
                     int Cout, unet_stream_t stream);
/* The same in the split-bf16 ("bf16x3") operand mode: fp32 tensors, fp32-class accuracy on the
 * bf16 matrix cores.  w3 = the pre-split planes of unet_pack_conv3x3_weights_bf16x3 (forward
 * layout; may be NULL for ksize 1).  Stride-1 3x3 shapes that tile as 4 x 32 pixels run the
 * split patch kernel with the activation applied before the split; other shapes run the fp32
 * kernels (same results to fp32 rounding). */
int unet_conv_in_fwd_bf16x3(const unet_act_src* s0, const unet_act_src* s1, float slope,
                            const float* w, const uint16_t* w3, const float* bias, int ksize,
                            int stride, float* y, void* workspace, size_t workspace_bytes,
                            int* UNET_HOST stats_px_out, int N, int H, int W, int Cout,
                            unet_stream_t stream);
/* InstanceNorm statistics of y [N][HoWo][Cout] from the summaries unet_conv_in_fwd left in
 * `workspace` (stats_px > 0: a few-microsecond merge) or from y itself (stats_px == 0), and the
 * folded coefficients for y's consumers: mean, rstd, alpha_out, beta_out [N][Cout]
 * (gamma / beta = the norm's affine parameters, mask [N][Cout] = this layer's dropout factors
 * or NULL).  Replaces the statistics half of nn.InstanceNorm2d (unet.py:118-119). */
int unet_conv_in_stats_finalize(const float* y, void* workspace, size_t workspace_bytes,
                                int stats_px, const float* gamma, const float* beta, float eps,
                                const float* mask, float* mean, float* rstd, float* alpha_out,
                                float* beta_out, int N, int HoWo, int Cout, unet_stream_t stream);

/* First convolution of a decoder stage with the bilinear 2x up-sampling done in the loader:
 *   y[N][H][W][Cout] = conv3x3(cat(upsample2x(act(low)), act(skip))) + bias,
 * low->x = [N][H/2][W/2][C0] raw, skip->x = [N][H][W][C1] raw: UpBlock.forward
 * (Our_UNet/models/unet.py:215-231) without the up-sampled tensor and without the concatenation.
 * Covers the shapes the patch-staged kernel tiles (unet_conv_up_in_fwd_supported != 0; H % 4,
 * W % 32, channels % 32, >= 512 tiles); otherwise use unet_upsample2x_in_fwd + unet_conv_in_fwd.
 * Workspace, *stats_px_out and the statistics finalize as unet_conv_in_fwd (stride 1). */
int unet_conv_up_in_fwd_supported(int N, int H, int W, int C0, int C1, int Cout);
int unet_conv_up_in_fwd(const unet_act_src* low, const unet_act_src* skip, float slope,
                        const float* wf, const float* bias, float* y, void* workspace,
                        size_t workspace_bytes, int* UNET_HOST stats_px_out, int N, int H, int W,
                        int Cout, unet_stream_t stream);

/* RGB stem straight from the dataset's uint8 HWC image [N][H][W][3]: the normalisation
 * ((v / 255) - mean[c]) / std[c] of PetSegmentationDataset.__getitem__ (Our_UNet/src/train.py:
 * 303-308) happens in the loaders of the first convolution and of its weight gradient, so the
 * fp32 image is never written (12x less input traffic).  mean3 / std3 are HOST pointers.
 * W % 128 == 0; other widths go through unet_preprocess_u8.  Workspaces / *stats_px_out as
 * unet_conv_in_fwd (stride 1) and unet_conv3x3_bwd_weight (Cx = 3). */
int unet_stem_u8_fwd(const uint8_t* image_hwc, const float* UNET_HOST mean3,
                     const float* UNET_HOST std3, const float* wf, const float* bias, float* y,
                     void* workspace, size_t workspace_bytes, int* UNET_HOST stats_px_out, int N,
                     int H, int W, int Cout, unet_stream_t stream);
int unet_stem_u8_bwd_weight(const uint8_t* image_hwc, const float* UNET_HOST mean3,
                            const float* UNET_HOST std3, const float* dy, float* dw_oihw,
                            void* workspace,
                            size_t workspace_bytes, int N, int H, int W, int Cout,
                            unet_stream_t stream);
/* The same on the mixed-precision pipeline: y / dy are bf16 tensors (statistics, workspace and
 * *stats_px_out as unet_conv_in_fwd_b16; dw stays fp32).  The fp32 accumulators are those of
 * the fp32 forms, so the results equal unet_conv_in_fwd_b16 / unet_conv_in_bwd_weight_b16 on the
 * image unet_preprocess_u8 writes, bit for bit. */
int unet_stem_u8_fwd_b16(const uint8_t* image_hwc, const float* UNET_HOST mean3,
                         const float* UNET_HOST std3, const float* wf, const float* bias,
                         uint16_t* y, void* workspace, size_t workspace_bytes,
                         int* UNET_HOST stats_px_out, int N, int H, int W, int Cout,
                         unet_stream_t stream);
int unet_stem_u8_bwd_weight_b16(const uint8_t* image_hwc, const float* UNET_HOST mean3,
                                const float* UNET_HOST std3, const uint16_t* dy, float* dw_oihw,
                                void* workspace,
                                size_t workspace_bytes, int N, int H, int W, int Cout,
                                unet_stream_t stream);

/* Weight gradient of the RGB stem with the stem layer's InstanceNorm + LeakyReLU + dropout
 * backward formed in its loader (fp32 tensors, W % 128 == 0).  g = dL/da of the stem layer, y its
 * raw output, `partial` the per-tile reductions (S1, S2) the producer of g left (`tiles` per
 * image, as unet_instnorm_lrelu_drop_bwd_partials takes them).  No gradient is taken with
 * respect to the image, so the layer's dL/dz has this one consumer and is never stored: the
 * summaries are merged, then the loader reads g and y and forms dz itself.  dw_oihw has the bits
 * of unet_instnorm_lrelu_drop_bwd_partials followed by unet_conv_in_bwd_weight /
 * unet_stem_u8_bwd_weight; dgamma / dbeta / dbias (each nullable) receive the layer's parameter
 * gradients.  x: the fp32 image [N][H][W][3], or NULL with the uint8 image and its mean3 / std3
 * (HOST pointers). */
size_t unet_stem_in_bwd_weight_fold_workspace_bytes(int N, int H, int W, int Cout);
int unet_stem_in_bwd_weight_fold(const float* x, const uint8_t* image_hwc,
                                 const float* UNET_HOST mean3, const float* UNET_HOST std3,
                                 const float* g, const float* y,
                                 const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, const float* mask, float slope,
                                 const void* partial, int tiles, float* dw_oihw, float* dgamma,
                                 float* dbeta, float* dbias, void* workspace,
                                 size_t workspace_bytes, int N, int H, int W, int Cout,
                                 unet_stream_t stream);

/* Weight gradient of a 32 -> 32 channel 3x3 layer (stride 1) with the layer's InstanceNorm +
 * LeakyReLU + dropout backward formed inside it (fp32 tensors), for the shapes
 * unet_conv_in_bwd_weight_fold32_supported accepts: those unet_conv_in_bwd_weight runs on the
 * 32-channel Winograd kernel under the calling thread's unet_set_c32_winograd switch.
 * g = dL/da of the layer (IN / OUT), y its raw output, `partial` the per-tile reductions (S1, S2)
 * the producer of g left (`tiles` per image).  The summaries are merged, then the weight
 * gradient's dy side reads g and y, forms dL/dz and stores it over g in place: on return g holds
 * dL/dz for the layer's data gradients, without the separate pass that would have written it.
 * x (activated on load with slope_x when x->alpha is set) is the layer's operand, or the half of
 * it whose columns ci_offset .. + 32 of dw_oihw[32][Cin_total][3][3] are written.  dw, dz and
 * dgamma / dbeta / dbias (each nullable) have the bits of unet_instnorm_lrelu_drop_bwd_partials
 * followed by unet_conv_in_bwd_weight. */
int unet_conv_in_bwd_weight_fold32_supported(int N, int H, int W, int Cx, int Cout);
size_t unet_conv_in_bwd_weight_fold32_workspace_bytes(int N, int H, int W);
int unet_conv_in_bwd_weight_fold32(const unet_act_src* x, float slope_x, float* g, const float* y,
                                   const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, const float* mask, float slope,
                                   const void* partial, int tiles, float* dw_oihw, int ci_offset,
                                   int Cin_total, float* dgamma, float* dbeta, float* dbias,
                                   void* workspace, size_t workspace_bytes, int N, int H, int W,
                                   unet_stream_t stream);

/* Weight gradient with the activation applied to the input operand on load:
 * dw_oihw[Cout][Cin_total][k][k] (columns ci_offset .. +x->C) = sum_pixels act(x) (x) dy.
 * Same workspace query as unet_conv3x3_bwd_weight.  ksize 1 keeps the centre tap. */
int unet_conv_in_bwd_weight(const unet_act_src* x, float slope, const float* dy, float* dw_oihw,
                            int ci_offset, int Cin_total, int ksize, int stride, void* workspace,
                            size_t workspace_bytes, int N, int H, int W, int Cout,
                            unet_stream_t stream);
/* The same in the split-bf16 operand mode (fp32 tensors; stride-1 3x3 layers on the bf16 matrix
 * cores with the activation applied before the three-term split, other shapes on the fp32
 * kernels).  Workspace as unet_conv3x3_bwd_weight_workspace_bytes. */
int unet_conv_in_bwd_weight_bf16x3(const unet_act_src* x, float slope, const float* dy, float* dw_oihw,
                            int ci_offset, int Cin_total, int ksize, int stride, void* workspace,
                            size_t workspace_bytes, int N, int H, int W, int Cout,
                            unet_stream_t stream);

/* up[N][2h][2w][C] = bilinear2x(act(x)) (the activation is applied to each of the four taps;
 * UpBlock.forward, Our_UNet/models/unet.py:219-225). */
int unet_upsample2x_in_fwd(const unet_act_src* x, float slope, float* up, int N, int h, int w,
                           unet_stream_t stream);

/* Backward of conv3x3(upsample2x(a)) at LOW resolution.  The bilinear up-sampling U is linear:
 *   dW[tap]  = sum_p (U a)[p + tap] (x) dy[p]   =  sum_q a[q] (x) D_tap[q]
 *   dL/da[q] = (U^T sum_tap W_tap^T shift_tap dy)[q]  =  sum_tap W_tap^T D_tap[q]
 * with D_tap = U^T shift_tap(dy): both gradients of the up-sampled operand of UpBlock's first
 * convolution (Our_UNet/models/unet.py:219-231) become GEMMs over the low-resolution pixels q --
 * a quarter of the positions, so a quarter of the FLOPs of the 3x3 weight / data gradient on
 * the up-sampled grid, no up-sampled tensor and no upsample2x_bwd pass.
 *   unet_upsample2x_bwd_taps:   D[N][h][w][9*C] (tap-major channels) from dy[N][2h][2w][C]
 *   unet_conv3x3_up_bwd_weight: dw_oihw[Cout][Cin_total][3][3] (columns ci_offset .. +x->C)
 *                               from act(x)[N][h][w][Cx] and D
 *   unet_conv3x3_up_bwd_data:   g[N][h][w][Ccols] (+)= sum_tap D_tap . wd[tap][ci_offset..][:]
 */
int unet_upsample2x_bwd_taps(const float* dy, float* D, int N, int h, int w, int C,
                             unet_stream_t stream);
/* General bilinear resize of NCHW planes, align_corners = False (x: [planes][h][w] ->
 * y: [planes][H][W]) and its adjoint (gather form, deterministic): the F.interpolate of
 * SimpleLoss for logits whose size differs from the target's (Our_UNet/models/losses.py:66-68)
 * and of CLIP_UNet's bottleneck features (CLIP_UNet/models/unet.py:444-450). */
int unet_resize_bilinear_fwd(const float* x, float* y, int planes, int h, int w, int H, int W,
                             unet_stream_t stream);
int unet_resize_bilinear_bwd(const float* gy, float* gx, int planes, int h, int w, int H, int W,
                             unet_stream_t stream);
size_t unet_conv3x3_up_bwd_weight_workspace_bytes(int N, int h, int w, int Cx, int Cout);
int unet_conv3x3_up_bwd_weight(const unet_act_src* x, float slope, const float* D, float* dw_oihw,
                               int ci_offset, int Cin_total, void* workspace,
                               size_t workspace_bytes, int N, int h, int w, int Cout,
                               unet_stream_t stream);
int unet_conv3x3_up_bwd_data(const float* D, const float* wd, int Cin_total, int ci_offset,
                             float* g, int N, int h, int w, int Cout, int Ccols, int accumulate,
                             unet_stream_t stream);

/* Data gradient whose output g = dL/da_l is FINAL for layer l (not a partial sum that another
 * call still accumulates into): the epilogue can also emit the two reductions of layer l's
 * InstanceNorm + LeakyReLU + dropout backward, S1 = sum gz and S2 = sum gz * xhat per tile,
 * which saves the pass that would re-read g and y_l (unet_instnorm_lrelu_drop_bwd's first half).
 * `bs` describes layer l; on return bs->tiles_out = summaries per image (0: this shape / kernel
 * has no such epilogue - run unet_instnorm_lrelu_drop_bwd as usual).  bs->partial needs
 * N * ceil(H*W / 64) * C * 8 bytes.  Consume with unet_instnorm_lrelu_drop_bwd_partials. */
typedef struct unet_bwd_stats {
  const float* y;      /* raw conv output of layer l, same shape as the gradient being written */
  const float* mean;   /* [N][C] */
  const float* rstd;   /* [N][C] */
  const float* gamma;  /* [C] */
  const float* beta;   /* [C] */
  const float* mask;   /* [N][C] dropout factors or NULL */
  float slope;
  void* partial;
  size_t partial_bytes;
  int tiles_out;
} unet_bwd_stats;
int unet_conv3x3_bwd_data_bs(const float* dy, const float* wd, int Cin_total, int ci_offset,
                             float* dx, int N, int H, int W, int Cout, int Ccols, int stride,
                             int accumulate, unet_bwd_stats* bs, unet_stream_t stream);
/* The same on the mixed-precision pipeline: dy, dx and bs->y are bf16 tensors (stride-1 shapes
 * of the patch kernel emit the reductions; bs->tiles_out = 0 otherwise). */
int unet_conv3x3_bwd_data_bs_b16(const uint16_t* dy, const float* wd, int Cin_total, int ci_offset,
                                 uint16_t* dx, int N, int H, int W, int Cout, int Ccols, int stride,
                                 int accumulate, unet_bwd_stats* bs, unet_stream_t stream);
/* unet_conv3x3_bwd_data_bs in the split-bf16 mode (wd3 = pre-split planes, data-gradient
 * layout); bs may be NULL (no reductions wanted). */
int unet_conv3x3_bwd_data_bs_bf16x3(const float* dy, const float* wd, const uint16_t* wd3,
                                    int Cin_total, int ci_offset, float* dx, int N, int H, int W,
                                    int Cout, int Ccols, int stride, int accumulate,
                                    unet_bwd_stats* bs, unet_stream_t stream);
int unet_conv3x3_up_bwd_data_bs(const float* D, const float* wd, int Cin_total, int ci_offset,
                                float* g, int N, int h, int w, int Cout, int Ccols, int accumulate,
                                unet_bwd_stats* bs, unet_stream_t stream);
/* ---- Winograd F(2x2, 3x3) form of the stride-1 3x3 layers (csrc/conv_wino.hip) ------------
 * 2.25x fewer matrix-core FLOPs than the direct kernels for the layers it tiles (image as
 * 8 x 32 pixels, >= 64 reduction channels in multiples of 8, output channels in multiples of
 * 64, >= 256 workgroups).  The transformed weights U = G g G^T (16 floats per filter, stored in
 * the kernel's LDS image order) are produced once per step by unet_pack_wino_weights:
 *   uf (forward,       Cout % 64 == 0, Cin % 8 == 0)  and/or
 *   ud (data gradient, Cin % 64 == 0, Cout % 8 == 0),  unet_wino_weight_floats() floats each.
 * Same arithmetic as nn.Conv2d / its data gradient (Our_UNet/models/unet.py:106-115) up to
 * fp32 rounding of the transforms (<= 3e-6 of max |y| measured). */
int unet_conv_wino_supported(int N, int H, int W, int C0, int C1, int Cout);
/* The 32 -> 32 channel stride-1 layers (enc0 / dec4 at full resolution) have a Winograd form of
 * their own inside unet_conv_in_fwd / unet_conv3x3_bwd_data(_bs): it needs no extra weight form
 * (U = G g G^T is built in the kernel's prologue from the packed weights), so it is a process-wide
 * switch rather than an entry point: 1 (default) = Winograd when the launch fills the chip (at
 * least 512 tiles of 8 x 32 pixels: the persistent kernel runs two workgroups per CU), 2 =
 * Winograd for every shape the kernel tiles, 0 = the direct kernel.  Returns the previous
 * setting.  The switch is kept PER CALLING THREAD (ABI 7; it was process-wide): a caller sets it
 * around its own launches and restores it, so two models on two threads - or a framework's
 * backward thread - cannot change each other's dispatch.  The weight gradient of the same layers (unet_conv_in_bwd_weight /
 * unet_conv3x3_bwd_weight with Cx = Cout = 32, stride 1, H % 8 == 0, W % 32 == 0) follows the
 * same switch: Winograd F(3x3,2x2) when there is an 8 x 32 tile for every CU (1) / always (2).
 * (csrc/conv_c32.hip, csrc/conv_wgrad.hip) */
int unet_set_c32_winograd(int on);
/* 1 when a 3x3 fused forward / data gradient of this shape runs that Winograd form (for FLOP
 * accounting: it issues 16/36 of the direct kernel's matrix-core FLOPs). */
int unet_conv_c32_is_winograd(int N, int H, int W, int Cin, int Cout, int stride);
/* The same switch covers unet_conv_up_in_fwd of the last decoder stage, (64 up-sampled + 32 skip)
 * -> 32 channels with both sources activated on load: K = 96 as three register-resident Winograd
 * chunks, the bilinear up-sampling folded into the input transform (1: with an 8 x 32 tile for
 * every CU, 2: every shape with H % 8 == 0 and W % 32 == 0).  1 when this shape takes it: */
int unet_conv_up_c32_is_winograd(int N, int H, int W, int C0, int C1, int Cout);
size_t unet_wino_weight_floats(int Cout, int Cin);
int unet_pack_wino_weights(const float* w_oihw, float* uf, float* ud, int Cout, int Cin,
                           unet_stream_t stream);
/* The same for several layers in one launch.  Entry k owns the blocks [block_begin,
 * block_begin + ceil(Cout * Cin / 8 / 256)); uf / ud may be null per entry (form not wanted);
 * the shape rules of unet_pack_wino_weights apply per entry (checked by the caller). */
typedef struct unet_wino_pack_entry {
  const float* w;   /* OIHW source [Cout][Cin][3][3] */
  float* uf;        /* forward form or null */
  float* ud;        /* data-gradient form or null */
  int Cout, Cin;
  int block_begin, reserved;
} unet_wino_pack_entry;
int unet_pack_wino_weights_batched(const unet_wino_pack_entry* UNET_DEVICE table_device, int n,
                                   int total_blocks, unet_stream_t stream);
/* unet_conv_in_fwd (ksize 3, stride 1) on the Winograd kernel: y = conv3x3(cat(act(s0),
 * act(s1))) + bias and the per-tile statistics of y (256 pixels per tile). */
int unet_conv_in_fwd_wino(const unet_act_src* s0, const unet_act_src* s1, float slope,
                          const float* uf, const float* bias, float* y, void* workspace,
                          size_t workspace_bytes, int* UNET_HOST stats_px_out, int N, int H, int W,
                          int Cout, unet_stream_t stream);
/* 1 when unet_conv3x3_bwd_weight / unet_conv_in_bwd_weight (ksize 3, fp32 tensors) run this
 * shape on the Winograd F(3x3,2x2) weight-gradient kernel (bench.py: executed FLOPs). */
int unet_conv3x3_bwd_weight_is_winograd(int N, int H, int W, int Cx, int Cout, int stride);
/* unet_conv_up_in_fwd on the Winograd kernel (the bilinear gather of the low-resolution source
 * runs inside its loader): low = [N][H/2][W/2][C0], skip = [N][H][W][C1]. */
int unet_conv_up_wino_supported(int N, int H, int W, int C0, int C1, int Cout);
int unet_conv_up_in_fwd_wino(const unet_act_src* low, const unet_act_src* skip, float slope,
                             const float* uf, const float* bias, float* y, void* workspace,
                             size_t workspace_bytes, int* UNET_HOST stats_px_out, int N, int H,
                             int W, int Cout, unet_stream_t stream);
/* unet_conv3x3_bwd_data_bs (stride 1, accumulate 0) on the Winograd kernel; ud covers the whole
 * weight [Cout][Cin_total], ci_offset % 64 == 0; bs may be NULL. */
int unet_conv3x3_bwd_data_bs_wino(const float* dy, const float* ud, int Cin_total, int ci_offset,
                                  float* dx, int N, int H, int W, int Cout, int Ccols,
                                  unet_bwd_stats* bs, unet_stream_t stream);

/* Merge of the per-tile reductions of the InstanceNorm + LeakyReLU + dropout backward:
 * partial[(n * tiles + t) * C + c] = (S1, S2) of tile t of image n (float pairs, as a data
 * gradient's unet_bwd_stats epilogue leaves them) ->
 * sums[n * C + c] = (S1, S2) and coef[n * C + c] = (S1, S2) / HW, float pairs.  The tiles are
 * summed in double in a fixed order (deterministic), one rounding at the end.  This is the first
 * step of unet_instnorm_lrelu_drop_bwd_partials and of the calls that form dz on the way to
 * another result (unet_head1x1_in_bwd_fold, unet_stem_in_bwd_weight_fold). */
int unet_instnorm_bwd_merge_partials(const void* partial, int tiles, void* coef, void* sums, int N,
                                     int HW, int C, unet_stream_t stream);

/* unet_instnorm_lrelu_drop_bwd with the reductions already summarised per tile
 * (partial[(n * tiles + t) * C + c] = (S1, S2)). */
int unet_instnorm_lrelu_drop_bwd_partials(const float* ga, const float* y, const float* mean,
                                          const float* rstd, const float* gamma,
                                          const float* beta, const float* mask, float slope,
                                          float* dy, float* dgamma, float* dbeta, float* dbias,
                                          const void* partial, int tiles, void* workspace,
                                          size_t workspace_bytes, int N, int HW, int C,
                                          unet_stream_t stream);
/* bf16 storage (mixed-precision pipeline): ga, y, dy are bf16 tensors. */
int unet_instnorm_lrelu_drop_bwd_partials_b16(const uint16_t* ga, const uint16_t* y,
                                              const float* mean, const float* rstd,
                                              const float* gamma, const float* beta,
                                              const float* mask, float slope, uint16_t* dy,
                                              float* dgamma, float* dbeta, float* dbias,
                                              const void* partial, int tiles, void* workspace,
                                              size_t workspace_bytes, int N, int HW, int C,
                                              unet_stream_t stream);

/* ---- mixed precision with bf16 activations in HBM (BASELINE config 4) ----------------------
 * The reference's AMP path is fp16 autocast + GradScaler (Our_UNet/src/train.py:638-652); the
 * MI355X form is bf16 (fp32's exponent range: no loss scaling).  The *_b16 entry points are the
 * fused-pipeline entry points above with every layer tensor -- raw convolution outputs y,
 * activation gradients, dy, D -- stored as bf16 (uint16_t* here; `x` of a unet_act_src then
 * points to bf16 data) while the RGB image, logits, InstanceNorm statistics / coefficients,
 * weights, weight gradients and the optimizer state stay fp32.  Convolutions contract bf16
 * operands on the bf16 matrix cores with fp32 accumulation (stride-1 weight gradients too;
 * stride-2 weight gradients and the low-resolution tap GEMM use the fp32 matrix cores on bf16
 * storage); the activation and all InstanceNorm arithmetic are fp32 on values widened on load;
 * statistics come from the fp32 accumulators before y is rounded. */
int unet_conv_in_fwd_b16(const unet_act_src* s0, const unet_act_src* s1, float slope,
                         const float* w, const float* bias, int ksize, int stride, uint16_t* y,
                         void* workspace, size_t workspace_bytes, int* UNET_HOST stats_px_out,
                         int N, int H, int W, int Cout, unet_stream_t stream);
/* unet_conv_in_fwd_b16 with the weights also given pre-rounded to bf16 (wb = [9][Cout][Cin],
 * plane 0 of unet_pack_conv3x3_weights_batched's wf3; may be null): the stride-1 patch kernel
 * stages its weight panels without the conversion, at half the L2 traffic; bit-identical. */
int unet_conv_in_fwd_b16_wb(const unet_act_src* s0, const unet_act_src* s1, float slope,
                            const float* w, const uint16_t* wb, const float* bias, int ksize,
                            int stride, uint16_t* y, void* workspace, size_t workspace_bytes,
                            int* UNET_HOST stats_px_out, int N, int H, int W, int Cout,
                            unet_stream_t stream);
/* unet_conv3x3_bwd_data_bs_b16 likewise (wdb = [9][Cin_total][Cout] bf16, plane 0 of wd3). */
int unet_conv3x3_bwd_data_bs_b16_wb(const uint16_t* dy, const float* wd, const uint16_t* wdb,
                                    int Cin_total, int ci_offset, uint16_t* dx, int N, int H,
                                    int W, int Cout, int Ccols, int stride, int accumulate,
                                    unet_bwd_stats* bs, unet_stream_t stream);
int unet_conv_in_stats_finalize_b16(const uint16_t* y, void* workspace, size_t workspace_bytes,
                                    int stats_px, const float* gamma, const float* beta, float eps,
                                    const float* mask, float* mean, float* rstd, float* alpha_out,
                                    float* beta_out, int N, int HoWo, int Cout,
                                    unet_stream_t stream);
int unet_conv_in_bwd_weight_b16(const unet_act_src* x, float slope, const uint16_t* dy,
                                float* dw_oihw, int ci_offset, int Cin_total, int ksize, int stride,
                                void* workspace, size_t workspace_bytes, int N, int H, int W,
                                int Cout, unet_stream_t stream);
int unet_conv3x3_bwd_data_b16(const uint16_t* dy, const float* wd, int Cin_total, int ci_offset,
                              uint16_t* dx, int N, int H, int W, int Cout, int Ccols, int stride,
                              int accumulate, unet_stream_t stream);
int unet_instnorm_lrelu_drop_bwd_b16(const uint16_t* ga, const uint16_t* y, const float* mean,
                                     const float* rstd, const float* gamma, const float* beta,
                                     const float* mask, float slope, uint16_t* dy, float* dgamma,
                                     float* dbeta, float* dbias, void* workspace,
                                     size_t workspace_bytes, int N, int HW, int C,
                                     unet_stream_t stream);
int unet_upsample2x_in_fwd_b16(const unet_act_src* x, float slope, uint16_t* up, int N, int h,
                               int w, unet_stream_t stream);
/* unet_conv_up_in_fwd on bf16 tensors: the first convolution of a decoder stage with the bilinear
 * 2x up-sampling of the (activated) low-resolution source done in the loader - no up-sampled
 * tensor (round 4; bit-identical to unet_upsample2x_in_fwd_b16 + unet_conv_in_fwd_b16_wb).
 * low [N][H/2][W/2][C0], skip [N][H][W][C1] (both activated on load), y [N][H][W][Cout] bf16;
 * w3 = the bf16-rounded plane of the packed weights (required).  Replaces UpBlock.forward
 * (Our_UNet/models/unet.py:215-231) under autocast. */
int unet_conv_up_in_fwd_b16_supported(int N, int H, int W, int C0, int C1, int Cout);
int unet_conv_up_in_fwd_b16(const unet_act_src* low, const unet_act_src* skip, float slope,
                            const float* wf, const uint16_t* w3, const float* bias, uint16_t* y,
                            void* workspace, size_t workspace_bytes, int* UNET_HOST stats_px_out,
                            int N, int H, int W, int Cout, unet_stream_t stream);
int unet_upsample2x_bwd_taps_b16(const uint16_t* dy, uint16_t* D, int N, int h, int w, int C,
                                 unet_stream_t stream);
int unet_conv3x3_up_bwd_weight_b16(const unet_act_src* x, float slope, const uint16_t* D,
                                   float* dw_oihw, int ci_offset, int Cin_total, void* workspace,
                                   size_t workspace_bytes, int N, int h, int w, int Cout,
                                   unet_stream_t stream);
int unet_conv3x3_up_bwd_data_b16(const uint16_t* D, const float* wd, int Cin_total, int ci_offset,
                                 uint16_t* g, int N, int h, int w, int Cout, int Ccols,
                                 int accumulate, unet_stream_t stream);
/* ... with the BSTATS epilogue (g final for the layer bs describes; bs->y bf16), as
 * unet_conv3x3_up_bwd_data_bs: removes that layer's stand-alone reduction pass. */
int unet_conv3x3_up_bwd_data_bs_b16(const uint16_t* D, const float* wd, int Cin_total,
                                    int ci_offset, uint16_t* g, int N, int h, int w, int Cout,
                                    int Ccols, int accumulate, unet_bwd_stats* bs,
                                    unet_stream_t stream);
/* ... with the weights also pre-rounded to bf16 (wdb = [9][Cin_total][Cout] bf16, plane 0 of
 * wd3; NULL = as above; the backward of UpBlock's first convolution with respect to its
 * up-sampled operand, Our_UNet/models/unet.py:219-231, under autocast,
 * Our_UNet/src/train.py:638-652): the contraction runs as a plain bf16 GEMM over the 9 * Cout contiguous
 * values of a D row (64-wide K steps, no conversion of the weights).  Same result as the form
 * above up to the summation order of the fp32 accumulators; bs may be NULL. */
int unet_conv3x3_up_bwd_data_bs_b16_wb(const uint16_t* D, const float* wd, const uint16_t* wdb,
                                       int Cin_total, int ci_offset, uint16_t* g, int N, int h,
                                       int w, int Cout, int Ccols, int accumulate,
                                       unet_bwd_stats* bs, unet_stream_t stream);
int unet_head1x1_in_fwd_b16(const unet_act_src* x, float slope, const float* w, const float* b,
                            float* logits_nchw, int N, int HW, int K, unet_stream_t stream);
int unet_head1x1_in_bwd_b16(const unet_act_src* x, float slope, const float* dlogits_nchw,
                            const float* w, uint16_t* da, float* dw, float* db, void* workspace,
                            size_t workspace_bytes, int N, int HW, int K, unet_stream_t stream);

/* Head on an activated-on-load operand: logits = act(x) . w + b, and its backward
 * (da = dL/d act(x), dw, db); x->C == 32. */
int unet_head1x1_in_fwd(const unet_act_src* x, float slope, const float* w, const float* b,
                        float* logits_nchw, int N, int HW, int K, unet_stream_t stream);
int unet_head1x1_in_bwd(const unet_act_src* x, float slope, const float* dlogits_nchw,
                        const float* w, float* da, float* dw, float* db, void* workspace,
                        size_t workspace_bytes, int N, int HW, int K, unet_stream_t stream);
/* ... with the reductions of the InstanceNorm + LeakyReLU + dropout backward of the layer whose
 * raw output x->x is (bs->y == x->x; Our_UNet/models/unet.py:128-134 in front of :427): da is
 * that layer's final dL/da, so the kernel that writes it also leaves S1 = sum gz and
 * S2 = sum gz * xhat per workgroup in bs->partial (bs->tiles_out summaries per image; 0 = the
 * shape does not split evenly - run unet_instnorm_lrelu_drop_bwd as usual).  _b16: x, da and
 * bs->y are bf16 tensors. */
int unet_head1x1_in_bwd_bs(const unet_act_src* x, float slope, const float* dlogits_nchw,
                           const float* w, float* da, float* dw, float* db, void* workspace,
                           size_t workspace_bytes, int N, int HW, int K, unet_bwd_stats* bs,
                           unet_stream_t stream);
int unet_head1x1_in_bwd_bs_b16(const unet_act_src* x, float slope, const float* dlogits_nchw,
                               const float* w, uint16_t* da, float* dw, float* db,
                               void* workspace, size_t workspace_bytes, int N, int HW, int K,
                               unet_bwd_stats* bs, unet_stream_t stream);

/* ... and with that layer's whole InstanceNorm + LeakyReLU + dropout backward (fp32 tensors):
 * where unet_head1x1_in_bwd_bs would leave the reductions (bs->tiles_out > 0 on return), da is
 * never stored.  A first launch leaves the reductions and dw / db, the summaries are merged, and
 * a second launch of the head's kernel forms da again per lane and writes the layer's dL/dz to
 * `dz` - the bits of unet_head1x1_in_bwd_bs followed by unet_instnorm_lrelu_drop_bwd_partials,
 * without the two passes over da; dgamma / dbeta / dbias (each nullable) receive the layer's
 * parameter gradients.  bs->tiles_out == 0: the call was unet_head1x1_in_bwd_bs, `dz` holds da
 * and unet_instnorm_lrelu_drop_bwd is the caller's next step.  The workspace holds the dw / db
 * slabs and the merged sums. */
size_t unet_head1x1_in_bwd_fold_workspace_bytes(int N, int HW, int K);
int unet_head1x1_in_bwd_fold(const unet_act_src* x, float slope, const float* dlogits_nchw,
                             const float* w, float* dz, float* dw, float* db, float* dgamma,
                             float* dbeta, float* dbias, void* workspace, size_t workspace_bytes,
                             int N, int HW, int K, unet_bwd_stats* bs, unet_stream_t stream);

/* ---- autoencoder pretraining step (recon.hip) ------------------------------------------------
 * The reference's phase 1 of transfer learning (AE_pretrained/README.md) on the same body as the
 * segmentation net.  x_bf16 selects the storage type of the layer tensors (x->x and da): 0 = fp32,
 * 1 = bf16 (matmul_precision="bf16"); the arithmetic is fp32 in both cases. */

/* reconstruction_output = Sequential(Conv2d(32, 3, 3, padding=1), Sigmoid())
 * (AE_pretrained/reconstruction/models/autoencoder.py:377-387, applied at :444): out (NCHW fp32
 * [N,K,H,W]) = sigmoid(conv3x3(act(x)) + b); x is activated on load as in unet_head1x1_in_fwd
 * (x->alpha == NULL: a plain activation), the zero padding applied after the activation.
 * w is OIHW [K][32][3][3]; x->C == 32, K == 3. */
int unet_recon3x3_fwd(const unet_act_src* x, int x_bf16, float slope, const float* w,
                      const float* b, float* out_nchw, int N, int H, int W, int K,
                      unet_stream_t stream);
size_t unet_recon3x3_bwd_workspace_bytes(int N, int H, int W);
/* autograd of the same (the Sigmoid and Conv2d backward of loss.backward(), src/train.py:434):
 * dz = dout * out * (1 - out) formed on load; da = dL/d act(x) (NHWC, the layer tensors' type:
 * the 3 -> 32 transposed 3x3 conv of dz), dw [K][32][3][3] and db [K] through per-workgroup
 * partials and a fixed-order double finalize.  bs (nullable): as unet_head1x1_in_bwd_bs, also
 * leave the InstanceNorm-backward reductions of the layer whose raw output x->x is
 * (bs->tiles_out summaries per image; 0 = not emitted, run unet_instnorm_lrelu_drop_bwd). */
int unet_recon3x3_bwd(const unet_act_src* x, int x_bf16, float slope, const float* dout_nchw,
                      const float* out_nchw, const float* w, void* da, float* dw, float* db,
                      void* workspace, size_t workspace_bytes, int N, int H, int W, int K,
                      unet_bwd_stats* bs, unet_stream_t stream);

/* nn.MSELoss() (reduction "mean") of the output against the input image
 * (AE_pretrained/reconstruction/src/train.py:420-437, called at :531 and :467).  target is the
 * NCHW fp32 tensor (target_u8 == 0) or the dataset's uint8 NHWC image [N,H,W,3] (target_u8 == 1,
 * t = v / 255 correctly rounded to fp32: the CPU division of image.float() / 255.0 at :257-266).
 * loss_out[0] = sum (out - t)^2 / (N*C*H*W); per_image[N] (double) = the per-image sums of
 * squares (validation's per-image MSE and PSNR, :470-477). */
size_t unet_mse_loss_workspace_bytes(int N, int C, int H, int W);
int unet_mse_loss_fwd(const float* out_nchw, const void* target, int target_u8, float* loss_out,
                      double* per_image, void* workspace, size_t workspace_bytes, int N, int C,
                      int H, int W, unet_stream_t stream);
/* dout = upstream[0] * 2 (out - t) / (N*C*H*W); upstream: a device float or NULL (= 1) */
int unet_mse_loss_grad(const float* out_nchw, const void* target, int target_u8,
                       const float* upstream, float* dout_nchw, int N, int C, int H, int W,
                       unet_stream_t stream);

/* optim.Adam(params, lr, weight_decay) (AE_pretrained/reconstruction/src/train.py:377-397;
 * amsgrad = maximize = False, coupled L2) over n floats: g = grad * grad_scale + wd * p, then
 * torch's exp_avg / exp_avg_sq / bias-corrected update.  hyper (fp64, device):
 * {lr, beta1, beta2, eps, weight_decay, grad_scale, step, -}, so a graph-captured step follows the
 * LR schedule and the bias correction; advance_step != 0 first adds 1 to hyper[6] on the device. */
int unet_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t n, double* hyper, int advance_step, unet_stream_t stream);

/* ---- SSIM (ssim.hip) ---------------------------------------------------------------------------
 * The 11-tap Gaussian-window SSIM of the reference's reconstruction metrics and SSIM loss over
 * pred (NCHW fp32 [N,C,H,W]) and target: the NCHW fp32 tensor (target_u8 == 0) or the dataset's
 * uint8 NHWC image [N,H,W,3] (target_u8 == 1, t = v / 255 rounded once to fp32, as
 * unet_mse_loss_fwd).  gauss11: 11 host floats, the 1-D window (the 2-D window is its outer
 * product); c1, c2: the stabilisers ((0.01 max_val)^2, (0.03 max_val)^2).  The window moments are
 * taken with zero padding outside the image (conv2d(padding=5)).  Any H, W >= 1. */

/* calculate_ssim / calculate_psnr / evaluate_reconstructions
 * (AE_pretrained/reconstruction/utils/metrics.py:15-147; src/evaluate.py:268-377) and the forward
 * of SSIMLoss / ReconstructionLoss (models/losses.py:12-79, :178-245).  One read of both images:
 * ssim_per_image[N] (double) = the mean of the SSIM map over C, H, W; sq_per_image[N] (double) =
 * the sum of (pred - t)^2 (MSE and PSNR).  loss_out (nullable, fp32 [1]) =
 * w_ssim * (1 - mean SSIM) + w_mse * sum sq / (N*C*H*W).  Per-workgroup partials and a
 * fixed-order finalize whose order depends on (C, H, W) only: an image's values are bit-identical
 * in any batch. */
size_t unet_ssim_workspace_bytes(int N, int C, int H, int W);
int unet_ssim_fwd(const float* pred_nchw, const void* target, int target_u8,
                  const float* UNET_HOST gauss11, float c1, float c2, double* ssim_per_image, double* sq_per_image,
                  float* loss_out, double w_ssim, double w_mse, void* workspace,
                  size_t workspace_bytes, int N, int C, int H, int W, unet_stream_t stream);
/* autograd of L = up * [w_ssim * (1 - mean SSIM) + w_mse * mean (pred - t)^2] (SSIMLoss /
 * ReconstructionLoss backward, models/losses.py:54-79, :226-245) in one launch: dpred (NCHW fp32).
 * upstream_per_image == 0: the means run over all N*C*H*W elements and up = upstream[0]
 * (size_average=True); 1: over each image's C*H*W and up = upstream[n] (size_average=False).
 * upstream: a device float array or NULL (= 1; not with upstream_per_image).  No saved maps: the
 * moments are recomputed on a 10-pixel halo. */
int unet_ssim_grad(const float* pred_nchw, const void* target, int target_u8,
                   const float* UNET_HOST gauss11, float c1, float c2, const float* upstream,
                   int upstream_per_image, double w_ssim, double w_mse, float* dpred_nchw, int N,
                   int C, int H, int W, unet_stream_t stream);

/* ---- Perceptual (VGG16 feature) loss (perceptual.hip) -------------------------------------------
 * PerceptualLoss (AE_pretrained/reconstruction/models/losses.py:82-168): the mean over the tapped
 * layers of F.mse_loss between the features of a frozen, randomly initialised VGG16
 * (models.vgg16(weights=None), :100) on the normalised output and target.  A trunk layer is
 * relu(conv3x3(x) + b): the convolutions run on the fused pipeline's entry points with the RAW
 * output y_l stored once and relu applied on load (unet_act_src with alpha = 1, beta = 0 and
 * slope = 0), on the STACKED tensor of 2N images - images 0..N-1 the output, N..2N-1 the target -
 * so one launch serves both streams; the reference's four prefix passes (:156-163) become one pass
 * with taps.  The entry points below are everything around the convolutions.  fp32 NHWC layer
 * tensors, C % 32 == 0, 64-bit indexing; reductions through per-workgroup partials in double and
 * a fixed-order finalize (bit-identical from run to run); no host synchronisation. */

/* PerceptualLoss._normalize (:134-136) into the stacked tensor: xn [2N][H][W][3] (plain NHWC) =
 * (x - mean[c]) / std[c], subtraction and division each correctly rounded (the reference's two
 * operations).  Images 0..N-1 from out_nchw [N,3,H,W]; N..2N-1 from target: the NCHW fp32 tensor
 * (target_u8 == 0) or the dataset's uint8 NHWC image (target_u8 == 1, v / 255 rounded once to
 * fp32 as unet_mse_loss_fwd).  mean3 / std3: 3 host floats each. */
int unet_perceptual_prep(const float* out_nchw, const void* target, int target_u8,
                         const float* UNET_HOST mean3, const float* UNET_HOST std3, float* xn,
                         int N, int H, int W, unet_stream_t stream);
/* nn.ReLU + nn.MaxPool2d(2, 2) of the trunk (torchvision configuration "D"): raw y [M][H][W][C]
 * -> plain p [M][H/2][W/2][C] = max(0, max of the 2x2 window); floor semantics, an odd last row
 * or column is ignored.  H, W >= 2. */
int unet_relu_maxpool2x2_fwd(const float* y, float* p, int M, int H, int W, int C,
                             unet_stream_t stream);
/* The sums of F.mse_loss(output_features, target_features) (:162) of one tapped layer: over raw
 * y [2N][H][W][C], sums[n] (double, n < N) = sum over the image of (relu(y[n]) - relu(y[n+N]))^2,
 * every term two fp32 roundings, the sum in double.  The order of the sum depends on (H, W, C)
 * only: an image pair's value is bit-identical in any batch.  The caller forms
 * loss = (1/L) sum_l sum_n sums[l][n] / (N C_l H_l W_l)  (:162-166). */
size_t unet_feature_mse_workspace_bytes(int N, int H, int W, int C);
int unet_feature_mse_fwd(const float* y, double* sums, void* workspace, size_t workspace_bytes,
                         int N, int H, int W, int C, unet_stream_t stream);
/* autograd of one trunk layer between two convolutions, for the output half y_o [N][H][W][C]:
 *   dz = y_o > 0 ? g_in + coef * (relu(y_o) - relu(y_t)) : 0
 * the ReLU backward, the layer's own feature-MSE gradient (y_t = the target half, NULL at a layer
 * that is not tapped; coef = 2 / (L N_batch C H W)) and g_in, at most one of
 *   g  [N][H][W][C]:      the data gradient of the next convolution, or
 *   gp [N][H/2][W/2][C]:  the gradient of the following 2x2 max-pool's output, routed to the
 *                         window's first maximum in row-major order (PyTorch's rule); positions
 *                         of an ignored odd row or column receive 0 from it.
 * Both NULL: the deepest tapped layer (y_t required). */
int unet_perceptual_relu_bwd(const float* y_o, const float* y_t, float coef, const float* g,
                             const float* gp, float* dz, int N, int H, int W, int C,
                             unet_stream_t stream);
/* Data gradient of conv1_1 with the normalisation's 1/std folded in: dout_nchw [N,3,H,W] =
 * conv3x3_transpose(dz [N][H][W][Cout], w_oihw [Cout][3][3][3])[c] / std3[c] (3 host floats), the
 * gradient with respect to the loss's `output` argument (:150).  Cout % 32 == 0, any H, W. */
int unet_perceptual_stem_bwd_data(const float* dz, const float* w_oihw, const float* UNET_HOST std3,
                                  float* dout_nchw, int N, int H, int W, int Cout,
                                  unet_stream_t stream);

/* ---- Grad-CAM (Our_UNet/utils/visualize.py:372-439) ---------------------------------------- *
 * The tail of generate_gradcam_heatmap after the backward pass, for a whole batch: A = the output
 * of the target stage, G = dL/dA, both NHWC [N][HW][C] in the layer tensors' storage type
 * (*_bf16: 0 = fp32, 1 = bf16; the arithmetic is fp32).  C = 4..256 a power of two, 512 or 1024;
 * HW <= 2^30.  Fixed-order sums, no floating-point atomics (two runs are bit-identical), nothing
 * is read back to the host.  One workspace of unet_gradcam_workspace_bytes(N, HW, C) serves the
 * three calls, in this order on one stream. */
size_t unet_gradcam_workspace_bytes(int N, int HW, int C);
/* w[N][C] = mean over the pixels of g (visualize.py:424), correctly divided by HW. */
int unet_gradcam_weights(const void* g, int g_bf16, float* w, void* workspace,
                         size_t workspace_bytes, int N, int HW, int C, unet_stream_t stream);
/* cam[N][HW] = max(0, sum_c w[n][c] * act(a)[n][p][c]) (:427-428); a is activated while it is
 * loaded, as every consumer of a fused layer does (a->alpha == NULL: a plain tensor; eval mode,
 * so the coefficients carry no dropout mask).  Leaves per-workgroup (min, max) of cam in the
 * workspace for unet_gradcam_heatmap. */
int unet_gradcam_map(const unet_act_src* a, int a_bf16, float slope, const float* w, float* cam,
                     void* workspace, size_t workspace_bytes, int N, int HW, unet_stream_t stream);
/* heatmap[N][H][W] = bilinear resize (align_corners = False, the rule of
 * unet_resize_bilinear_fwd) of the per-image normalisation of cam[N][h][w] (:431-437):
 * (cam - min) / max(cam - min), each tap normalised as it is read; an image whose
 * max(cam - min) is 0 stays all zero (the reference's `if cam.max() != 0`, decided on the
 * device, no division).  workspace: as left by unet_gradcam_map with the same N and HW = h * w. */
int unet_gradcam_heatmap(const float* cam, const void* workspace, size_t workspace_bytes,
                         float* heatmap, int N, int h, int w, int H, int W, unet_stream_t stream);

/* ---- CLIP ViT image tower (vit.hip) -------------------------------------------------------------
 * ClipPatchExtractor.forward (CLIP_UNet/models/unet.py:581-613): resize to the tower's resolution,
 * clip_model.encode_image (OpenAI CLIP's VisionTransformer, frozen), broadcast of the embedding to
 * a 16 x 16 map.  Forward only.  The residual stream [N T, D], LayerNorm statistics, softmax and
 * every epilogue are fp32; GEMM and attention operands are bf16 (rounded to nearest even) with
 * fp32 accumulators.  No atomics: two runs are bit-identical.  Limits: T <= 257 tokens, D a
 * multiple of 64 and <= 1024, head dimension 64 (ViT-B/32, B/16, L/14 at 224); anything else is
 * UNET_E_INVALID before a launch. */

/* The patch matrix of conv1 (kernel = stride = P, no bias) as a GEMM operand: patches bf16
 * [N G^2][Kp], G = R / P, row (n, gy, gx), column k = (c P + py) P + px (the order of
 * conv1.weight.reshape(D, -1)); columns 3 P^2 .. Kp-1 are zero (Kp % 16 == 0).  image: fp32 NCHW
 * [N,3,H,W] taken as it is (image_u8 == 0; mean3 / std3 unused) or the dataset's uint8 NHWC
 * [N,H,W,3] with (v / 255 - mean3[c]) / std3[c] folded in (3 host floats each).  H x W != R x R:
 * F.interpolate(mode="bilinear", align_corners=False) of the normalised image (:595), sampled while
 * gathering. */
int unet_vit_patchify(const void* image, int image_u8, const float* UNET_HOST mean3,
                      const float* UNET_HOST std3, void* patches, int N, int H, int W, int R, int P, int Kp,
                      unet_stream_t stream);
/* out [M][Nout] = a [M][K] w[Nout][K]^T, a and w bf16 with K contiguous, any M, Nout % 64 == 0,
 * K % 16 == 0; rows >= M of `out` are not touched.  epilogue:
 *   0  out fp32 = product (bias unused)                  the patch embedding
 *   1  out bf16 = product + bias[Nout]                   in_proj (QKV)
 *   2  out bf16 = QuickGELU(product + bias), x sigmoid(1.702 x)   mlp.c_fc
 *   3  out fp32 += product + bias, in place              out_proj / mlp.c_proj into the stream */
int unet_vit_gemm_bf16(const void* a, const void* w, const float* bias, void* out, int epilogue,
                       int M, int Nout, int K, unet_stream_t stream);
/* Token assembly and ln_pre: out fp32 [N T][D] = LayerNorm over D of
 * (t == 0 ? cls[D] : patches[n (T-1) + t-1][D]) + pos[t][D]. */
int unet_vit_tokens_ln(const float* patches, const float* cls, const float* pos,
                       const float* gamma, const float* beta, float eps, float* out, int N, int T,
                       int D, unet_stream_t stream);
/* out bf16 [rows][D] = LayerNorm(x fp32 [rows][D]) * gamma + beta, biased variance of the centred
 * row, one pass over memory. */
int unet_vit_layernorm(const float* x, const float* gamma, const float* beta, float eps, void* out,
                       int rows, int D, unet_stream_t stream);
/* Multi-head self-attention of nn.MultiheadAttention's packed projection, all (image, head) pairs
 * in one launch: qkv bf16 [N T][3 D] (q, k, v thirds; head h = columns 64h .. 64h+63 of each),
 * out bf16 [N T][D] = softmax(q k^T / 8) v.  Scores and the row sum are fp32, the probabilities
 * are rounded to bf16 for the second product. */
int unet_vit_attention(const void* qkv, void* out, int N, int T, int D, int heads,
                       unet_stream_t stream);
/* ln_post of each image's class row of x [N T][D], @ proj [D][E] (fp32), broadcast to
 * out fp32 NCHW [N][E][grid][grid] (:611-612: bilinear interpolation from 1 x 1 is a copy). */
int unet_vit_head(const float* x, const float* gamma, const float* beta, float eps,
                  const float* proj, float* out, int N, int T, int D, int E, int grid,
                  unet_stream_t stream);

/* ---- from decoded samples to a network-size batch (letterbox.hip) ---------------------
 * What the reference does with OpenCV on the host before a sample reaches the network: the
 * aspect-preserving resize into a centred square (data_augmentation/src/preprocess_dataset.py:
 * 307-355, preprocess_training_labels.py:109-167, CLIP_UNet/scripts/create_clip_resized_images.py:
 * 104-152), the dataset's plain stretch (src/train.py __getitem__), the re-encoding of the trimap
 * bytes (preprocess_test_val_labels.py:201-331) and the class-pixel scan of src/train.py main.
 *
 * A ragged batch is ONE device byte arena holding B samples of different sizes (images HWC uint8,
 * masks HW uint8, at any byte offset) and a device table of one record per sample, never read on the
 * host: table[b][UNET_LETTERBOX_FIELDS] (int64)
 *     0 image byte offset    1 mask byte offset (< 0: the sample has no mask)
 *     2 h    3 w             source size
 *     4 out_h    5 out_w     size the sample is resized to
 *     6 pad_y    7 pad_x     where the resized sample sits in its S_h x S_w tile
 * arena_bytes bounds every read: a record whose image (mask) does not lie inside the arena is
 * treated as a record with bad sizes. */
#define UNET_LETTERBOX_FIELDS 8

/* image_out[B][S_h][S_w][3] and (mask_out != NULL) mask_out[B][S_h][S_w], uint8: every sample
 * resized to out_h x out_w - the image with OpenCV's INTER_LINEAR, the mask with INTER_NEAREST -
 * and written at (pad_y, pad_x) of its tile; every other byte of the tile is 0 (no memset: the
 * kernel writes whole rows).  One launch, grid (row bands, B).  A stretch is out = S, pad = 0.
 * lut (nullable) [B][256] uint8 is applied to the mask bytes read (not to the padding).
 * Per axis (src -> dst), all in the precision named:
 *   scale = 1.0 / ((double)dst / (double)src)
 *   linear   f = (float)((d + 0.5) * scale - 0.5) (double, two roundings), s = floor(f), f -= s;
 *            s < 0: s = 0, f = 0;  s >= src - 1: s = src - 1, f = 0;
 *            taps s and min(s + 1, src - 1), weights (rint((1.f - f) * 2048.f), rint(f * 2048.f));
 *            R = S[s] a0 + S[s1] a1 along x for the two rows, then
 *            out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2
 *   area     h == 2 out_h and w == 2 out_w: out = (a + b + c + d + 2) >> 2 over the 2 x 2 block
 *            instead (OpenCV's INTER_LINEAR takes its fast area path there)
 *   nearest  s = min((int)floor(d * scale), src - 1), the product in double.
 * A record with h or w outside 1..16384, out outside 1..S, a negative pad or pad + out > S gives
 * that sample an all-zero tile (image and mask); a sample without a mask gets a zero mask tile.
 * UNET_E_INVALID before the launch: null arena / table / image_out, a lut without mask_out,
 * B outside 1..65535, S_h or S_w outside 1..4096. */
int unet_letterbox_u8(const uint8_t* arena, size_t arena_bytes, const int64_t* table, int B,
                      int S_h, int S_w, uint8_t* image_out, uint8_t* mask_out, const uint8_t* lut,
                      unet_stream_t stream);

/* hist[B][256] (uint64, device; zeroed here) = how often every byte value occurs in each sample's
 * mask at its original size: the set of values present (what the label table of the trimap
 * re-encoding needs) and the class pixel counts (the static class weights).  Fields 4..7 of the
 * records are not read; a contiguous [B][H][W] batch is the table with equal sizes.  A record
 * with h or w outside 1..16384, no mask, or a mask outside the arena gives zero counts.  Integer
 * adds only: the result does not depend on the order of the workgroups.
 * UNET_E_INVALID before the launch: null arena / table / hist, B outside 1..65535. */
int unet_byte_histogram_u8(const uint8_t* arena, size_t arena_bytes, const int64_t* table, int B,
                           uint64_t* hist, unet_stream_t stream);

/* ---- latent-space analysis (latent.hip) ----------------------------------------------
 * analyze_latent_space of AE_pretrained/reconstruction/src/evaluate.py:380-440 from the code matrix
 * x [N][D] (fp32, row-major, 16-byte aligned; N in 2..65536, D a multiple of 4).  Every sum has a
 * fixed order: two runs are bit-identical. */

/* Bytes of the workspace of unet_latent_col_mean / unet_latent_project.  0 for a bad shape. */
size_t unet_latent_colsum_workspace_bytes(int N, int D);
/* mean[d] = (sum_i x[i][d]) / N */
int unet_latent_col_mean(const float* x, float* mean, void* workspace, size_t workspace_bytes,
                         int N, int D, unet_stream_t stream);
/* out[c][d] = sum_i (x[i][d] - mean[d]) w[i][c], c = 0, 1; w [N][2]: the principal axes from the
 * dual eigenvectors (w = U / sqrt(lambda)). */
int unet_latent_project(const float* x, const float* mean, const float* w, float* out,
                        void* workspace, size_t workspace_bytes, int N, int D,
                        unet_stream_t stream);

/* g [N][N] = (x - mean)(x - mean)^T on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, fp32 sums):
 * the mean is subtracted while x is loaded; only the 128 x 128 tiles on or above the diagonal are
 * formed, in unet_latent_gram_splitk(N, D) slabs of D that a second launch sums in ascending order
 * and mirrors, so g is bitwise symmetric.  x may exceed 2 GiB (64-bit row offsets). */
size_t unet_latent_gram_workspace_bytes(int N, int D);
int unet_latent_gram_splitk(int N, int D);
int unet_latent_gram(const float* x, const float* mean, float* g, void* workspace,
                     size_t workspace_bytes, int N, int D, unet_stream_t stream);
/* z [N][8] = g q for q [N][8]: the product of the block subspace iteration */
int unet_latent_gram_apply(const float* g, const float* q, float* z, int N, unet_stream_t stream);

/* Exact t-SNE (scikit-learn's method='exact' restated), N in 2..8192.
 * cond_p: pc [N][N] = the conditional probabilities of sklearn's _binary_search_perplexity (100
 *   steps, tolerance 1e-5 on the entropy) over the squared distances max(g_ii + g_jj - 2 g_ij, 0),
 *   diag [N] = the diagonal of g; the row's minimum off-diagonal distance is subtracted before
 *   exp; pc_ii = 0.  rowsum [N + 1] (double): the row sums of pc; entry N is scratch of joint_p.
 * joint_p: p = max((pc + pc^T) / max(sum, eps), eps) off the diagonal, 0 on it (eps = DBL_EPSILON,
 *   as _joint_probabilities). */
int unet_tsne_cond_p(const float* g, const float* diag, float perplexity, float* pc,
                     double* rowsum, int N, unet_stream_t stream);
int unet_tsne_joint_p(const float* pc, double* rowsum, float* p, int N, unet_stream_t stream);
/* One iteration of sklearn's _gradient_descent on _kl_divergence, two launches.
 *   state [N][6] = (y0, y1, update0, update1, gains0, gains1), read from state_in, written to
 *   state_out (which must differ); rows [N][8] scratch.  With q_ij = 1 / (1 + |y_i - y_j|^2),
 *   Z = sum_{i != j} q_ij: grad_i = 4 (sum_j e p_ij q_ij (y_i - y_j) - sum_j q_ij^2 (y_i - y_j) / Z),
 *   e = exaggeration; gains + 0.2 where update grad < 0, else gains 0.8, floored at 0.01;
 *   update = momentum update - lr gains grad; y += update.
 *   want_stats != 0: stats[0] = KL = sum_{i != j} e p log(e p Z / q), stats[1] = |gains grad|
 *   (the norm _gradient_descent tests), both at state_in. */
int unet_tsne_step(const float* p, const float* state_in, float* state_out, float* rows,
                   double* stats, float exaggeration, float momentum, float lr, int want_stats,
                   int N, unet_stream_t stream);

/* out [H][W][3] (uint8) = the scatter picture on a white ground: centres [N][2] (int32 pixel
 * x, y), labels [N] (uint8), palette [K][3] (uint8 RGB).  Point n covers the pixels with
 * dx^2 + dy^2 <= radius^2; the covering points blend in index order,
 * dst = (dst 77 + src 179 + 128) >> 8 per channel (alpha = 0.7).  A label >= K draws nothing. */
int unet_latent_scatter(const int* centres, const uint8_t* labels, const uint8_t* palette, int K,
                        uint8_t* out, int N, int H, int W, int radius, unet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H_ */
