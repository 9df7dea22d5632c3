/*
 * fdet.h -- C-ABI of libfdet_hip.so: the MI355X (gfx950) hot path of a YOLO-style face
 * detector (training step + inference), drop-in for the arithmetic behind the Python
 * surface of smpurkis/PyTorch-Face-Detection-from-Scratch.
 *
 * The reference is pure Python and has no FFI of its own; each entry point below cites
 * the reference function (path:line under /root/reference) or the third-party kernel the
 * reference dispatches to that it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (hipMalloc'd / torch-ROCm storage) unless the
 *    parameter name starts with `h_`.  Tensors are dense, row-major, float32 unless noted;
 *    feature maps are NCHW.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call only
 *    enqueues work on that stream and returns; nothing synchronises, allocates or frees.
 *    The caller owns all buffers, including workspaces (sizes via the *_ws_bytes helpers).
 *  - Return value: 0 on success, negative FDET_E* on error (nothing is enqueued then);
 *    fdet_last_error() returns a thread-local message.  Never throws across the boundary.
 *  - No global mutable state: calls from different threads (e.g. the autograd worker) on
 *    different streams are safe.
 */
#ifndef FDET_H
#define FDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDET_VERSION 100           /* 0.1.0 */
#define FDET_OK 0
#define FDET_EINVAL (-1)           /* bad argument / unsupported shape */
#define FDET_ELAUNCH (-2)          /* hipLaunch failed (message holds hipGetErrorString) */
#define FDET_EWORKSPACE (-3)       /* workspace too small */

int fdet_version(void);
const char* fdet_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Detection math (bit-exact integer/index work, fp32 within 1e-4)
 * ------------------------------------------------------------------------------------- */

/* Grid-cell target encode.  Replaces WIDERFaceDataset.convert_bbx_to_feature_map,
 * datasets/WIDERFace/dataset.py:32-64, batched.
 *   boxes      [total,5] rows [conf,x,y,w,h] (pixel units), images concatenated
 *   box_offset [B+1] int32, image n owns rows box_offset[n] .. box_offset[n+1]-1
 *   out        [B,5,S,S]; fully written (zeros where no box)
 * Semantics kept: map dim1 indexes x; offsets use the UNCLAMPED cell index; cells are
 * clamped to [0,S-1]; the LAST box written to a cell wins. */
int fdet_encode_targets(const float* boxes, const int32_t* box_offset, int B, int S,
                        float img_w, float img_h, float* out, void* stream);

/* YOLO loss, forward + analytic backward in one pass.  Replaces losses/YoloLoss.py:4-44
 * called per image and summed over the batch (models/ModelMeta.py:173-176) plus autograd.
 *   pred, gt       [B,5,S,S]
 *   loss_per_image [B]   (written)
 *   loss_sum       [1]   (written; fixed-order sum of loss_per_image, deterministic)
 *   grad_pred      [B,5,S,S] = grad_scale * d loss_sum / d pred, or NULL to skip
 * Keeps: NaN->0.1 when nansum(pred_n)!=0 (:8-9), pred ch1/ch2 swap (:18), weights 3 and 1/S,
 * the x**0.5 backward singularity (0*inf = NaN as autograd produces). */
int fdet_yolo_loss_fwd_bwd(const float* pred, const float* gt, int B, int S,
                           float* loss_per_image, float* loss_sum, float* grad_pred,
                           float grad_scale, void* stream);

/* Threshold + affine decode + xywh->xyxy + round-half-even.  Replaces
 * ReduceBoundingBoxes.scale_batch_bbx_xywh / remove_low_probabilty_bbx /
 * convert_batch_to_xyxy / torch.round, datasets/utils.py:111-126,152-155,162, batched.
 *   maps   [B,5,S,S]
 *   scores [B,S*S]      candidates in row-major (i,j) order of `x[0] > pt` (strict)
 *   boxes  [B,S*S,4]    rounded x1,y1,x2,y2
 *   counts [B] int32    number of candidates per image */
int fdet_decode(const float* maps, int B, int S, float prob_threshold, float img_w, float img_h,
                float* scores, float* boxes, int32_t* counts, void* stream);

/* Greedy NMS, batched, one image per workgroup.  Replaces torchvision.ops.nms 0.11.2
 * (call site datasets/utils.py:164).  Stable descending-score order; fp32 overlap compared
 * against the double threshold; keep indices are returned in visiting order.
 *   boxes [B,Kmax,4] xyxy, scores [B,Kmax], counts [B] (candidates per image, <= Kmax)
 *   keep  [B,Kmax] int32 indices into the image's candidate list, keep_counts [B] int32
 * Kmax <= 4096. */
int fdet_nms(const float* boxes, const float* scores, const int32_t* counts, int B, int Kmax,
             double iou_threshold, int32_t* keep, int32_t* keep_counts, void* stream);

/* Fused ReduceBoundingBoxes.forward (datasets/utils.py:157-170) for a batch of maps:
 * decode -> NMS -> gather -> xyxy->xywh.
 *   out [B,S*S,5] rows [score,x,y,w,h] in keep order, out_counts [B] int32 */
int fdet_reduce_bounding_boxes(const float* maps, int B, int S, float prob_threshold,
                               double iou_threshold, float img_w, float img_h,
                               float* out, int32_t* out_counts, void* stream);

/* Step metrics.  Replaces the per-image block of ModelMeta.step, models/ModelMeta.py:199-214
 * (torchvision.ops.box_iou + counts), given the reduced boxes of targets and predictions.
 *   gt/pred [B,Kmax,5] rows [score,x,y,w,h], gt_counts/pred_counts [B]
 *   per_image [B,3]  (sum IoU, recall, precision) for each image (0 when no prediction)
 *   totals    [3]    fixed-order sums over the batch divided by B (:216-218) */
int fdet_step_metrics(const float* gt, const int32_t* gt_counts, const float* pred,
                      const int32_t* pred_counts, int B, int Kmax, float* per_image,
                      float* totals, void* stream);

/* uint8 -> float32 / 255 (true division).  Replaces `resize(x) / 255.0`,
 * models/PoolResnet.py:95, for inputs already at the model resolution (Resize is then the
 * identity round trip) and `img / 255`, datasets/WIDERFace/dataset.py:146. */
int fdet_u8_to_f32_norm(const uint8_t* in, float* out, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser
 * ------------------------------------------------------------------------------------- */

/* Adam on one flat parameter buffer.  Replaces torch.optim._multi_tensor.Adam.step reached
 * through SAMSGD.step, models/ModelMeta.py:12,81 (lr 1e-4, betas .9/.999, eps 1e-8, wd 0).
 * `step` is 1-based.  Hyper-parameters are doubles (Python floats in the reference; bias
 * corrections are formed in double and rounded once).  grad_scale multiplies the gradient
 * first (1.0 normally). */
int fdet_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                   int step, double lr, double beta1, double beta2, double eps, float grad_scale,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * SSD detection math (next row after the YOLO path; BASELINE.json config 4).  Priors are ordered
 * (scale, i, j); h_patch_sizes is a HOST array (reference: (60,30,15,7) -> P = 4774).
 * ------------------------------------------------------------------------------------- */
int fdet_ssd_num_priors(const int* h_patch_sizes, int nscales);
/* Multi-scale target encode: WIDERFaceDatasetSSD.convert_bbx_to_feature_map per scale + concat
 * (datasets/WIDERFace/dataset_ssd.py:36-76,134-139).  boxes/box_offsets as fdet_encode_targets;
 * out [B,P,5] rows [conf - 0.001*ps, off_x, off_y, w/W, h/H]. */
int fdet_ssd_encode_targets(const float* boxes, const int32_t* box_offsets, int B, const int* h_patch_sizes,
                            int nscales, float img_w, float img_h, float* out, void* stream);
/* ssd_loss(y_hat[:,:,0], y_hat[:,:,1:], y[:,:,0], y[:,:,1:], neg_pos_ratio) and its autograd
 * (losses/SSDLoss.py:25-86, models/ModelMetaSSD.py:127-129): per-image hard negative mining
 * (rank of -log(conf) among the negatives, ties by index), BCE over positives + mined negatives
 * with rounded labels, smooth-L1 over positives, divided by the batch's positive count.
 *   pred/target [B,P,5]; loss [1]; grad [B,P,5] or NULL; mask [B,P] (1 = contributes) or NULL.
 * A batch without a positive prior: loss = 0/0 = NaN as the reference, grad all zero as its autograd (nothing is selected). */
size_t fdet_ssd_loss_ws_bytes(int B);
int fdet_ssd_loss_fwd_bwd(const float* pred, const float* target, int B, int P, int neg_pos_ratio, float* loss,
                          float* grad, uint8_t* mask, void* ws, size_t ws_bytes, void* stream);
/* The same loss split at its only batch-wide quantity, for data-parallel training (the positive count of
 * losses/SSDLoss.py:86 is the count of the WHOLE batch): `parts` leaves the UNSCALED gradient of this rank's shard in
 * grad and the shard's three fp64 sums [BCE, smooth-L1, positive priors] in sums; the caller SUM-all-reduces the three
 * doubles; `finish` writes loss = (sums[1] + sums[0]) / sums[2] and scales grad by 1 / sums[2].  One rank: the pair
 * equals fdet_ssd_loss_fwd_bwd.  ws of `finish`: >= 16 bytes. */
int fdet_ssd_loss_parts(const float* pred, const float* target, int B, int P, int neg_pos_ratio, float* grad, uint8_t* mask,
                        double* sums, void* ws, size_t ws_bytes, void* stream);
int fdet_ssd_loss_finish(const double* sums, float* loss, float* grad, size_t n_grad, void* ws, size_t ws_bytes, void* stream);
/* ReduceSSDBoundingBoxes.forward for a batch (datasets/utils.py:54-92): decode (with_priors: scale by
 * 1/ps and add the cell origin), threshold (strict >), xyxy, round half even, greedy NMS, xywh.
 *   x [B,P,5]; out [B,P,5] rows [score,x,y,w,h] (first out_counts[n] rows valid). */
int fdet_ssd_reduce_bounding_boxes(const float* x, int B, const int* h_patch_sizes, int nscales, int with_priors,
                                   float prob_threshold, double iou_threshold, float img_w, float img_h,
                                   float* out, int32_t* out_counts, void* stream);
/* the same with a caller-supplied prior table: priors [P,4] on the device (ReduceSSDBoundingBoxes(priors=...),
 * datasets/utils.py:31-32: added to x, y, w, h after the 1/ps scaling of x, y), NULL = calculate_priors() */
int fdet_ssd_reduce_bounding_boxes_priors(const float* x, int B, const int* h_patch_sizes, int nscales, int with_priors,
                                          const float* priors, float prob_threshold, double iou_threshold, float img_w,
                                          float img_h, float* out, int32_t* out_counts, void* stream);

/* SSD heads (models/SSD.py:233-245,206-218): z [N,CP,ps,ps] holds Linear(C,5) of one scale in channels 0..4
 * (CP >= 5, extra channels ignored / zeroed); rows prior_start + i*ps + j of y [N,P,5] get
 * [sigmoid(z0), z1/ps + i/ps, z2/ps + j/ps, z3, z4].  _bwd maps d loss/d y back to dz (needs y for the sigmoid). */
int fdet_ssd_head_pack_fwd(const float* z, int N, int CP, int ps, int prior_start, int P, float* y, void* stream);
int fdet_ssd_head_pack_bwd(const float* dy, const float* y, int N, int CP, int ps, int prior_start, int P, float* dz,
                           void* stream);

/* Bilinear Resize fused with the /255 normalisation: replaces `self.resize(x) / 255.0`
 * (models/PoolResnet.py:91,95; models/Resnet.py likewise) and `Resize(...)(x); x / 255.0`
 * (models/BaseModel.py:64-65), i.e. torchvision 0.11.2 transforms.Resize on tensors =
 * F.interpolate(mode="bilinear", align_corners=False), no antialias.
 *   u8 : src [N,C,Hs,Ws] uint8 -> dst [N,C,Hd,Wd] f32 = round_half_even(interp) / 255   (the uint8 round trip)
 *   f32: src [N,C,Hs,Ws] f32   -> dst = interp / divisor                                 (no rounding)
 * Same-size dimensions are the identity. */
int fdet_resize_bilinear_u8_norm(const uint8_t* src, float* dst, int N, int C, int Hs, int Ws,
                                 int Hd, int Wd, void* stream);
int fdet_resize_bilinear_f32_norm(const float* src, float* dst, int N, int C, int Hs, int Ws,
                                  int Hd, int Wd, float divisor, void* stream);

/* ---------------------------------------------------------------------------------------
 * Conv stack (PoolResnet / Resnet): fp32 implicit GEMM on v_mfma_f32_32x32x2_f32
 * ------------------------------------------------------------------------------------- */

/* Repack OIHW 3x3 weights [Cout,Cin,3,3] into the two K-major panels the conv kernels read:
 *   wpk_fwd [Cin*9][CoutP]  k=(ci,tap)          A panel of the forward conv
 *   wpk_bwd [Cout*9][CinP]  k=(co,flipped tap)  A panel of the data-gradient conv
 * CoutP/CinP = channel count rounded up to 32 (zero padded).  Either output may be NULL. */
int fdet_pack_conv3x3_weights(const float* w, int Cout, int Cin, float* wpk_fwd, float* wpk_bwd,
                              void* stream);

/* 3x3 stride-1 pad-1 convolution with fused tail.  Replaces nn.Conv2d + LeakyReLU(0.2)
 * [+ Dropout2d + skip add + MaxPool2d(2)] of ResidualBlock.forward,
 * models/PoolResnet.py:33-43 (models/Resnet.py:30-40).
 *   x [N,Cin,H,W], wpk = wpk_fwd of fdet_pack_conv3x3_weights, bias [Cout]
 *   z = lrelu(conv(x)+bias, slope)
 *   y_full [N,Cout,H,W]  = z                         (NULL to skip; saved for backward)
 *   y_out  [N,Cout,H,W] = z*drop_scale[n,c] + skip      (NULL to skip; un-pooled tail)
 *   skip [N,Cout,H,W] or NULL; drop_scale [N,Cout] or NULL (eval).
 * `pool` must be 1: blocks that pool write y_full here and finish in fdet_block_tail_fwd. */
int fdet_conv3x3_fwd(const float* x, const float* wpk, const float* bias, float* y_full,
                     const float* skip, const float* drop_scale, float* y_out,
                     int N, int Cin, int Cout, int H, int W, int pool, float slope, void* stream);

/* Data gradient of the 3x3 conv with fused tail (autograd of the above):
 *   dx = conv_transpose(dz) * lrelu'(act) + add
 *   dz [N,Cout,H,W], wpk = wpk_bwd, act [N,Cin,H,W] or NULL (lrelu'(a)=1 if a>0 else slope),
 *   add [N,Cin,H,W] or NULL, dx [N,Cin,H,W]. */
int fdet_conv3x3_dgrad(const float* dz, const float* wpk, const float* act, const float* add,
                       float* dx, int N, int Cin, int Cout, int H, int W, float slope, void* stream);

/* bf16x3 variants of the three entry points above: identical arguments and results within ~1e-5
 * (tests: 1e-4), computed on v_mfma_f32_32x32x16_bf16 with every fp32 operand split into two
 * bf16 values (x = hi + lo; products a_hi*b_lo + a_lo*b_hi + a_hi*b_hi, fp32 accumulation).
 * ~5x the MFMA rate of the fp32 path: the convs become HBM-bound.  Channel counts must be
 * multiples of 16.  The packed panels hold [hi | lo] bf16 and are EXACTLY as large as the fp32
 * panels (same buffers can be reused); they are not interchangeable with them. */
int fdet_pack_conv3x3_weights_bf16x3(const float* w, int Cout, int Cin, void* wpk_fwd, void* wpk_bwd,
                                     void* stream);
/* L same-shape layers in one launch; h_* are HOST arrays of L device pointers (either panel array may be NULL). */
int fdet_pack_conv3x3_weights_bf16x3_batched(const float* const* h_w, int L, int Cout, int Cin,
                                             void* const* h_wpk_fwd, void* const* h_wpk_bwd, void* stream);
int fdet_conv3x3_fwd_bf16x3(const float* x, const void* wpk, const float* bias, float* y_full,
                            const float* skip, const float* drop_scale, float* y_out,
                            int N, int Cin, int Cout, int H, int W, int pool, float slope, void* stream);
int fdet_conv3x3_dgrad_bf16x3(const float* dz, const void* wpk, const float* act, const float* add,
                              float* dx, int N, int Cin, int Cout, int H, int W, float slope, void* stream);

/* Weight + bias gradient of the 3x3 conv: dW[co,ci,ky,kx] = sum_{n,y,x} dz*x_shifted,
 * db[co] = sum dz.  Deterministic two-pass (per-workgroup slabs in `ws`, then a fixed-order
 * reduce).  dW [Cout,Cin,3,3], db [Cout] are overwritten. */
size_t fdet_conv3x3_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W);
int fdet_conv3x3_wgrad(const float* x, const float* dz, float* dW, float* db, void* ws,
                       size_t ws_bytes, int N, int Cin, int Cout, int H, int W, void* stream);

/* bf16x3 variant of the weight gradient (same arguments/results within ~1e-5 of the tensor's scale;
 * see the bf16x3 note above).  Rows of up to 16 vector lanes (VW = 4, 2, 1 floats for W%4==0, W%2==0,
 * else) are staged whole; wider rows need W % 4 == 0 and are cut into 56-column segments.
 * fdet_conv3x3_wgrad_bf16x3_ws_bytes returns 0 when the shape is not supported. */
size_t fdet_conv3x3_wgrad_bf16x3_ws_bytes(int N, int Cin, int Cout, int H, int W);
int fdet_conv3x3_wgrad_bf16x3(const float* x, const float* dz, float* dW, float* db, void* ws,
                              size_t ws_bytes, int N, int Cin, int Cout, int H, int W, void* stream);

/* Batched form: L <= 16 same-shape layers in ONE launch (+ one reduce launch).  h_x / h_dz / h_dW /
 * h_db are HOST arrays of L device pointers.  Small layers (15x15) are launch/reduction-overhead
 * bound one at a time; batched, every workgroup owns bands of a single layer and writes one slab. */
size_t fdet_conv3x3_wgrad_bf16x3_batched_ws_bytes(int L, int N, int Cin, int Cout, int H, int W);
/* Plan query of the bf16x3 / precision16 weight gradient of L layers (launches nothing): fills out[0..min(n,8)-1] with
 * ok, pipelined kernel, 32-lane rows (lpr32), float4 quads (pk4), a reserved slot (pack: always 0), vector width, output-channel
 * tiles (MTC) and column segments (NSEG).  ok == 0 exactly when the entry points refuse the shape. */
int fdet_conv3x3_wgrad_bf16x3_plan(int N, int Cin, int Cout, int H, int W, int L, int* out, int n);
int fdet_conv3x3_wgrad_bf16x3_batched(const float* const* h_x, const float* const* h_dz, float* const* h_dW,
                                      float* const* h_db, int L, void* ws, size_t ws_bytes,
                                      int N, int Cin, int Cout, int H, int W, void* stream);

/* Residual-block CHAIN at one resolution, running activation resident in LDS (bf16x3 arithmetic).
 * `nblocks` consecutive un-pooled ResidualBlocks (models/PoolResnet.py:33-43 / models/Resnet.py:30-40 with
 * pool == 1) in ONE launch, one workgroup per image; HBM only sees the tensors kept for backward.
 * Needs 64 channels and H*roundup4(W+1) <= 256 (15x15, 10x10 ...): fdet_block_chain_supported.
 * All h_* arguments are HOST arrays of `nblocks` DEVICE pointers.
 *   forward : a_k = lrelu(conv1_k(h)); c_k = lrelu(conv2_k(a_k)); h <- c_k*scale_k[n,f] + h
 *     x [N,64,H,W]; h_wpk1/h_wpk2: forward panels of fdet_pack_conv3x3_weights_bf16x3; h_b1/h_b2 biases;
 *     h_scale: [N,64] dropout scales (array or entries NULL = eval); h_a/h_c: where to keep a_k / c_k
 *     (array or entries NULL: not kept); h_out: block outputs (entries may be NULL except the last).
 *   backward: dz2_k = dout*scale_k*lrelu'(c_k); dz1_k = conv2_k^T(dz2_k)*lrelu'(a_k);
 *             dout <- conv1_k^T(dz1_k) + dout, for k = nblocks-1 .. 0; dx = final dout.
 *     h_wpk1b/h_wpk2b: backward panels; h_dz1/h_dz2 [N,64,H,W] are written (operands of the weight gradients). */
int fdet_block_chain_supported(int F, int H, int W);
/* Plan query (launches nothing): the chain kernels run N images of this map (batch-size limits included); ps = 1: the PS
 * flavour (fdet_block_chain_fwd_ps / _bwd_ps).  The entry points refuse exactly what this refuses. */
int fdet_block_chain_ok(int N, int F, int H, int W, int ps);
int fdet_block_chain_fwd_bf16x3(const float* x, const void* const* h_wpk1, const float* const* h_b1,
                                const void* const* h_wpk2, const float* const* h_b2,
                                const float* const* h_scale, float* const* h_a, float* const* h_c,
                                float* const* h_out, int nblocks, int N, int F, int H, int W, float slope,
                                void* stream);
int fdet_block_chain_bwd_bf16x3(const float* dout, const void* const* h_wpk1b, const void* const* h_wpk2b,
                                const float* const* h_scale, const float* const* h_a, const float* const* h_c,
                                float* const* h_dz1, float* const* h_dz2, float* dx, int nblocks, int N, int F,
                                int H, int W, float slope, void* stream);

/* The same chain with the tensors kept per block in the engine's PS layout (csrc/fdet_ps.h; PS image-0 pointers):
 *   forward : h_a_ps[k] (both planes) and h_out_ps[k], k < nblocks-1 (both planes) are operands of the weight gradients,
 *             h_c_ps[k] receives the hi plane only (backward needs the signs of c_k); arrays or entries may be NULL
 *             (not kept).  The last block's output is written to out_last as fp32 NCHW.  x: fp32 NCHW, or PS if x_is_ps.
 *   backward: dout, dx fp32 NCHW; h_dz1_ps / h_dz2_ps are written as PS.
 * No reference counterpart beyond the one of fdet_block_chain_*_bf16x3; values are identical to that flavour's
 * (a PS element is the fp32 value rounded to its bf16 hi + lo parts, which is all the bf16x3 consumers read). */
int fdet_block_chain_fwd_ps(const void* x, int x_is_ps, const void* const* h_wpk1, const float* const* h_b1,
                            const void* const* h_wpk2, const float* const* h_b2, const float* const* h_scale,
                            void* const* h_a_ps, void* const* h_c_ps, void* const* h_out_ps, float* out_last,
                            int nblocks, int N, int F, int H, int W, float slope, void* stream);
int fdet_block_chain_bwd_ps(const float* dout, const void* const* h_wpk1b, const void* const* h_wpk2b,
                            const float* const* h_scale, const void* const* h_a_ps, const void* const* h_c_ps,
                            void* const* h_dz1_ps, void* const* h_dz2_ps, float* dx, int nblocks, int N, int F,
                            int H, int W, float slope, void* stream);

/* Residual-block tail for pooled blocks: out = maxpool_pool(c*drop_scale[n,f] + x)
 * (Dropout2d + skip add + MaxPool2d(2), models/PoolResnet.py:39-42).  pool in {1,2}.
 *   c,x [N,F,H,W]; drop_scale [N,F] or NULL; out [N,F,H/pool,W/pool] (floor: an odd last row/column is dropped). */
int fdet_block_tail_fwd(const float* c, const float* x, const float* drop_scale, float* out,
                        int N, int F, int H, int W, int pool, void* stream);

/* Pooled residual block with the tail fused into the convolutions (bf16x3, maps of even height and even width
 * <= 62; Cout % 32 == 0).  Replaces conv2 + LeakyReLU + Dropout2d + skip + MaxPool2d(2) of
 * models/PoolResnet.py:36-42 (models/Resnet.py:33-39) and their autograd without ever writing c = lrelu(conv2):
 *   forward : out_pooled [N,Cout,H/2,W/2] = maxpool2x2(lrelu(conv(x)+bias) * drop_scale + skip)
 *             route [N,Cout,H/2,W/2] uint8 (NULL in eval): bits 0-3 = (c > 0) of the window's four elements in
 *             ATen scan order (row-major), bits 4-5 = index of the maximum (first maximum wins, NaN is a maximum)
 *   backward: fdet_pool_route_bwd        dz2 [N,F,H,W] = unpool(dout_pooled) * drop_scale * lrelu'(c)
 *             fdet_conv3x3_dgrad_unpool  dx = conv^T(dz) + unpool(dout_pooled)      (conv1's data gradient + skip path)
 * wpk: forward / backward panels of fdet_pack_conv3x3_weights_bf16x3. */
int fdet_conv3x3_pool_fusion_ok(int N, int Cin, int Cout, int H, int W);   /* 1: the two kernels below have a tiling for the shape */
/* Diagnostic: the route of the last fdet_conv3x3_{fwd,dgrad}[_pool|_unpool]_bf16{x3,} call on the calling thread, as
 * recorded where the launch was issued: out[0..min(n,6)-1] = kernel family (1 ping-pong, 2 aligned-band small-tile,
 * 3 small-tile, 4 general persistent), vector width, output-channel tiles (MT), epilogue mode (EPI_* of
 * csrc/fdet_conv_common.h), column-segmented rows (0/1), precision16 (0/1).  All zero after a refused call. */
int fdet_conv3x3_x3_last_route(int* out, int n);
/* Plan query of the PS conv kernels (fdet_conv3x3_ps_*; launches nothing): 1 when they accept N images of this shape.
 * pooled: 0 = conv / data gradient, 1 = pooled block with an fp32 pooled output (and its backward), 2 = pooled block
 * with a PS pooled output.  The entry points refuse exactly what this refuses. */
int fdet_conv3x3_ps_ok(int N, int Cin, int Cout, int H, int W, int pooled);
int fdet_conv3x3_fwd_pool_bf16x3(const float* x, const void* wpk, const float* bias, const float* skip,
                                 const float* drop_scale, float* out_pooled, unsigned char* route, int N, int Cin,
                                 int Cout, int H, int W, float slope, void* stream);
int fdet_conv3x3_dgrad_unpool_bf16x3(const float* dz, const void* wpk, const float* dout_pooled,
                                     const unsigned char* route, float* dx, int N, int Cin, int Cout, int H, int W,
                                     float slope, void* stream);
int fdet_pool_route_bwd(const float* dout_pooled, const unsigned char* route, const float* drop_scale, float* dz2,
                        int N, int F, int H, int W, float slope, void* stream);

/* Engine-private PRE-SPLIT ("PS") activations of the bf16x3 conv stack (csrc/fdet_ps.h): a feature map [N,C,H,W]
 * (C % 8 == 0, W <= 62) kept as bf16 hi | lo planes with 8 channels innermost, rows padded to 16/32/64 slots with
 * zero halo slots, zero rows between images -- the layout the MFMA operands have in LDS, so the conv kernels stage
 * it with LDS-DMA and their epilogues write it for the next consumer.  Same bytes per element as fp32.  No
 * counterpart in the reference (its tensors are fp32 NCHW: models/PoolResnet.py:33-43); fp32 NCHW stays the format at
 * every C-ABI boundary that mirrors a reference interface.
 *   fdet_ps_bytes          allocation size in bytes (includes one all-zero guard image on either side; the caller
 *                          zero-fills the allocation ONCE, producers write real elements only); 0 = unsupported shape
 *   fdet_ps_image0_offset  byte offset of image 0 inside the allocation: the pointer every other call takes
 *   fdet_ps_from_f32 / fdet_ps_to_f32   converters (value = float(hi) + float(lo), 16 significant bits) */
size_t fdet_ps_bytes(int N, int C, int H, int W);
size_t fdet_ps_image0_offset(int N, int C, int H, int W);
int fdet_ps_from_f32(const float* x, void* ps, int N, int C, int H, int W, void* stream);
int fdet_ps_to_f32(const void* ps, float* x, int N, int C, int H, int W, void* stream);
/* Column strips (round 4; config 3's 320 / 160 / 80-column maps, models/Resnet.py:30-40): an even map wider than 63 columns is
 * kept as S = fdet_ps_strips(W) strips of <= 62 columns, each a PS image of its own whose edge slots hold the neighbour
 * strip's column.  Every fdet_*_ps entry point takes the FULL width and plans the strips itself; the caller's part is
 *   fdet_ps_halo_exchange(zero_only = 0)  after a producer that writes real elements only (a conv epilogue,
 *                                         fdet_pool_route_bwd_ps) and before a 3x3 conv reads the tensor;
 *   fdet_ps_halo_exchange(zero_only = 1)  before the tensor is the dz operand of fdet_conv3x3_wgrad_ps_batched (a halo slot
 *                                         is not a position of its strip) when its halo slots may hold columns;
 * fdet_ps_from_f32 writes the halos itself.  Both are no-ops on plain (<= 63-column) tensors. */
int fdet_ps_strips(int W);
int fdet_ps_halo_exchange(void* ps, int N, int C, int H, int W, int zero_only, int hi_only, void* stream);
/* 3x3 convs on PS tensors (Cout == 64, Cin % 16 == 0, maps of 15..62 columns, or wider even maps as column strips); wpk: forward / backward panels of
 * fdet_pack_conv3x3_weights_bf16x3.  Same arithmetic as fdet_conv3x3_fwd_bf16x3 / fdet_conv3x3_dgrad_bf16x3
 * (models/PoolResnet.py:33-36 and its autograd):
 *   fwd      : y_ps  = LeakyReLU(conv(x_ps) + bias)
 *   dgrad_act: dx_ps = conv^T(dz_ps) * LeakyReLU'(act_ps) */
int fdet_conv3x3_ps_fwd(const void* x_ps, const void* wpk, const float* bias, void* y_ps, int N, int Cin, int Cout,
                        int H, int W, float slope, void* stream);
int fdet_conv3x3_ps_dgrad_act(const void* dz_ps, const void* wpk, const void* act_ps, void* dx_ps, int N, int Cin,
                              int Cout, int H, int W, float slope, void* stream);

/* Pooled residual block on PS tensors (models/PoolResnet.py:36-42 and its autograd; 64 channels, even maps), the tail
 * fused into the convolutions as in fdet_conv3x3_fwd_pool_bf16x3 / fdet_conv3x3_dgrad_unpool_bf16x3 / fdet_pool_route_bwd:
 *   fwd_pool     : pooled = maxpool2x2(lrelu(conv(x_ps)+bias) * drop_scale + skip_ps) -> pool_ps (PS, may be NULL) and / or
 *                  pool_f32 (fp32 NCHW, may be NULL); route8 [N][8][H/2][W/2][8] uint8 (channel-innermost routing bytes,
 *                  NULL in eval): bits 0-3 = (c > 0) of the window's four elements in scan order, bits 4-5 = argmax
 *                  (first maximum wins, NaN is a maximum)
 *   route_bwd    : dz2_ps = unpool(dout_pooled) * drop_scale * lrelu'(c)        (dout_pooled: fp32 NCHW)
 *   dgrad_unpool : dx (fp32 NCHW) = conv^T(dz_ps) + unpool(dout_pooled) */
int fdet_conv3x3_ps_fwd_pool(const void* x_ps, const void* wpk, const float* bias, const void* skip_ps,
                             const float* drop_scale, void* pool_ps, float* pool_f32, unsigned char* route8, int N, int Cin,
                             int Cout, int H, int W, float slope, void* stream);
int fdet_pool_route_bwd_ps(const float* dout_pooled, const unsigned char* route8, const float* drop_scale, void* dz2_ps,
                           int N, int C, int H, int W, float slope, void* stream);
int fdet_conv3x3_ps_dgrad_unpool(const void* dz_ps, const void* wpk, const float* dout_pooled, const unsigned char* route8,
                                 float* dx, int N, int Cin, int Cout, int H, int W, float slope, void* stream);
/* The PoolResnet stem Conv2d(3,64,10,s8,p2)+bias (models/PoolResnet.py:70-72) writing its output as a PS tensor
 * (image-0 pointer of an (N,64,Ho,Wo) PS allocation): same arithmetic as fdet_stem_fwd_bf16x3. */
int fdet_stem_fwd_ps(const float* x, const float* w, const float* bias, void* y_ps, int N, int Cin, int F, int H, int W,
                     int k, int stride, int pad, void* stream);
/* Weight / bias gradients of L same-shape 64-channel 3x3 layers from PS tensors (h_x[l], h_dz[l]: host arrays of
 * image-0 device pointers): dW[l] [64,64,3,3], db[l] [64] (autograd of models/PoolResnet.py:33-36; same results as
 * fdet_conv3x3_wgrad_bf16x3_batched to the rounding of the PS format).  ws: fdet_conv3x3_wgrad_ps_ws_bytes bytes
 * (0 = unsupported shape).  Deterministic (fixed-order slab reduction). */
size_t fdet_conv3x3_wgrad_ps_ws_bytes(int L, int N, int C, int H, int W);
int fdet_conv3x3_wgrad_ps_batched(const void* const* h_x, const void* const* h_dz, float* const* h_dW, float* const* h_db,
                                  int L, int N, int C, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* Pointwise (1x1) convolution / per-position Linear layer as a dense GEMM on the matrix cores, bf16x3 arithmetic
 * (fp32-level accuracy).  Replaces nn.Conv2d(Cin, Cout, 1) of SeparableResidualBlock.pointwise_conv_skip
 * (models/SSD.py:24-30) and nn.Linear(C, 5) applied at every position (models/SSD.py:183-185) and their autograd.
 * Tensors are [N, C, P] fp32 with P = H*W positions per image (NCHW); any Cin / Cout >= 1.
 *   pack : w [Cout,Cin] -> K-major bf16 hi|lo panels; each buffer fdet_pointwise_packed_bytes(Cout, Cin) bytes
 *   fwd  : y = lrelu_slope(W x + bias)         (slope 1 = identity; bias may be NULL)
 *   dgrad: dx = W^T dz (+ add, may be NULL)
 *   wgrad: dW [Cout,Cin] = sum_{n,p} dz x^T ; db [Cout] = sum dz (db may be NULL); deterministic slab reduction;
 *          ws: fdet_pointwise_wgrad_ws_bytes(N, Cin, Cout, P) bytes of device scratch. */
size_t fdet_pointwise_packed_bytes(int Cout, int Cin);
int fdet_pack_pointwise_weights_bf16x3(const float* w, int Cout, int Cin, void* wpk_fwd, void* wpk_bwd, void* stream);
int fdet_pointwise_fwd_bf16x3(const float* x, const void* wpk_fwd, const float* bias, float* y, int N, int Cin, int Cout,
                              int P, float slope, void* stream);
int fdet_pointwise_dgrad_bf16x3(const float* dz, const void* wpk_bwd, const float* add, float* dx, int N, int Cin,
                                int Cout, int P, void* stream);
size_t fdet_pointwise_wgrad_ws_bytes(int N, int Cin, int Cout, int P);
int fdet_pointwise_wgrad_bf16x3(const float* x, const float* dz, float* dW, float* db, void* ws, size_t ws_bytes, int N,
                                int Cin, int Cout, int P, void* stream);
/* precision16 twins (the one-pass contract of fdet_conv3x3_*_bf16 below): same arguments, panels
 * (fdet_pack_pointwise_weights_bf16x3, hi half read only) and workspace size (fdet_pointwise_wgrad_ws_bytes).  Operands
 * rounded to bf16 (RNE), ONE v_mfma_f32_32x32x16_bf16 per (m, n) tile, fp32 accumulation and epilogue (bias, slope, add);
 * every stored y / dx rounded once to bf16 in its fp32 word; dW / db fp32 sums over bf16 operands (db = sum of bf16(dz)). */
int fdet_pointwise_fwd_bf16(const float* x, const void* wpk_fwd, const float* bias, float* y, int N, int Cin, int Cout,
                            int P, float slope, void* stream);
int fdet_pointwise_dgrad_bf16(const float* dz, const void* wpk_bwd, const float* add, float* dx, int N, int Cin,
                              int Cout, int P, void* stream);
int fdet_pointwise_wgrad_bf16(const float* x, const float* dz, float* dW, float* db, void* ws, size_t ws_bytes, int N,
                              int Cin, int Cout, int P, void* stream);

/* MobileNetV3-small backbone, inference, bf16 (BASELINE.json config 5).  Replaces the forward of
 * models/MobilenetV3Backbone.py:35-60 (timm tf_mobilenetv3_small_100 feature extractor + Conv2d(576,5,3,p1) + sigmoid).
 * Engine-private activations are NHWC bf16 ([N][H][W][C], C % 8 == 0); BatchNorm (eps 1e-3) is folded into the conv
 * weights by the caller.  act: 0 none, 1 ReLU, 2 Hardswish.
 *   fdet_mb_stem      x [N,3,H,W] f32 in [0,1] (x_is_u8: uint8, divided by 255) -> y [N,H/2,W/2,16]; Conv2dSame(3,16,3,s2)
 *                     with folded weights w [16][3][3][3] f32, bias [16], then Hardswish
 *   fdet_mb_depthwise KxK (3|5) depthwise, stride 1 (pad K/2) or 2 (TF "SAME"); w [K*K][C] f32, bias [C]; y [N,Ho,Wo,C];
 *                     pool [N][slots][C] f32 (or NULL), slots = fdet_mb_depthwise_pool_slots(...): per-image partial channel
 *                     sums of y, one row per workgroup column (SqueezeExcite numerators; no atomics: bit-reproducible)
 *   fdet_mb_se_gate   gate [N][C] = hardsigmoid(W2 relu(W1 (sum of the pool rows / HW) + b1) + b2); w1 [R][C], w2 [C][R] f32
 *   fdet_mb_pointwise y [N,P,Cout] = act(W (x * gate) + bias) (+ res); x [N,P,Cin]; w bf16 [ceil32(Cout)][ceil16(Cin)] zero
 *                     padded; bias f32 [ceil32(Cout)]; gate [N][Cin] or NULL; res [N,P,Cout] or NULL
 *   fdet_mb_head      y [N,5,S,S] f32 = sigmoid(Conv2d(C,5,3,p1)(f)); f [N,S,S,C] bf16 (C % 16 == 0); w bf16 [2][64][C]: row
 *                     tap*5 + ch of the fp32 weight (rows 45..63 zero) split into hi = bf16(w) and lo = bf16(w - hi); bias [5]
 *                     f32; ws >= fdet_mb_head_ws_bytes(N, S) (the 45 per-position tap products, f32) */
int fdet_mb_stem(const void* x, int x_is_u8, const float* w, const float* bias, void* y, int N, int H, int W, void* stream);
int fdet_mb_depthwise(const void* x, const float* w, const float* bias, void* y, float* pool, int N, int H, int W, int C,
                      int K, int stride, int act, void* stream);
int fdet_mb_depthwise_pool_slots(int N, int H, int W, int C, int K, int stride);
int fdet_mb_se_gate(const float* pool, int slots, int HW, const float* w1, const float* b1, const float* w2, const float* b2,
                    int N, int C, int R, float* gate, void* stream);
int fdet_mb_pointwise(const void* x, const void* w, const float* bias, const float* gate, const void* res, void* y, int N,
                      int P, int Cin, int Cout, int act, void* stream);
size_t fdet_mb_head_ws_bytes(int N, int S);
int fdet_mb_head(const void* f, const void* w, const float* bias, float* y, void* ws, size_t ws_bytes, int N, int S, int C,
                 void* stream);

/* Backward of the residual-block tail (dropout, skip, max-pool, second LeakyReLU):
 *   e = c*drop_scale + x ; out = maxpool(e) ; given dout [N,F,H/pool,W/pool]:
 *   de = unpool(dout) (first max in window scan order wins, as ATen max_pool2d backward)
 *   dz2 = de * drop_scale * lrelu'(c)
 *   c,x [N,F,H,W]; dz2 [N,F,H,W]; de [N,F,H,W] written only if pool==2 (else de==dout, may be NULL). */
int fdet_block_tail_bwd(const float* dout, const float* c, const float* x, const float* drop_scale,
                        float* dz2, float* de, int N, int F, int H, int W, int pool, float slope,
                        void* stream);

/* Stem convolution (no activation).  Replaces nn.Conv2d(3,F,k,stride,pad) of
 * models/PoolResnet.py:70-76,98 (k10 s8 p2) and models/Resnet.py:64-70 (k3 s2 p1); other
 * (k,stride,pad) return FDET_EINVAL.
 *   x [N,Cin,H,W], w [F,Cin,k,k] (OIHW), bias [F], y [N,F,Ho,Wo].
 * `ws` (fdet_stem_ws_bytes) holds the K-major weight panel the kernel reads (rebuilt per
 * call) and, for the weight gradient, the per-workgroup slabs of the fixed-order reduction. */
size_t fdet_stem_ws_bytes(int N, int Cin, int F, int H, int W, int k, int stride, int pad);
int fdet_stem_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes,
                  int N, int Cin, int F, int H, int W, int k, int stride, int pad, void* stream);
/* bf16x3 variant of fdet_stem_fwd (PoolResnet geometry only: 3 channels, k10 s8 p2); same
 * arguments, results within ~1e-5.  `ws` is unused. */
int fdet_stem_fwd_bf16x3(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes,
                         int N, int Cin, int F, int H, int W, int k, int stride, int pad, void* stream);
/* dW [F,Cin,k,k], db [F] from x and dy [N,F,Ho,Wo] (autograd of the stem; the input image
 * needs no gradient, so there is no data-gradient entry point). */
int fdet_stem_wgrad(const float* x, const float* dy, float* dW, float* db, void* ws, size_t ws_bytes,
                    int N, int Cin, int F, int H, int W, int k, int stride, int pad, void* stream);
/* bf16x3 variant of fdet_stem_wgrad (PoolResnet geometry, W % 16 == 0); same workspace size. */
int fdet_stem_wgrad_bf16x3(const float* x, const float* dy, float* dW, float* db, void* ws, size_t ws_bytes,
                           int N, int Cin, int F, int H, int W, int k, int stride, int pad, void* stream);

/* Head: Dropout2d(0.5) + Conv2d(F,5,k,pad) + Sigmoid.  Replaces models/PoolResnet.py:100-102
 * (k6 p0) and models/Resnet.py:94-96 (k3 p1).
 *   x [N,F,H,W], drop_scale [N,F] or NULL, w [5,F,k,k], bias [5], y [N,5,S,S] (post-sigmoid). */
int fdet_head_fwd(const float* x, const float* drop_scale, const float* w, const float* bias,
                  float* y, int N, int F, int H, int W, int k, int pad, void* stream);
/* Backward of the head given dy = d loss / d y (post-sigmoid):
 *   dx [N,F,H,W] (includes drop_scale), dW [5,F,k,k], db [5]. */
size_t fdet_head_bwd_ws_bytes(int N, int F, int H, int W, int k, int pad);
int fdet_head_bwd(const float* x, const float* drop_scale, const float* w, const float* y,
                  const float* dy, float* dx, float* dW, float* db, void* ws, size_t ws_bytes,
                  int N, int F, int H, int W, int k, int pad, void* stream);

/* precision16 (round 4): the PS kernels with ONE bf16 MFMA pass on the hi planes -- bf16 activations and weights, fp32
 * accumulation, fp32 epilogue arithmetic and fp32 master weights / gradients: the arithmetic of the reference's
 * Trainer(precision=16) (train_model.py:50) with bf16 as the 16-bit type.  Same arguments as the functions without the
 * suffix; the PS tensors they produce hold their hi plane only (the lo plane is left untouched: zero in a buffer that only
 * ever served this mode). */
int fdet_conv3x3_ps_fwd_p16(const void* x_ps, const void* wpk, const float* bias, void* y_ps, int N, int Cin,
                            int Cout, int H, int W, float slope, void* stream);
int fdet_conv3x3_ps_dgrad_act_p16(const void* dz_ps, const void* wpk, const void* act_ps, void* dx_ps, int N,
                                  int Cin, int Cout, int H, int W, float slope, void* stream);
int fdet_conv3x3_ps_fwd_pool_p16(const void* x_ps, const void* wpk, const float* bias, const void* skip_ps,
                                 const float* drop_scale, void* pool_ps, float* pool_f32, unsigned char* route8,
                                 int N, int Cin, int Cout, int H, int W, float slope, void* stream);
int fdet_conv3x3_ps_dgrad_unpool_p16(const void* dz_ps, const void* wpk, const float* dout_pooled,
                                     const unsigned char* route8, float* dx, int N, int Cin, int Cout, int H, int W,
                                     float slope, void* stream);
int fdet_pool_route_bwd_ps_p16(const float* dout_pooled, const unsigned char* route8, const float* drop_scale,
                               void* dz2_ps, int N, int C, int H, int W, float slope, void* stream);
int fdet_stem_fwd_ps_p16(const float* x, const float* w, const float* bias, void* y_ps, int N, int Cin, int F, int H,
                         int W, int k, int stride, int pad, void* stream);
/* Inference: the PoolResnet stem on the uint8 FRAMES themselves: the `x / 255.0` of models/PoolResnet.py:95 (models/BaseModel.py:65)
 * happens in the stem's staging (a 256-entry table of the bf16 hi | lo parts of p / 255), results identical to
 * fdet_u8_to_f32_norm + fdet_stem_fwd_ps, and the fp32 image is never written.  frames: [N][3][H][W] uint8, 4-byte aligned,
 * W % 4 == 0; precision16 != 0: one MFMA pass, hi plane only. */
int fdet_stem_fwd_ps_u8(const unsigned char* frames, const float* w, const float* bias, void* y_ps, int N, int Cin, int F, int H,
                        int W, int k, int stride, int pad, int precision16, void* stream);
/* precision16 stem weight gradient (one MFMA pass on bf16(dy) x bf16(x), fp32 sums; the workspace of fdet_stem_wgrad_bf16x3):
 * the PoolResnet stem (k10 s8 p2) and the Resnet / SSD stem (3ch k3 s2 p1, the shapes of its bf16x3 matrix-core kernel). */
int fdet_stem_wgrad_bf16(const float* x, const float* dy, float* dW, float* db, void* ws, size_t ws_bytes,
                         int N, int Cin, int F, int H, int W, int k, int stride, int pad, void* stream);
/* Plan queries of the stem (launch nothing; the entry points refuse exactly what these refuse, batch sizes included):
 *   fdet_stem_fwd_ps_ok    fdet_stem_fwd_ps / _p16 (u8 = 0) or fdet_stem_fwd_ps_u8 (u8 = 1) accept N images of this shape
 *   fdet_stem_wgrad_x3_ok  fdet_stem_wgrad_bf16x3 (precision16 = 0) or fdet_stem_wgrad_bf16 (precision16 = 1) do
 * The PoolResnet stem runs batches beyond the 32-bit offsets of its pipelined kernels as consecutive launches over image
 * chunks; its weight gradient sums the per-workgroup partials of every chunk in one reduction (fdet_stem_ws_bytes). */
int fdet_stem_fwd_ps_ok(int N, int Cin, int F, int H, int W, int k, int stride, int pad, int precision16, int u8);
int fdet_stem_wgrad_x3_ok(int N, int Cin, int F, int H, int W, int k, int stride, int pad, int precision16);
/* Diagnostic: what the last fdet_stem_{fwd,wgrad}* call on the calling thread launched, recorded where the launch was
 * issued: out[0..min(n,8)-1] = kernel family (FDET_STEM_*), pass (1 forward, 2 weight gradient), precision16 (0/1), uint8
 * input (0/1), PS output (0/1), launches of the main kernel (image chunks), gridDim.x and work items (output rows, or
 * row x 64-column segment items of the scalar-fed kernel) of the first launch.  All zero after a refused call. */
#define FDET_STEM_VALU_K10 1         /* fp32 VALU, k10 s8 p2 */
#define FDET_STEM_VALU_K3_GENERIC 2  /* fp32 VALU, k3 s2 p1 (any H, W) */
#define FDET_STEM_VALU_K3_SCALAR 3   /* fp32 VALU, k3 s2 p1 weight gradient fed by scalar loads (H, W even, Wo % 4 == 0) */
#define FDET_STEM_MFMA 4             /* fp32 MFMA, k10 */
#define FDET_STEM_X3_SINGLE 5        /* bf16x3 k10, one LDS tile */
#define FDET_STEM_X3_PIPE 6          /* bf16x3 / precision16 k10, pipelined */
#define FDET_STEM_K3_MATRIX 7        /* bf16x3 / precision16 k3 weight gradient on the matrix cores */
#define FDET_STEM_K3_PS_FWD 8        /* k3 forward with a PS (column-strip) output */
int fdet_stem_last_route(int* out, int n);
int fdet_conv3x3_wgrad_ps_batched_p16(const void* const* h_x, const void* const* h_dz, float* const* h_dW,
                                      float* const* h_db, int L, int N, int C, int H, int W, void* ws,
                                      size_t ws_bytes, void* stream);
int fdet_block_chain_fwd_ps_p16(const void* x, int x_is_ps, const void* const* h_wpk1, const float* const* h_b1,
                                const void* const* h_wpk2, const float* const* h_b2, const float* const* h_scale,
                                void* const* h_a_ps, void* const* h_c_ps, void* const* h_out_ps, float* out_last,
                                int nblocks, int N, int F, int H, int W, float slope, void* stream);
int fdet_block_chain_bwd_ps_p16(const float* dout, const void* const* h_wpk1b, const void* const* h_wpk2b,
                                const float* const* h_scale, const void* const* h_a_ps, const void* const* h_c_ps,
                                void* const* h_dz1_ps, void* const* h_dz2_ps, float* dx, int nblocks, int N, int F,
                                int H, int W, float slope, void* stream);

/* precision16 on the fp32-I/O conv kernels (every channel count that is a multiple of 16; the pooled pair needs multiples
 * of 32 as its bf16x3 twin does): same arguments, panels (fdet_pack_conv3x3_weights_bf16x3), workspace sizes
 * (fdet_conv3x3_wgrad_bf16x3[_batched]_ws_bytes) and support predicates (fdet_conv3x3_pool_fusion_ok) as the _bf16x3 twins.
 * Contract:
 *   - every fp32 operand the kernel loads is rounded to bf16 (RNE, the hi part only); the panels' lo half is not read;
 *   - ONE v_mfma_f32_32x32x16_bf16 per (m, n) tile instead of three, fp32 accumulation;
 *   - epilogue arithmetic in fp32 (bias, LeakyReLU, dropout scale, skip add, max-pool, routing bytes, lrelu' mask, `add`);
 *   - every activation / activation gradient the kernel stores is rounded ONCE to bf16 (RNE) and stored in its fp32 word
 *     (y == bf16(y)); pooled maxima are taken on the fp32 values, so the routing bytes are those of the bf16x3 kernel
 *     on the same accumulators;
 *   - weight and bias gradients are fp32 sums of products of the bf16-rounded operands (bias: sum of bf16(dz)).
 * The F=64 pre-split precision16 path above has the same contract. */
int fdet_conv3x3_fwd_bf16(const float* x, const void* wpk, const float* bias, float* y_full,
                          const float* skip, const float* drop_scale, float* y_out, int N, int Cin,
                          int Cout, int H, int W, int pool, float slope, void* stream);
int fdet_conv3x3_dgrad_bf16(const float* dz, const void* wpk, const float* act, const float* add,
                            float* dx, int N, int Cin, int Cout, int H, int W, float slope, void* stream);
int fdet_conv3x3_fwd_pool_bf16(const float* x, const void* wpk, const float* bias, const float* skip,
                               const float* drop_scale, float* out_pooled, unsigned char* route, int N,
                               int Cin, int Cout, int H, int W, float slope, void* stream);
int fdet_conv3x3_dgrad_unpool_bf16(const float* dz, const void* wpk, const float* dout_pooled,
                                   const unsigned char* route, float* dx, int N, int Cin, int Cout,
                                   int H, int W, float slope, void* stream);
int fdet_conv3x3_wgrad_bf16(const float* x, const float* dz, float* dW, float* db, void* ws,
                            size_t ws_bytes, int N, int Cin, int Cout, int H, int W, void* stream);
int fdet_conv3x3_wgrad_bf16_batched(const float* const* h_x, const float* const* h_dz, float* const* h_dW,
                                    float* const* h_db, int L, void* ws, size_t ws_bytes, int N, int Cin,
                                    int Cout, int H, int W, void* stream);

/* MobileNetV3-small backbone, training pieces (round 4; models/MobilenetV3Backbone.py:49-60 trained through
 * models/ModelMeta.py:115-227): fp32 NCHW tensors [N][C][P = H*W].  The 1x1 convs use fdet_pointwise_*_bf16x3, the head
 * fdet_head_fwd / fdet_head_bwd.  PARITY UNPINNED (timm absent): checked against torch autograd on the CPU oracle.
 *   stem     : timm Conv2dSame(3,16,3,stride 2) without bias (TF "SAME" padding), output ceil(H/2) x ceil(W/2); weight gradient
 *   dw       : depthwise conv k = 3 | 5, stride 1 (pad k/2) or 2 (TF "SAME"), no bias; bwd = data + weight gradient
 *   bn       : nn.BatchNorm2d in TRAINING mode (batch statistics over N,H,W; running = (1-momentum)*running + momentum*batch
 *              with the unbiased variance) fused with the activation (0 none, 1 ReLU, 2 Hardswish) and an optional residual
 *              add; bwd takes dy = d/dy and returns dz, dgamma, dbeta.  ws: fdet_mbt_bn_ws_bytes(C)
 *   se       : timm SqueezeExcite y = x * hardsigmoid(W2 relu(W1 mean_hw(x) + b1) + b2); w1 [R,C], w2 [C,R];
 *              pooled [N,C], hidden [N,R], pre [N,C] are kept by the forward for the backward; bwd ws: (2*N*C + N*R) floats */
int fdet_mbt_stem_fwd(const float* x, const float* w, float* z, int N, int H, int W, void* stream);
size_t fdet_mbt_taps_ws_bytes(int C, int k);   /* workspace of the tap-gradient kernels; k = 0: the stem (C = 16, 27 taps) */
int fdet_mbt_stem_wgrad(const float* x, const float* dz, float* dW, void* ws, size_t ws_bytes, int N, int H, int W, void* stream);
int fdet_mbt_dw_fwd(const float* x, const float* w, float* z, int N, int C, int H, int W, int k, int s, void* stream);
int fdet_mbt_dw_bwd(const float* x, const float* dz, const float* w, float* dx, float* dW, void* ws, size_t ws_bytes, int N,
                    int C, int H, int W, int k, int s, void* stream);
size_t fdet_mbt_bn_ws_bytes(int C);
int fdet_mbt_bn_fwd(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, float* save_mean, float* save_invstd, const float* residual, float* y,
                    void* ws, size_t ws_bytes, int N, int C, int P, int act, void* stream);
int fdet_mbt_bn_bwd(const float* z, const float* dy, const float* gamma, const float* beta, const float* save_mean,
                    const float* save_invstd, float* dz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, int N,
                    int C, int P, int act, void* stream);
int fdet_mbt_se_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* pooled,
                    float* hidden, float* pre, float* y, int N, int C, int R, int P, void* stream);
int fdet_mbt_se_bwd(const float* x, const float* dy, const float* pooled, const float* hidden, const float* pre,
                    const float* w1, const float* w2, float* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws,
                    size_t ws_bytes, int N, int C, int R, int P, void* stream);

/* Training head fused with the loss (round 4): ONE launch sequence for what models/PoolResnet.py:100-102 +
 * losses/YoloLoss.py:4-44 (called per image and summed, models/ModelMeta.py:173-176) + their autograd compute:
 *   y = sigmoid(conv(x * drop_scale, w) + bias);  loss_per_image[n] = yolo_loss(y[n], gt[n]);  loss_sum = sum_n;
 *   dx = d loss_sum / d x (includes drop_scale),  dW [5,F,k,k],  db [5].
 * Equivalent to fdet_head_fwd + fdet_yolo_loss_fwd_bwd(grad_scale 1) + fdet_head_bwd; loss_per_image / loss_sum are
 * bit-identical to that sequence GIVEN y, y itself is computed in bf16x3 arithmetic (~1e-5 of the fp32 head).
 * Supported geometry (fdet_head_loss_fused_supported): F = 64, k = 6, pad = 0, maps of at most 15x15 (PoolResnet).
 * ws: fdet_head_loss_fused_ws_bytes() bytes, 16-byte aligned; its LAST 64 bytes are a ticket counter that must be
 * zero at the first call (the kernel leaves it zero); do not share ws between launches that may overlap. */
int fdet_head_loss_fused_supported(int F, int H, int W, int k, int pad);
size_t fdet_head_loss_fused_ws_bytes(int N, int F, int H, int W, int k, int pad);
int fdet_head_loss_fused(const float* x, const float* drop_scale, const float* w, const float* bias,
                         const float* gt, float* y, float* loss_per_image, float* loss_sum, float* dx,
                         float* dW, float* db, void* ws, size_t ws_bytes, int N, int F, int H, int W, int k,
                         int pad, void* stream);

/* Dropout2d scale factors: out[i] = (u_i >= p) ? 1/(1-p) : 0 with u from a counter-based
 * generator keyed by (seed, offset+i).  Replaces nn.Dropout2d's per-(n,c) Bernoulli draw
 * (models/PoolResnet.py:31,69).  The stream differs from ATen's Philox usage, so parity
 * tests inject masks instead. */
int fdet_dropout_scales(float* out, size_t n, float p, uint64_t seed, uint64_t offset, void* stream);

/* Dropout2d scales of every dropout layer of a model in one launch (nn.Dropout2d of models/PoolResnet.py:31,69,
 * models/SSD.py:47; per-rank streams of SURVEY.md 8e).  The counter is indexed by the GLOBAL image number:
 *   counter(image g, layer k, channel c) = base + g*LS + sum_{j<k} channels[j] + c,  LS = sum_k channels[k]
 * so that a data-parallel rank that owns images [first_image, first_image+n) draws exactly the planes a single
 * process draws for the concatenated batch.  channels / p: HOST arrays of nlayers (<= 32) entries.
 * out: layer k is a dense [n][channels[k]] array at float offset n * sum_{j<k} channels[j]. */
int fdet_dropout_scales_layers(float* out, int n, int nlayers, const int* channels, const float* p,
                               uint64_t seed, uint64_t base, uint64_t first_image, void* stream);

/* ---------------------------------------------------------------------------------------
 * On-device training augmentation (csrc/fdet_augment.hip).  Replaces the albumentations
 * pipelines of datasets/WIDERFace/datamodule.py:105-134 (training_transform /
 * default_transform) and the box rounding of dataset.py:81-91 on a ragged batch:
 *   bank    one device byte buffer of HWC uint8 RGB images
 *   table   [n_images] {offset (bytes, 64-bit), h, w}; h_table: the same rows in host memory
 *   params  [B] per-image records sampled on the host (fdet_amd/datasets/augment.py);
 *           h_params: the same records in host memory (validated before any launch)
 * Per-pixel draws (noise, glass offsets) come from a hash of (seed, params.key, tag, y, x).
 * ------------------------------------------------------------------------------------- */
typedef struct fdet_aug_image {
  int64_t offset;            /* byte offset of pixel (0,0) in the bank */
  int32_t h, w;
} fdet_aug_image;

#define FDET_AUG_FLIP 1            /* HorizontalFlip */
#define FDET_AUG_ROTATE 2          /* Rotate by angle (cos_a, sin_a), reflect-101 border */
#define FDET_AUG_BRIGHTNESS 4      /* v*alpha + beta */
#define FDET_AUG_NOISE 8           /* v + sigma*N(0,1) per pixel and channel */
#define FDET_AUG_GLASS 16          /* GlassBlur(sigma 0.1, max_delta 1, 1 iteration, fast mode) */
#define FDET_AUG_MOTION 32         /* MotionBlur with the motion_k x motion_k kernel motion_w */
#define FDET_AUG_CROP 64           /* informational: RandomResizedCrop drew the crop window */
#define FDET_AUG_CROP_FALLBACK 128 /* informational: ... by its centre-crop fallback */

typedef struct fdet_aug_params {
  int32_t image;                   /* row of the image table */
  int32_t flags;                   /* FDET_AUG_* */
  int32_t crop_x0, crop_y0, crop_w, crop_h;   /* crop window in source pixels (whole image when no crop) */
  float angle, cos_a, sin_a;       /* degrees, positive = counter-clockwise on screen */
  float alpha, beta;               /* contrast factor, brightness offset (0..255 units) */
  float sigma;                     /* noise standard deviation */
  uint32_t key;                    /* per-image key of the pixel hash */
  int32_t motion_k;                /* 1, 3, 5 or 7 */
  float motion_w[49];              /* row-major motion_k x motion_k weights (sum 1) */
  int32_t reserved;
} fdet_aug_params;                 /* 256 bytes */

/* Geometric chain + photometric ops -> uint8 intermediate mid [B,3,Ho,Wo] (one bilinear sample
 * of the source per pixel, one rounding). */
int fdet_aug_warp(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                  const fdet_aug_params* params, const fdet_aug_params* h_params, int B, int Ho, int Wo,
                  uint32_t seed, uint8_t* mid, void* stream);
/* GlassBlur + MotionBlur on mid -> out_u8 [B,3,Ho,Wo] and out_f32 = out_u8 / 255 (bit-identical to
 * fdet_u8_to_f32_norm).  Wo % 4 == 0 takes the vector stores (4-byte / 16-byte aligned outputs). */
int fdet_aug_finish(const uint8_t* mid, const fdet_aug_params* params, const fdet_aug_params* h_params, int B, int Ho,
                    int Wo, uint32_t seed, uint8_t* out_u8, float* out_f32, void* stream);
/* Box transform of the same chain.  boxes [total,5] rows [conf,x,y,w,h] in source pixels of the
 * bank's images, box_offset [n_images+1] (image i owns rows box_offset[i]..box_offset[i+1]-1).
 * Writes the surviving rows [1,x,y,w,h] (clipped area >= 10, rounded half-to-even) of the batch
 * compacted into rows [max_rows,5] and out_offset [B+1] (the layout of fdet_encode_targets);
 * rows past max_rows are counted in out_offset but not written. */
int fdet_aug_boxes(const float* boxes, const int32_t* box_offset, const fdet_aug_image* table,
                   const fdet_aug_image* h_table, int n_images, const fdet_aug_params* params,
                   const fdet_aug_params* h_params, int B, int Ho, int Wo, int max_rows, float* rows,
                   int32_t* out_offset, void* stream);

/* ---- dataset-level evaluation (csrc/fdet_eval.hip) ------------------------------------------------
 * PASCAL VOC / WIDER Face matching of one batch, accumulated (+=) into score-binned true/false-positive
 * histograms: the device-side state of a precision/recall curve and its AP over a whole validation set.
 * No counterpart in the reference (its only quality numbers are the per-batch step metrics above).
 *   pred [B,Kmax,5] rows [score,x,y,w,h] + pred_counts [B]: the output pair of fdet_reduce_bounding_boxes /
 *        fdet_ssd_reduce_bounding_boxes; rows need not be sorted
 *   gt_rows [gt_cap,5] rows [conf,x,y,w,h] + gt_offset [B+1]: the layout of fdet_encode_targets / fdet_aug_boxes
 *   iou_thresholds [T]: HOST array, 1 <= T <= FDET_EVAL_MAX_THRESHOLDS;  max_gt: largest box count of one image the
 *        launch reserves LDS for (<= FDET_EVAL_MAX_GT);  n_bins <= FDET_EVAL_MAX_BINS (1000: the WIDER protocol)
 *   tp, fp [T,n_bins] uint32, bin = min(n_bins-1, (int)floorf(score * n_bins)) in fp32; a negative score, -inf and
 *        NaN go to bin 0 (NaN is ordered as -inf: visited last), a score >= 1 and +inf to the last bin
 *   counters [FDET_EVAL_N_COUNTERS] uint64: ground-truth boxes, images, detections, rejected images
 *   match [B,Kmax] int32 or NULL: for iou_thresholds[0], the row of gt_rows a detection matched, else -1
 * Per image and threshold: detections in descending score (ties: ascending row); the candidate of a detection is
 * the box of highest IoU among ALL of the image's boxes (ties: lowest row; fp32 box_iou as in fdet_step_metrics on
 * x, y, x+w, y+h; a NaN IoU is never a candidate); true positive iff IoU >= threshold and the candidate has not been
 * claimed by an earlier detection, else false positive.
 * Sizes known on the host that exceed the limits return FDET_EINVAL.  Counts only the device knows (pred_counts[n] >
 * Kmax, more than max_gt boxes, offsets outside 0..gt_cap) reject that image as a whole: it adds nothing but
 * counters[FDET_EVAL_N_REJECTED] += 1, which the caller must read as an error; nothing is ever truncated. */
#define FDET_EVAL_MAX_THRESHOLDS 10
#define FDET_EVAL_MAX_DET 4864
#define FDET_EVAL_MAX_GT 4096
#define FDET_EVAL_MAX_BINS 4096
#define FDET_EVAL_N_GT 0
#define FDET_EVAL_N_IMAGES 1
#define FDET_EVAL_N_DET 2
#define FDET_EVAL_N_REJECTED 3
#define FDET_EVAL_N_COUNTERS 4
int fdet_eval_match(const float* pred, const int32_t* pred_counts, int B, int Kmax, const float* gt_rows,
                    const int32_t* gt_offset, int gt_cap, int max_gt, const float* iou_thresholds, int T,
                    int n_bins, uint32_t* tp, uint32_t* fp, uint64_t* counters, int32_t* match, void* stream);

/* ---- WIDER Face protocol evaluation (csrc/fdet_eval_wider.hip) ---------------------------------------
 * The matching rule of the WIDER Face evaluation protocol for one batch, for up to FDET_EVAL_WIDER_MAX_SUBSETS subsets
 * (Easy / Medium / Hard) in one pass, accumulated (+=) into per-(subset, score threshold) histograms.  It is not the VOC
 * rule of fdet_eval_match: boxes outside a subset are ignored, not missed; there is no uniqueness rule; overlaps use
 * inclusive pixel coordinates.  No counterpart in the reference.
 *   pred [B,Kmax,5] rows [score,x,y,w,h] + pred_counts [B]: as for fdet_eval_match
 *   pred_scale [B,2] (sx, sy) or NULL (= 1): detections are taken to source pixels as x*sx, y*sy, w*sx, h*sy, four
 *        separate fp32 multiplies, nothing rounded to integers
 *   gt_rows [gt_cap,5] + gt_offset [B+1]: ALL boxes of the images, source pixels, the layout of fdet_eval_match
 *   gt_subsets [gt_cap] uint32: bit s set = the box is kept in subset s (bits >= n_subsets are not read)
 *   score_norm: DEVICE [2] doubles (min, max - min) or NULL (= 0, 1); n = ((double)score - min) / (max - min)
 *   proposals, hits [n_subsets,n_bins] uint32
 *   counters [n_subsets + FDET_EVAL_WIDER_N_COUNTERS] uint64: kept boxes per subset, then images, detections,
 *        rejected images
 * Per image: detections in descending raw score (ties: ascending row; NaN last).  Everything below in fp64, fixed
 * operation order, no contraction: x1 = x, y1 = y, x2 = x + w, y2 = y + h for detections and boxes alike;
 * iw = min(x2) - max(x1) + 1, ih likewise (min(a,b) = a < b ? a : b, max(a,b) = a > b ? a : b, detection first);
 * overlap = iw*ih / (area_d + area_g - iw*ih) with area = (x2-x1+1)*(y2-y1+1) when iw > 0 and ih > 0, else 0.
 * The candidate of a detection is the box of highest overlap among ALL boxes (ties: lowest row; a NaN overlap is never
 * a candidate).  For subset s: overlap >= iou_threshold on a candidate that s does not keep drops the detection from s;
 * every other detection is a proposal; overlap >= iou_threshold on a kept candidate that no earlier detection has
 * recalled recalls it.  bin b = the smallest t in 0..n_bins-1 with n >= 1.0 - (double)(t+1)/n_bins (n < 0 and NaN:
 * counted nowhere); proposals[s][b] += 1 per proposal, hits[s][b] += 1 per recalled box at the bin of the detection
 * that recalled it first.  The sums over bins <= t are the protocol's proposal and recall counts at threshold t.
 * Limits and rejection: as fdet_eval_match (FDET_EVAL_MAX_DET, FDET_EVAL_MAX_GT, FDET_EVAL_MAX_BINS). */
#define FDET_EVAL_WIDER_MAX_SUBSETS 8
#define FDET_EVAL_WIDER_N_IMAGES 0
#define FDET_EVAL_WIDER_N_DET 1
#define FDET_EVAL_WIDER_N_REJECTED 2
#define FDET_EVAL_WIDER_N_COUNTERS 3
int fdet_eval_wider(const float* pred, const int32_t* pred_counts, int B, int Kmax, const float* pred_scale,
                    const float* gt_rows, const int32_t* gt_offset, int gt_cap, const uint32_t* gt_subsets,
                    int n_subsets, int max_gt, double iou_threshold, const double* score_norm, int n_bins,
                    uint32_t* proposals, uint32_t* hits, uint64_t* counters, void* stream);

/* ---- tiled full-resolution detection (csrc/fdet_tiles.hip) ------------------------------------------
 * Run the network on overlapping windows of a source image and merge the windows' boxes per image.  No counterpart
 * in the reference.  bank / table / h_table: as for the augmentation above.  tiles [T] / h_tiles: the windows in
 * device and host memory (fdet_amd.tiling.plan_tiles makes them); `image` is a row of the table. */
typedef struct fdet_tile {
  int32_t image, x0, y0, w, h;     /* window (x0, y0, w, h) in source pixels of table[image] */
} fdet_tile;                       /* 20 bytes */

/* Window t of the bank -> frames [T,3,Ho,Wo] planar uint8 (the frames forward_frames takes).  The sample is the one
 * fdet_aug_warp takes with flags = 0 and the window as its crop, byte for byte: sx = (u + 0.5) * (w / Wo) + x0 - 0.5
 * in fp64, two taps per axis clamped to the WINDOW, fp32 bilinear weights, one rint (half-to-even) + clamp; a window
 * of exactly Ho x Wo is a copy.  h_table / h_tiles are validated before the launch: a window outside its image, a
 * non-positive size or an image row outside the table returns FDET_EINVAL and nothing is written.  T <= 65535. */
int fdet_tile_gather(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                     const fdet_tile* tiles, const fdet_tile* h_tiles, int T, int Ho, int Wo, uint8_t* frames,
                     void* stream);

/* Cross-window merge, one workgroup per source image, no host synchronisation.
 *   rows [T,K,5] [score,x,y,w,h] in frame pixels + counts [T]: the reducers' output for the T frames
 *   tile_offset [n_images+1]: image n owns tiles tile_offset[n]..tile_offset[n+1]-1, whose `image` must be n;
 *        table [n_images]: only h and w are read
 *   1. x_s = rint(x0 + x * (w_win / Wo)), w_s = rint(w * (w_win / Wo)), likewise y / h: fp32, separate multiply and
 *      add, half-to-even
 *   2. edge_margin > 0: a detection is dropped when x < edge_margin at a window side with x0 > 0, when
 *      x + w > Wo - edge_margin at a side with x0 + w_win < image w, likewise y (frame pixels, fp32); sides that
 *      are sides of the image never drop anything; 0 turns the rule off
 *   3. greedy NMS over the image's union with the semantics of fdet_nms: stable descending score (ties: tile, then
 *      row; a NaN score is ordered as -inf), fp32 overlap on x_s, y_s, x_s + w_s, y_s + h_s compared in double with
 *      iou_threshold, a NaN overlap never suppresses
 *   out [n_images,Kout,5] [score,x_s,y_s,w_s,h_s] in visiting order, rows past the count zeroed; out_counts [n_images]
 * Limits: FDET_TILE_MAX_CANDIDATES candidates per image after step 2 and Kout survivors.  An image over either,
 * with counts[t] outside 0..K or with inconsistent tile_offset / tiles is rejected as a whole: out_counts = 0 and
 * rejected[0] += 1, which the caller must read as an error; nothing is ever truncated. */
#define FDET_TILE_MAX_CANDIDATES 4864
int fdet_tile_merge(const float* rows, const int32_t* counts, const fdet_tile* tiles, const int32_t* tile_offset,
                    int n_images, int T, int K, int Ho, int Wo, const fdet_aug_image* table, float edge_margin,
                    double iou_threshold, int Kout, float* out, int32_t* out_counts, uint64_t* rejected, void* stream);

/* Test-time augmentation for the two entries above: a mirrored second pass and box voting.
 *
 * fdet_tile_gather_flags: fdet_tile_gather plus flags [T] (device) / h_flags (host copy, validated with the windows).
 *   Bit 0 set: the frame is written mirrored left to right; output pixel (v, u) holds exactly what the unflagged
 *   frame holds at (v, Wo-1-u) (the same sample arithmetic on column Wo-1-u; one pass, the taps are read in reversed
 *   order, the stores keep their order).  An unflagged window gives fdet_tile_gather's bytes.  A flag byte with any
 *   other bit set returns FDET_EINVAL and nothing is written. */
int fdet_tile_gather_flags(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                           const fdet_tile* tiles, const fdet_tile* h_tiles, const uint8_t* flags, const uint8_t* h_flags,
                           int T, int Ho, int Wo, uint8_t* frames, void* stream);

/* fdet_tile_merge with un-mirroring and box voting.  Launch, limits and rejection are fdet_tile_merge's (one workgroup
 * per image, FDET_TILE_MAX_CANDIDATES candidates and Kout survivors, an image over either rejected as a whole).
 *   flags [T] device, NULL = all zero; out_votes [n_images,Kout] int32; min_votes >= 1; vote 0 | 1
 *   0. a row of a tile with flags bit 0 set: x <- ((float)Wo - x) - w, two fp32 subtractions in that order; y, w, h
 *      unchanged
 *   1., 2. as fdet_tile_merge, on the un-mirrored row
 *   3. the visiting loop of fdet_tile_merge (same order, same overlap test) with ownership: a live candidate i that is
 *      visited becomes a keeper and owns itself; every live j after it whose overlap with i exceeds iou_threshold dies
 *      and is owned by i, the first keeper that suppresses it, and by no other
 *   4. vote = 1: member weight q = llrint((double)min(score, 1.0f) * 1048576.0); q = 0 when the score is NaN or <= 0,
 *      or when any of the member's x1 = x_s, y1 = y_s, x2 = x_s + w_s, y2 = y_s + h_s (fp32) is not finite or exceeds
 *      2^24 in magnitude.  Per keeper, over its members, in int64: Q = sum q, sum q*x1, sum q*y1, sum q*x2, sum q*y2
 *      (the coordinates are integer-valued).  Q > 0: X1 = rint((double)sum q*x1 / (double)Q) (half to even), likewise
 *      Y1, X2, Y2; the row is [score of the keeper, X1, Y1, X2 - X1, Y2 - Y1] as fp32.  Q == 0 or vote = 0: the
 *      keeper's own [score, x_s, y_s, w_s, h_s].  votes = the number of members, the keeper included.  The sums are
 *      integers, so no order of addition changes a result.
 *   5. keepers with votes < min_votes are not written and do not count towards Kout (they still suppressed in 3);
 *      survivors in visiting order; rows of out and out_votes past the count are zeroed
 * With flags all zero, vote = 0 and min_votes = 1, out and out_counts are fdet_tile_merge's, byte for byte. */
int fdet_tile_merge_vote(const float* rows, const int32_t* counts, const fdet_tile* tiles, const uint8_t* flags,
                         const int32_t* tile_offset, int n_images, int T, int K, int Ho, int Wo,
                         const fdet_aug_image* table, float edge_margin, double iou_threshold, int min_votes, int vote,
                         int Kout, float* out, int32_t* out_votes, int32_t* out_counts, uint64_t* rejected, void* stream);

/* ---- rendering detections into a second bank (csrc/fdet_render.hip) ----------------------
 * dst image i = src image i with the first counts[i] rows of rows[i] rendered into it.  src / src_table / h_src_table
 * and dst / dst_table / h_dst_table: two banks as above, image i of the one and of the other of equal h and w.
 * rows [n_images,K,5] fp32 [score,x,y,w,h] in source pixels (NULL only with K = 0); counts [n_images] int32 on the
 * device, h_counts the same values in host memory; ws [n_images+1] int32 device scratch.  The source is never written.
 *   1. the destination image starts as a copy of the source image (device-to-device copies: one per run of images
 *      that follow each other in both banks)
 *   2. box -> pixels, fp32 then truncation toward zero: x0 = (int)x, y0 = (int)y, x1 = (int)(x + w), y1 = (int)(y + h),
 *      both ends inclusive.  A box is skipped when x, y, w or h is not finite, w < 1 or h < 1, or |x|, |y|, |x + w| or
 *      |y + h| exceeds 2^24, or when x1 == x0 or y1 == y0 (zero width or height in pixels: with w, h >= 1 only where
 *      the truncation folds a start in (-1, 0) and an end in [0, 1) onto pixel 0).  Rows at index >= counts[i] are
 *      never read.
 *   3. pixelate = 1: cell = max(1, ceil(max(x1-x0+1, y1-y0+1) / blocks)); cell (i, j) covers
 *      [x0+i*cell, x0+(i+1)*cell-1] n [x0, x1] n [0, W-1], likewise y; every pixel of a non-empty cell becomes
 *      (sum + cnt/2) / cnt per channel, in integers, over the cell's pixels of the SOURCE image; a pixel that several
 *      boxes cover takes the value of the box with the lowest row index
 *   4. outline = 1, after 3: t = (w <= 15 || h <= 15) ? 1 : 3 on the fp32 w and h (datasets/utils.py:198-201); a pixel
 *      inside the image takes (red, green, blue) when it lies in [x0,x1] x [y0,y1] and not in [x0+t,x1-t] x [y0+t,y1-t].
 *      This is the set of pixels PIL's ImageDraw.rectangle(outline=..., width=t) paints.
 * Validated on the host, FDET_EINVAL and nothing written: the byte ranges the two tables span overlap; h / w differ
 * between the tables; K < 0; blocks < 1; h_counts[i] outside 0..K; a flag that is not 0 | 1; a colour outside 0..255. */
int fdet_render_boxes(const uint8_t* src, const fdet_aug_image* src_table, const fdet_aug_image* h_src_table,
                      const float* rows, const int32_t* counts, const int32_t* h_counts, int n_images, int K, uint8_t* dst,
                      const fdet_aug_image* dst_table, const fdet_aug_image* h_dst_table, int outline, int pixelate,
                      int blocks, int red, int green, int blue, int32_t* ws, void* stream);

/* fdet_render_boxes plus Gaussian blur as PIL computes it: steps 1, 2 and 4 above unchanged, and
 *   3b. blur = 1.  PIL's ImageFilter.GaussianBlur is three box-blur passes along the rows and three along the columns
 *      (BoxBlur.c), each in 32-bit integer fixed point with a uint8 rounding of its own; the only float arithmetic is
 *      the derivation of three integers (r, ww, fw) per radius, done once on the host (render.blur_table).
 *      1. the pixel rectangle [x0,x1] x [y0,y1] and the skip rule are step 2's.  S = max(x1-x0+1, y1-y0+1) on the
 *         unclipped rectangle; the region R is the rectangle clipped to the image; an empty R does nothing
 *      2. the box's parameters are entry min(S, n_tab-1) of blur_tab [n_tab][3] int32 (r, ww, fw) on the device;
 *         h_blur_tab, the same values in host memory, is validated in 64 bits: r >= 0, ww >= 0, fw >= 0 and
 *         (2r+1)*ww + 2*fw <= 2^24.  With that bound 255 * weights + 2^23 < 2^32: the device arithmetic is plain
 *         unsigned 32-bit and nothing wraps.  The device does no float arithmetic for the blur.
 *      3. one pass along a line v[0..n-1] of one channel:
 *           out[i] = (ww * sum_{d=-r..r} v[c(i+d)] + fw * (v[c(i-r-1)] + v[c(i+r+1)]) + 2^23) >> 24,
 *         c(j) = clamp(j, 0, n-1): the edges of R are replicated and nothing outside R is read
 *      4. B = R's pixels of the SOURCE image taken through three passes along the rows of R, then three along its
 *         columns, each pass starting from the previous pass's uint8 output
 *      5. a pixel of R takes B's value unless a box of lower row index covers it (step 3's rule: the lowest index
 *         wins).  Every box reads the source, so no order of execution changes a byte
 *      6. the outline (step 4) comes after the blur
 *   For one box this is im.paste(im.crop((cx0, cy0, cx1+1, cy1+1)).filter(GaussianBlur(radius)), (cx0, cy0)) on the
 *   clipped box when the table holds PIL's parameters for that radius; for several, pasted in descending row index,
 *   each crop taken from the original image.
 * With blur = 0 dst holds fdet_render_boxes's bytes; blur_tab, h_blur_tab and rejected may then be NULL and ws needs
 * (n_images+1) int32.  With blur = 1: ws [ws_bytes] is device scratch of fdet_render_blur_ws_bytes(...) bytes for the
 * same h_src_table, h_counts and a host copy h_rows of rows ((n_images+1) int32, one int64 per box of h_counts, then
 * 3 bytes per pixel of every box's R; 0 for bad arguments).  Every offset into ws is computed on the device and
 * checked against ws_bytes: a box whose share does not fit (or whose R has a side above FDET_BLUR_MAX_LINE) is left
 * as the copy and counted in rejected[0] (uint64, device, += the number of such boxes), which the caller must read as
 * an error; nothing is written out of bounds.  The library allocates nothing.
 * Validated on the host, FDET_EINVAL and nothing written: everything fdet_render_boxes validates; blur not 0 | 1;
 * blur = 1 with pixelate = 1; with blur = 1 a NULL table or rejected, n_tab < 1, a table entry outside the bound of
 * 3b.2, an image with h or w above FDET_BLUR_MAX_LINE, ws_bytes below the (n_images+1) int32 + one int64 per box. */
#define FDET_BLUR_MAX_LINE 8192
size_t fdet_render_blur_ws_bytes(const fdet_aug_image* h_src_table, const float* h_rows, const int32_t* h_counts,
                                 int n_images, int K);
int fdet_render_boxes_blur(const uint8_t* src, const fdet_aug_image* src_table, const fdet_aug_image* h_src_table,
                           const float* rows, const int32_t* counts, const int32_t* h_counts, int n_images, int K,
                           uint8_t* dst, const fdet_aug_image* dst_table, const fdet_aug_image* h_dst_table, int outline,
                           int pixelate, int blur, int blocks, const int32_t* blur_tab, const int32_t* h_blur_tab,
                           int n_tab, int red, int green, int blue, void* ws, size_t ws_bytes, uint64_t* rejected,
                           void* stream);

/* ---- tracking faces across frame sequences (csrc/fdet_track.hip) --------------------------
 * Associates the detections of consecutive frames with a table of FDET_TRACK_SLOTS tracks per sequence: identity
 * (an id per track, never reused) and gap bridging (a track the detector misses is still emitted for emit_misses
 * frames).  No counterpart in the reference.  One workgroup per sequence walks its frames in order; no host
 * synchronisation.  Integer arithmetic throughout; the only floating-point operations are the fp32 sums of step 1 and
 * the one double multiply of step 3.
 *
 * State: per sequence one fdet_track_seq followed by FDET_TRACK_SLOTS fdet_track, in device memory; all-zero bytes are
 * a fresh state.  A slot is live when its id != 0; a free slot is all zero.  Corners are kept in 1/16 pixel. */
#define FDET_TRACK_SLOTS     128     /* live tracks per sequence */
#define FDET_TRACK_MAX_DETS  256     /* valid detections per frame */
#define FDET_TRACK_MAX_COORD 16384   /* |corner| bound, keeps every product below 2^62 */

typedef struct fdet_track {
  int32_t id, x1q, y1q, x2q, y2q, hits, misses, born;
  float score;
  /* reserved[0] = vx256, reserved[1] = vy256 under fdet_track_update_motion: the velocity of the box in 1/256 pixel per
   * frame, applied to all four corners alike; reserved[2] is unused.  fdet_track_update never reads the three words: it
   * carries those of a live track through unchanged and zeroes them when the slot is freed (step 6) and when a track is
   * born into it (step 7).  A state is driven by one of the two entries from fresh on. */
  int32_t reserved[3];
} fdet_track;                        /* 48 bytes */
typedef struct fdet_track_seq {
  int32_t next_id, frame, dropped, reserved;
} fdet_track_seq;                    /* 16 bytes, followed by FDET_TRACK_SLOTS fdet_track */

/* n_seq * (16 + 128 * 48) bytes; 0 for n_seq < 1. */
size_t fdet_track_state_bytes(int n_seq);

/* rows [T,K,5] fp32 [score,x,y,w,h] + counts [T] int32: what the reducers and TiledDetector.detect return, one row of
 * `rows` per frame.  seq_offset [n_seq+1] int32 (device) / h_seq_offset (the same values in host memory): sequence s
 * owns frames seq_offset[s]..seq_offset[s+1]-1 in time order.  state: fdet_track_state_bytes(n_seq) bytes, updated in
 * place.  Per frame t of a sequence, in order:
 *   1. valid detections.  Only the first counts[t] rows are read.  A row is valid when score, x, y, w, h are finite,
 *      every corner X1 = rint(x), Y1 = rint(y), X2 = rint(x + w), Y2 = rint(y + h) (fp32 sums, half to even, then
 *      converted to int) has |c| <= FDET_TRACK_MAX_COORD, and X2 - X1 >= 1 and Y2 - Y1 >= 1.  An invalid row takes
 *      no part in anything below and gets det_ids = 0.
 *   2. track box in pixels: P = (q + 8) >> 4 per corner (arithmetic shift: floor).
 *   3. overlap of a live track and a valid detection: iw = min(P.x2, X2) - max(P.x1, X1), ih likewise,
 *      inter = (iw > 0 && ih > 0) ? iw * ih : 0, uni = areaT + areaD - inter, all int64.  The pair is eligible when
 *      (double)inter > iou_threshold * (double)uni.
 *   4. greedy matching: until no eligible pair remains among unmatched tracks and unmatched detections, the pair with
 *      the largest IoU is matched; two IoUs compare exactly, as inter_a * uni_b against inter_b * uni_a in int64; ties
 *      go to the lower slot, then to the lower row index.
 *   5. matched track: q <- (alpha256 * 16 * D + (256 - alpha256) * q + 128) >> 8 per corner with D the detection's
 *      corner (int64, arithmetic shift); hits += 1; misses = 0; score = the detection's score.  alpha256 = 256 copies
 *      the detection.  x2q - x1q >= 16 and y2q - y1q >= 16 always hold, so P never degenerates.
 *   6. unmatched live track: misses += 1; when misses > max_misses the slot is freed (all zero).  Frees come before
 *      births: a freed slot can be taken in the same frame.
 *   7. births: the unmatched valid detections in row order; one gives birth when score >= birth_score (fp32).  It takes
 *      the lowest free slot: id = ++next_id, q = 16 * D, hits = 1, misses = 0, born = frame, score = its score.  With
 *      no free slot the detection is dropped and dropped += 1; that is not an error.
 *   8. det_ids [T,K] int32: det_ids[t][j] = the id row j was matched to or born as, else 0 (rows >= counts[t] too).
 *   9. emit, in slot order, every live track with hits >= min_hits and misses <= emit_misses:
 *      out_rows [T,128,5] fp32 [score, P.x1, P.y1, P.x2 - P.x1, P.y2 - P.y1], out_ids [T,128], out_misses [T,128],
 *      out_counts [T]; rows past out_counts[t] are zeroed.  Then frame += 1.
 * Rejection: a sequence with a counts[t] outside 0..K or a frame with more than FDET_TRACK_MAX_DETS valid rows is
 * rejected as a whole: its state stays as it was before the call, all its frames get out_counts = 0 and zeroed
 * out_rows / out_ids / out_misses / det_ids, and rejected[0] += 1, which the caller must read as an error.  Other
 * sequences are unaffected; nothing is ever truncated.
 * Validated on the host, FDET_EINVAL and nothing launched: h_seq_offset not monotone from 0 to T; n_seq < 1, T < 0 or
 * K < 0; alpha256 outside 1..256; max_misses < 0, min_hits < 1, emit_misses outside 0..max_misses; iou_threshold not
 * in [0, 1); a required pointer NULL (rows and det_ids are required when T * K > 0, counts and the out_* when T > 0). */
int fdet_track_update(const float* rows, const int32_t* counts, const int32_t* seq_offset, const int32_t* h_seq_offset,
                      int n_seq, int T, int K, double iou_threshold, int alpha256, int max_misses, int min_hits,
                      int emit_misses, float birth_score, void* state, float* out_rows, int32_t* out_ids,
                      int32_t* out_misses, int32_t* out_counts, int32_t* det_ids, uint64_t* rejected, void* stream);

/* fdet_track_update with a constant-velocity motion model: an integer alpha-beta filter on each track's centre velocity
 * (vx256, vy256 = reserved[0], reserved[1] of fdet_track) and an optional growth of the emitted box while a track coasts.
 * The same kernel source, launch shape, limits, rejection and host validation; the nine steps above with these changes
 * (int64, arithmetic shifts, M = FDET_TRACK_MAX_COORD):
 *   0.  predict, every live track, before step 2: per axis s = (v256 + 8) >> 4 (1/16 pixel); both corners of the axis move
 *       by s when the moved pixel corners (q + s + 8) >> 4 both stay within +-M, else the corners stay and the axis'
 *       velocity becomes 0.  Widths are kept, so the >= 16 invariants of step 5 hold.
 *   5'. matched track, before the blend of step 5, q the predicted corners and D the detection's pixel corners:
 *       rx = 16 * (D.x1 + D.x2) - (x1q + x2q) (twice the centre residual in 1/16 pixel),
 *       vx256 <- clamp(vx256 + ((beta256 * 8 * rx + 128) >> 8), -256 * max_speed, 256 * max_speed); y likewise.  Then step
 *       5 as it is, on the predicted q.
 *   6'. unmatched track that survives step 6: v256 <- (v256 * damp256 + 128) >> 8 per axis.
 *   9'. a track emitted with misses = m > 0: gx = min((grow256 * m * (P.x2 - P.x1) + 256) >> 9, M), gy from the height, and
 *       the row is [score, P.x1 - gx, P.y1 - gy, P.x2 - P.x1 + 2 gx, P.y2 - P.y1 + 2 gy]; every value stays below 2^17 in
 *       magnitude, exact in fp32.  Matching (steps 3, 4) uses the un-grown box and the state is never grown.
 * A freed slot is all zero and a track is born with velocity 0, as above.  A rejected sequence leaves its state untouched,
 * the velocities included.  With beta256 = 0 and grow256 = 0 outputs and state equal fdet_track_update's byte for byte
 * from a fresh state; with alpha256 = beta256 = 256 a box moving by whole pixels per frame, |v| <= max_speed, is predicted
 * exactly from its third frame on.
 * Validated on the host as fdet_track_update, and: beta256, damp256, grow256 outside 0..256, max_speed outside 0..1024
 * (pixels per frame) give FDET_EINVAL with nothing launched. */
int fdet_track_update_motion(const float* rows, const int32_t* counts, const int32_t* seq_offset, const int32_t* h_seq_offset,
                             int n_seq, int T, int K, double iou_threshold, int alpha256, int max_misses, int min_hits,
                             int emit_misses, float birth_score, int beta256, int damp256, int max_speed, int grow256,
                             void* state, float* out_rows, int32_t* out_ids, int32_t* out_misses, int32_t* out_counts,
                             int32_t* det_ids, uint64_t* rejected, void* stream);

/* Offline refinement of the tracker's output (csrc/fdet_track_refine.hip): a second pass over WHOLE
 * sequences that back-fills a track before its first detection, interpolates the gaps between its detections, stitches
 * the fragments of one face into one id and drops short chains.  One workgroup per sequence, no host synchronisation;
 * no counterpart in the reference.  Integer arithmetic (int64, arithmetic shifts, floor division) apart from step 1 of
 * fdet_track_update on an anchor's row and the one double multiply of the stitching threshold.
 *
 * det_rows [T,K,5] are the rows that were given to fdet_track_update(_motion) (only rows with det_ids > 0 are read),
 * det_ids [T,K] what it returned for them (values <= 0: no id), trk_rows [T,128,5] / trk_ids / trk_misses [T,128] /
 * trk_counts [T] its out_rows / out_ids / out_misses / out_counts.  seq_offset / h_seq_offset as there; every sequence's
 * frames are ALL its frames in time order (cutting a video into calls is the caller's business).
 * Outputs: out_rows [T,256,5] fp32 [score,x,y,w,h], out_ids / out_misses / out_kind [T,256], out_counts [T]; rows past
 * out_counts[t] are zeroed.  out_kind: 0 = detected, 1 = coasted by the online tracker, 2 = interpolated, 3 = back-filled.
 * Per sequence:
 *   1. anchors.  Track id i has an anchor at frame t when (a) it was emitted at t with trk_misses == 0: the box is the
 *      emitted row's, or (b) it was not emitted at t at all and a row j has det_ids[t][j] == i (the detections before
 *      the min_hits-th): the box is that row's.  Either box is the row's corners by step 1 of fdet_track_update (the
 *      identity on an emitted row, whose values are integers), the score is the row's score.  An emitted row with
 *      trk_misses != 0 is a coasted row.  An id that has coasted rows but no anchor in the sequence passes through
 *      untouched: its rows keep kind 1 under its own id, and none of the steps 2..5 concern it.
 *   2. stitch (skipped when stitch_gap < 0).  Chains are built from the tracks with anchors in ascending id.  A chain is
 *      named by its lowest id and remembers the frame L and the box A of its last anchor.  Track j with first anchor
 *      (f, F) may join a chain with L < f, f - L - 1 <= stitch_gap and (double)inter > stitch_iou * (double)uni, inter
 *      and uni by step 3 of fdet_track_update on A and F.  Among those it joins the one with the largest IoU (compared
 *      exactly by cross-multiplication as in step 4), the lowest chain id on a tie.  Every row and anchor of j takes the
 *      chain's id, and (L, A) become j's last anchor.  A track that joins nothing starts a chain.
 *   3. length filter.  A chain with fewer than min_length anchors disappears from every frame, coasted rows included.
 *   4. interpolate.  For consecutive anchors (a, A), (b, B) of a chain with b - a >= 2, every frame a < t < b gets, per
 *      corner c, A.c + floor((2 * (B.c - A.c) * (t - a) + (b - a)) / (2 * (b - a))) (round half up), score = A's
 *      score, misses = t - a, kind 2.
 *   5. back-fill.  For a chain's first anchor (f, F), every frame t of the sequence with f - lookback <= t < f gets F
 *      grown by step 9' of fdet_track_update_motion with m = f - t and grow256; score = F's score, misses = m, kind 3.
 *   6. per frame and chain at most one row.  An anchor (kind 0: the row it came from, copied as it is, misses 0) wins
 *      over an interpolated row, that over a coasted row of the input (copied as it is, with its misses; of several
 *      member tracks coasting in one frame, the one with the highest id), and a back-filled row comes last.
 *   7. order and room.  Rows of kinds 0..2 in ascending chain id, then rows of kind 3 in ascending chain id; the first
 *      FDET_TRACK_REFINE_ROWS are written and rejected[1] += the number that did not fit, which is not an error.
 * Rejection: a sequence with a trk_counts[t] outside 0..128, an emitted id <= 0, ids spanning more than
 * FDET_TRACK_REFINE_MAX_IDS (highest - lowest + 1, emitted ids and det_ids > 0 alike), an anchor whose row is not valid
 * by step 1, or more than FDET_TRACK_SLOTS anchors in one frame (neither is something fdet_track_update produces) is
 * rejected as a whole: its frames get zeroed outputs and rejected[0] += 1; other sequences are unaffected.  An id
 * occurring twice in one frame is malformed as well: which occurrence counts is unspecified, but nothing is read or
 * written out of bounds.
 * ws: fdet_track_refine_ws_bytes(n_seq, T) bytes of device memory (T * 4100; 0 when nothing is launched), 4-byte aligned.
 * Validated on the host, FDET_EINVAL and nothing launched: h_seq_offset not monotone from 0 to T; n_seq < 1, K < 0, T < 0
 * or T > 2^24; lookback outside 0..1024; grow256 outside 0..256; stitch_gap > 65535; stitch_iou not in [0, 1);
 * min_length < 1; ws_bytes too small; a required pointer NULL (det_rows and det_ids when T * K > 0, seq_offset,
 * h_seq_offset and rejected always, the rest when T > 0). */
#define FDET_TRACK_REFINE_ROWS     256    /* rows per refined frame */
#define FDET_TRACK_REFINE_MAX_IDS  4096   /* span of ids (highest - lowest + 1) in one sequence of one call */
size_t fdet_track_refine_ws_bytes(int n_seq, int T);
int fdet_track_refine(const float* det_rows, const int32_t* det_ids, int K, const float* trk_rows, const int32_t* trk_ids,
                      const int32_t* trk_misses, const int32_t* trk_counts, const int32_t* seq_offset,
                      const int32_t* h_seq_offset, int n_seq, int T, int lookback, int grow256, int stitch_gap,
                      double stitch_iou, int min_length, float* out_rows, int32_t* out_ids, int32_t* out_misses,
                      int32_t* out_kind, int32_t* out_counts, void* ws, size_t ws_bytes, uint64_t* rejected, void* stream);

/* ---- face chips and the sharpest chip of each track (csrc/fdet_chips.hip) ------------------
 * fdet_chip_extract cuts one fixed-size square crop ("chip") per detection row out of the image bank;
 * fdet_chip_best_update keeps, per track id, the sharpest chip seen so far.  No counterpart in the reference.  Integer
 * arithmetic throughout; the only floating-point operations are the fp32 sums and roundings of step 1. */
#define FDET_CHIP_MIN_SIZE 8
#define FDET_CHIP_MAX_SIZE 256
#define FDET_CHIP_MAX_SIDE 8192      /* source window side; bounds the work per chip (S*S taps) */
#define FDET_CHIP_MAX_CHIPS (1 << 20)

typedef struct fdet_chip_info {
  int32_t image, row;        /* rows[image][row] */
  int32_t wx0, wy0, S;       /* source window [wx0, wx0+S) x [wy0, wy0+S) in pixels of table[image] */
  int32_t inside256;         /* floor(256 * window pixels inside the image / S^2) */
  int32_t flags;             /* bit 0: valid */
  int32_t reserved;
  int64_t sharp;
} fdet_chip_info;            /* 40 bytes */

/* bank / table / h_table: an image bank as above.  rows [n_images,K,5] fp32 [score,x,y,w,h] in source pixels (NULL only
 * with K = 0) and counts [n_images] int32 on the device: what the reducers, TiledDetector.detect and the tracker return;
 * h_counts: the same values in host memory.  chip_offset [n_images+1] int32 (device) / h_chip_offset (host): the
 * exclusive prefix sum of h_counts.  Chip chip_offset[i] + j belongs to row j of image i; M = h_chip_offset[n_images].
 * chips: [M,C,C,3] uint8 (planar = 0, the bank's HWC layout) or [M,3,C,C] (planar = 1); info [M].  Per chip:
 *   1. corners as step 1 of fdet_track_update: X1 = rint(x), Y1 = rint(y), X2 = rint(x + w), Y2 = rint(y + h) (fp32 sums,
 *      half to even).  The row is valid when score, x, y, w, h are finite, every |corner| <= 16384, X2 - X1 >= 1 and
 *      Y2 - Y1 >= 1, the box meets the image (X2 > 0, X1 < W, Y2 > 0, Y1 < H) and the S of step 2 is <=
 *      FDET_CHIP_MAX_SIDE.  An invalid row gives an all-zero chip and an info of zeros except image and row; that is
 *      not an error.
 *   2. square window with margin: side = max(X2 - X1, Y2 - Y1); m = (side * margin256 + 128) >> 8; S = side + 2 * m;
 *      wx0 = (X1 + X2 - S) >> 1, wy0 = (Y1 + Y2 - S) >> 1 (arithmetic shift: floor).
 *   3. per-axis taps of chip column u of C (rows alike): pairs (window index i in 0..S-1, integer weight) whose weights
 *      sum to D.  S >= C, exact area averaging, D = S: every i with w = min((i+1)*C, (u+1)*S) - max(i*C, u*S) > 0, weight
 *      w (S == C: one tap, a copy).  S < C, bilinear in integers, D = 2*C: t = (2*u + 1)*S - C, i0 = floor(t / (2*C))
 *      (may be -1), f = t - i0*2*C; the taps are (i0, 2*C - f) and (i0 + 1, f), indices clamped to 0..S-1.
 *   4. window index i reads image column clamp(wx0 + i, 0, W-1), rows alike (edge replication).  Per channel
 *      value = (sum_y sum_x wy*wx*p + D*D/2) / (D*D) in int64, integer division; D*D*255 < 2^35.
 *   5. inside = max(0, min(wx0+S, W) - max(wx0, 0)) * (the same in y); inside256 = (inside * 256) / (S*S) in int64.
 *   6. sharpness of the chip as written: L = (77*R + 150*G + 29*B + 128) >> 8;
 *      sharp = sum over 1 <= v,u <= C-2 of (4*L(v,u) - L(v-1,u) - L(v+1,u) - L(v,u-1) - L(v,u+1))^2 in int64
 *      (at C = 256 at most 254^2 * 1020^2 = 67 122 446 400 < 2^40).
 * Validated on the host, FDET_EINVAL and nothing written: C outside 8..256; margin256 outside 0..256; planar not 0 | 1;
 * K < 0; n_images < 1; an h_counts[i] outside 0..K; h_chip_offset not the prefix sum of h_counts; M >
 * FDET_CHIP_MAX_CHIPS; a table row of non-positive size; a required pointer NULL (chips and info are required when
 * M > 0).  M = 0 is success with no launch. */
int fdet_chip_extract(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                      const float* rows, const int32_t* counts, const int32_t* h_counts,
                      const int32_t* chip_offset, const int32_t* h_chip_offset, int K, int C, int margin256,
                      int planar, uint8_t* chips, fdet_chip_info* info, void* stream);

/* The best-shot gallery: n_seq * G entries in device memory, carried from call to call like the tracker state; all-zero
 * bytes are an empty gallery.  Entry k - 1 of sequence s belongs to track id k (the tracker's ids are dense from 1 per
 * sequence and never reused). */
typedef struct fdet_chip_best {
  int32_t id;                /* 0 = empty */
  int32_t frame, image_wx0, image_wy0, S, inside256, seen, reserved;
  int64_t sharp;
} fdet_chip_best;            /* 40 bytes */

/* n_seq * G * 40; 0 for bad arguments. */
size_t fdet_chip_gallery_bytes(int n_seq, int G);

/* chips / info [M]: what fdet_chip_extract wrote (either layout: a chip is C*C*3 bytes).  ids [n_images,K] int32,
 * row-aligned with the rows the chips were cut from: the id of chip i is ids[info[i].image * K + info[i].row].
 * seq_offset [n_seq+1] int32 (device) / h_seq_offset (host): frame t = info[i].image belongs to the sequence s with
 * seq_offset[s] <= t < seq_offset[s+1]; the recorded frame number is frame_base[s] + t - seq_offset[s] (frame_base
 * [n_seq] int32, device).  gallery: fdet_chip_gallery_bytes(n_seq, G) bytes; gallery_chips [n_seq,G,C*C*3] uint8;
 * scratch [n_seq*G] uint64 (cleared by the call); overflow [1] uint64 counter.
 *   1. a chip is a candidate when it is valid, id >= 1, S >= min_side and inside256 >= min_inside256 (and its sharp lies
 *      in 0..2^40-1, which fdet_chip_extract guarantees).  A candidate with id > G adds one to overflow[0] and takes no
 *      further part; that is not an error.
 *   2. among the candidates of one (sequence, id) in this call the winner has the largest sharp; ties go to the lowest
 *      chip index.
 *   3. the winner replaces the entry when the entry is empty or when sharp > entry.sharp, strictly: id, frame,
 *      image_wx0 = wx0, image_wy0 = wy0, S, inside256 and sharp are set and the chip's C*C*3 bytes are copied.
 *   4. seen += the number of candidates of that id in this call, whether or not the winner replaced anything.
 * Ties and strictness make the result independent of how a sequence is cut into calls.
 * Validated on the host, FDET_EINVAL and nothing written: G < 1; M outside 0..FDET_CHIP_MAX_CHIPS; C outside 8..256;
 * h_seq_offset not monotone from 0; n_seq < 1; K < 0; min_side < 0; min_inside256 outside 0..256; a required pointer
 * NULL (chips, info and ids are required when M > 0).  M = 0 is success with no launch. */
int fdet_chip_best_update(const uint8_t* chips, const fdet_chip_info* info, int M, int C, const int32_t* ids, int K,
                          const int32_t* seq_offset, const int32_t* h_seq_offset, int n_seq, const int32_t* frame_base,
                          int G, int min_side, int min_inside256, void* gallery, uint8_t* gallery_chips,
                          uint64_t* scratch, uint64_t* overflow, void* stream);

/* Depthwise-separable residual block (models/SeparableCNN.py:40-51; none of its three convs has a bias):
 *   a = lrelu(W1 x)   b = lrelu(dw3x3(a), pad 1)   c = W2 b   e = c * drop_scale[n,c] + x   out = maxpool2x2(e) | e
 * fdet_sepblock_fwd runs the whole block in ONE kernel on fp32 NCHW tensors: both 1x1 convs as bf16x3 GEMMs on the matrix
 * cores, the depthwise conv and both LeakyReLUs in LDS between them (csrc/fdet_sepblock.hip).
 *   x [N,F,H,W]; w1_pk / w2_pk: FORWARD panels of fdet_pack_pointwise_weights_bf16x3 (Cout = Cin = F); wd [F,1,3,3];
 *   drop_scale [N,F] or NULL (eval); pool 1 | 2 (2: even H and W); out [N,F,H/pool,W/pool]
 *   training: a_save, b_save [N,F,H,W] (both or neither) receive a and b; route [N,F,H/2,W/2] uint8 (pooled training
 *   passes; else NULL) receives bits 4-5 = index of the window's maximum in scan order (first maximum wins, NaN is a
 *   maximum) with bits 0-3 set, which makes fdet_pool_route_bwd return unpool(dout) * drop_scale for this block.
 * Supported: F % 8 == 0, 8 <= F <= 128, any map that has a tiling within the LDS (fdet_sepblock_plan returns 1 and writes
 * {rows, columns of a tile, bands, column segments, LDS bytes, haloed positions per tile} to out[0..n-1]; launches
 * nothing).  Everything else returns FDET_EINVAL and computes nothing.
 * Backward is composed from fdet_pointwise_{dgrad,wgrad}_bf16x3, fdet_mbt_dw_bwd, fdet_pool_route_bwd and
 *   fdet_sepblock_gate_bwd: out[n,f,p] = g[n,f,p] * drop_scale[n,f] * lrelu'(act[n,f,p])   (act / drop_scale may be NULL:
 *   factor 1; lrelu' = 1 where act > 0 else slope: act is the POST-activation value, whose sign is the pre-activation's;
 *   out may alias g).
 * fdet_sepblock_lrelu: y = lrelu(z) over n floats (the composed forward's activation after the depthwise conv). */
int fdet_sepblock_plan(int F, int H, int W, int pool, int* out, int n);
int fdet_sepblock_fwd(const float* x, const void* w1_pk, const float* wd, const void* w2_pk, const float* drop_scale,
                      float* out, float* a_save, float* b_save, unsigned char* route, int N, int F, int H, int W,
                      int pool, float slope, void* stream);
int fdet_sepblock_gate_bwd(const float* g, const float* act, const float* drop_scale, float* out, int N, int F, int P,
                           float slope, void* stream);
int fdet_sepblock_lrelu(const float* z, float* y, size_t n, float slope, void* stream);

/* ---- baseline JPEG decode into the device image bank (csrc/fdet_jpeg.hip) ----------------------------
 * The hybrid split of GPU JPEG decoders: the host does the serial work (marker parsing, Huffman decoding), the device
 * the arithmetic (dequantisation, 8x8 inverse DCT, chroma upsampling, colour conversion) and writes HWC uint8 RGB
 * straight into the bank.  Every device step is integer arithmetic in libjpeg, so the result is byte-identical to
 * libjpeg-turbo's default decode (accurate-integer "islow" IDCT, "fancy" upsampling, 16-bit fixed-point YCbCr -> RGB), which
 * is what PIL's Image.open(...).convert("RGB") returns.  Replaces the PIL decode behind datasets/WIDERFace/annotations.py
 * bank_from_files (the reference decodes with cv2.imread in DataLoader workers, datasets/WIDERFace/dataset.py).
 *
 * Supported: 8-bit baseline sequential DCT (SOF0; SOF1 with 8-bit samples), Huffman coding, ONE interleaved scan; 1 component
 * (grey: R = G = B) or 3 components YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; 8- or 16-bit DQT entries;
 * optional DRI; APPn / COM skipped.  Everything else that is a well-formed JPEG (progressive, arithmetic, lossless, 12-bit,
 * CMYK / 4 components, an Adobe APP14 segment declaring RGB or components named R G B, multi-scan baseline, other sampling
 * ratios) returns FDET_JPEG_UNSUPPORTED so that a caller can fall back to another decoder; a truncated or corrupt stream
 * returns FDET_JPEG_ECORRUPT.
 *
 * The two host functions are plain C++ without a HIP call or mutable global state: any number of threads may call them at
 * once.  `bytes` is HOST memory here, as are `out` and `coef`. */
#define FDET_JPEG_UNSUPPORTED (-4) /* a JPEG outside the supported subset (fall back to another decoder) */
#define FDET_JPEG_ECORRUPT (-5)    /* not a JPEG, truncated or corrupt */

typedef struct fdet_jpeg_info_t {
  int32_t width, height, ncomp;    /* ncomp 1 | 3 */
  int32_t restart_interval;        /* MCUs between RSTn markers, 0 = none */
  int32_t hs[3], vs[3];            /* sampling factors per component (a single component is reported as 1x1) */
  int32_t blocks_w[3], blocks_h[3];/* 8x8 block grid per component INCLUDING the padding blocks of the last MCUs */
  int32_t mcus_x, mcus_y;
  int64_t coef_count;              /* int16 coefficients of the image = 64 * sum of blocks_w * blocks_h */
  uint16_t qt[3][64];              /* dequantisation table per component, natural (row-major) order */
} fdet_jpeg_info_t;                /* 464 bytes */

/* Parse the markers up to the first SOS.  Nothing of `out` is meaningful unless 0 is returned. */
int fdet_jpeg_info(const uint8_t* bytes, size_t n, fdet_jpeg_info_t* out);

/* Huffman-decode the scan (DC prediction, byte stuffing, restart markers) into quantised coefficients in natural,
 * de-zigzagged order: component c is one [blocks_h[c]][blocks_w[c]][64] int16 plane, planes in component order, padding
 * blocks included (they are coded in the stream).  capacity = int16 elements at `coef`; fewer than coef_count returns
 * FDET_EWORKSPACE.  No read goes past bytes + n and no write past coef + capacity, whatever the stream holds. */
int fdet_jpeg_entropy_decode(const uint8_t* bytes, size_t n, int16_t* coef, size_t capacity);

/* One image of a reconstruct call.  Offsets are the caller's choice (the planes of different images must not overlap). */
typedef struct fdet_jpeg_desc {
  int64_t bank_offset;             /* byte offset of pixel (0,0) in the bank; the image takes height * width * 3 bytes */
  int64_t coef_offset[3];          /* first int16 of component c's plane in `coef` (multiple of 8: 16-byte loads) */
  int64_t plane_offset[3];         /* first byte of component c's sample plane [blocks_h*8][blocks_w*8] in the workspace
                                      (multiple of 8) */
  int32_t width, height, ncomp;
  int32_t hs, vs;                  /* luma sampling 1x1 | 2x1 | 2x2 (chroma is 1x1); 1x1 for ncomp = 1 */
  int32_t blocks_w[3], blocks_h[3];
  int32_t reserved;
  uint16_t qt[3][64];
} fdet_jpeg_desc;                  /* 488 bytes */

/* coef (DEVICE, coef_count int16) -> RGB in the bank, two kernels on `stream`:
 *   1. dequantise + libjpeg's jpeg_idct_islow (13-bit constants, 2 pass-1 bits), level shift and range limit through the
 *      masked limit table (index & 1023: 0..127 -> +128, 128..511 -> 255, 512..895 -> 0, 896..1023 -> -896), one wave per eight
 *      blocks, into the uint8 sample planes of `workspace`.  32-bit arithmetic: exact whenever the dequantised
 *      coefficients fit in 16 bits, which is also the domain of libjpeg-turbo's SIMD IDCT
 *   2. chroma upsampling + colour conversion + crop to width x height.  A chroma plane of downsampled width dw =
 *      ceil(width / hs) > 2 takes the "fancy" triangle filter: 2x1 out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] =
 *      (3 in[i] + in[i+1] + 2) >> 2; 2x2 the same on column sums 3 * near row + far row with (… + 8) >> 4 and (… + 7) >> 4;
 *      columns clamp to 0..dw-1 and the far row to 0..ceil(height / vs)-1 (edge replication; padding samples are read
 *      only where they lie inside those bounds).  dw <= 2 replicates, as the library does.  R = Y + ((91881 Cr' + 32768) >> 16),
 *      G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16), clamped, with Cb' = Cb - 128.
 * descs (DEVICE) / h_descs (HOST copy, validated before anything is enqueued): blocks that do not cover the image,
 * sampling outside the supported set, a misaligned offset or a plane / coefficient / bank range outside the given sizes
 * return FDET_EINVAL.  bank must be 16-byte aligned.  n_images <= 65535. */
int fdet_jpeg_reconstruct(const int16_t* coef, size_t coef_count, const fdet_jpeg_desc* descs, const fdet_jpeg_desc* h_descs,
                          int n_images, uint8_t* workspace, size_t workspace_bytes, uint8_t* bank, size_t bank_bytes,
                          void* stream);

/* ---- baseline JPEG encode out of the device image bank (csrc/fdet_jpeg_enc.hip) ------------
 * The mirror image of the decoder, with the entropy coder on the device as well: only the compressed scan crosses to the
 * host.  For an RGB image, quality 1..100 and subsampling 4:4:4 | 4:2:2 | 4:2:0 the file (header + byte-stuffed scan + EOI)
 * equals, byte for byte, what PIL's Image.save(f, "JPEG", quality=q, subsampling=s) writes with libjpeg-turbo at its
 * defaults (no optimize, no progressive, no restart markers, no EXIF / ICC / DPI).  The reference writes its annotated
 * images with cv2.imwrite on the host (detect_images.py); tests/jpeg_enc_cpu_ref.py restates every rule below in numpy.
 *
 * Two phases, so that every buffer is sized exactly before anything is written into it:
 *   plan   colour conversion, edge padding, downsampling, forward DCT, quantisation -> int16 coefficients; the exact bit
 *          length of every block; a per-image exclusive scan -> every block's bit offset and every image's total
 *   emit   (after the host has read the totals and sized the scan buffer) every block writes its bits at its offset
 * Byte stuffing (FF -> FF 00) is left to the host, which does it while it assembles the file.
 *
 * Blocks are numbered in scan order per image: MCU by MCU, row-major; inside an MCU the hs * vs luma blocks row-major, then
 * Cb, then Cr.  An image has mcus_x * mcus_y * (hs * vs + 2) blocks, the dummy blocks the MCU grid adds included. */
#define FDET_JPEG_SUB_444 0        /* luma 1x1: PIL subsampling=0 */
#define FDET_JPEG_SUB_422 1        /* luma 2x1: PIL subsampling=1 */
#define FDET_JPEG_SUB_420 2        /* luma 2x2: PIL subsampling=2 */
#define FDET_JPEG_ENC_MAX_BLOCK_BITS (11 + 16 + 63 * (16 + 10)) /* DC code + bits, 63 x (AC code + bits): no block is longer */
#define FDET_JPEG_ENC_MAX_BLOCKS (1 << 20)  /* per image: its bit total stays below 2^31 */
#define FDET_JPEG_ENC_HEADER_BYTES 623      /* SOI .. SOS of every file this encoder writes */

/* HOST only, no HIP call, no mutable global.  out[0..63] luminance, out[64..127] chrominance table of `quality` (1..100) in
 * natural (row-major) order: clamp((base * scale + 50) / 100, 1, 255) of the Annex K tables with scale = 5000 / quality
 * below 50 and 200 - 2 * quality from 50 on. */
int fdet_jpeg_quant_tables(int quality, uint16_t* out);

/* HOST only.  SOI, APP0 (JFIF 1.01, density 1x1), DQT 0, DQT 1 (zigzag order), SOF0, DHT DC0 AC0 DC1 AC1 (the Annex K
 * typical tables), SOS: everything in front of the scan, FDET_JPEG_ENC_HEADER_BYTES bytes.  *n receives that count;
 * FDET_EWORKSPACE (and *n set) when capacity is smaller.  width, height 1..65535. */
int fdet_jpeg_write_header(int width, int height, int quality, int subsampling, uint8_t* out, size_t capacity, size_t* n);

/* One image of an encode call. */
typedef struct fdet_jpeg_enc_desc {
  int64_t bank_offset;             /* byte offset of pixel (0,0) in the bank, any alignment; height * width * 3 bytes */
  int64_t block_base;              /* the image's first block in the workspace's arrays; images follow each other densely,
                                      in call order: block_base[0] = 0, block_base[i + 1] = block_base[i] + n_blocks[i] */
  int64_t scan_offset;             /* emit only: first byte of the image's stream in the scan buffer (multiple of 4) */
  int32_t width, height;
  int32_t mcus_x, mcus_y;          /* ceil(width / (8 hs)), ceil(height / (8 vs)) */
  int32_t n_blocks;                /* mcus_x * mcus_y * (hs * vs + 2) <= FDET_JPEG_ENC_MAX_BLOCKS */
  int32_t reserved;
} fdet_jpeg_enc_desc;              /* 48 bytes */

/* Workspace of a plan over total_blocks blocks of n_images images, in bytes; 0 for a bad count.  Layout, B = total_blocks:
 *   int16  coef[B][64]   quantised coefficients in ZIGZAG order        at byte 0
 *   uint32 bits[B]       bit length of the block's code                at byte 128 B
 *   uint32 start[B]      bit offset of the block in its image's stream at byte 132 B
 *   uint32 total[n]      bits of image i's stream, before padding      at byte 136 B */
size_t fdet_jpeg_enc_ws_bytes(int64_t total_blocks, int n_images);

/* Phase 1, three kernels on `stream`; bank is read only.  Per block of 8x8 samples:
 *   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   padding  a sample column past the image reads the last column; a row past it the last row, except that a 4:2:0
 *            chroma row past ceil(height / 2) - 1 repeats THAT downsampled row (libjpeg pads after downsampling)
 *   chroma   4:2:0 (a + b + c + d + 1 + (x & 1)) >> 2, 4:2:2 (a + b + (x & 1)) >> 1, x the output column
 *   FDCT     libjpeg's jpeg_fdct_islow on sample - 128 (13-bit constants, 2 pass-1 bits, rows then columns)
 *   quantise sign(x) * ((|x| + (d >> 1)) / d), d = 8 * q[k]
 *   dummy    a luma block outside ceil(width / 8) x ceil(height / 8): all AC zero, DC that of the nearest preceding real block
 *            of its MCU
 *   bits     Annex K typical Huffman tables; the DC difference against the previous block of the component in scan order
 * descs (DEVICE) / h_descs (HOST copy, validated before anything is enqueued): a size outside 1..65535, an MCU grid that is
 * not the size's, a block_base that does not continue the previous image, an image outside bank_bytes, a workspace smaller
 * than fdet_jpeg_enc_ws_bytes, a quality outside 1..100 or n_images outside 1..65535 return FDET_EINVAL / FDET_EWORKSPACE. */
int fdet_jpeg_enc_plan(const uint8_t* bank, size_t bank_bytes, const fdet_jpeg_enc_desc* descs,
                       const fdet_jpeg_enc_desc* h_descs, int n_images, int quality, int subsampling, uint8_t* workspace,
                       size_t workspace_bytes, void* stream);

/* Phase 2, one kernel on `stream`.  h_totals: HOST copy of the workspace's total[n] after the plan has finished.  scan
 * (DEVICE, 4-byte aligned, scan_bytes): the caller has ZERO-FILLED it on `stream`; image i's stream takes the
 * ceil(total[i] / 8) bytes from scan_offset[i], most significant bit first, the last byte padded with 1-bits, NOT byte-stuffed.
 * A block stores the whole 32-bit words it owns and ORs (atomically) the partial words it shares with its neighbours.
 * Validated on the host before the launch: every total within n_blocks * FDET_JPEG_ENC_MAX_BLOCK_BITS, every scan_offset a
 * multiple of 4, the streams (each rounded up to 4 bytes) inside scan_bytes and not overlapping (ascending offsets). */
int fdet_jpeg_enc_emit(const fdet_jpeg_enc_desc* descs, const fdet_jpeg_enc_desc* h_descs, const uint32_t* h_totals,
                       int n_images, int subsampling, const uint8_t* workspace, size_t workspace_bytes, uint8_t* scan,
                       size_t scan_bytes, void* stream);

/* ---- Huffman decoding of baseline JPEG scans on the device (csrc/fdet_jpeg.hip prepare, csrc/fdet_jpeg_huff.hip kernels,
 * DESIGN.md 5p) ----
 * The entropy decoder of the section above moved to the device: the host only unstuffs the scan and builds the decode
 * tables (fdet_jpeg_scan_prepare, O(file bytes)); the device finds the symbol boundaries by self-synchronisation
 * (fdet_jpeg_huffman_sync) and writes the coefficient planes (fdet_jpeg_huffman_emit).  The planes are BYTE FOR BYTE what
 * fdet_jpeg_entropy_decode writes for every stream that function accepts; a stream it refuses sets the image's flag word,
 * and the caller decodes that image on the host, so that the error is the host decoder's.  tests/jpeg_huff_cpu_ref.py
 * restates every rule below in Python.
 *
 * Segments.  A segment is one restart interval, or the whole scan without DRI.  Its unstuffed bytes (FF 00 -> FF; fill FFs
 * in front of a marker dropped; the run ends at any marker or at the end of the file) start at a multiple of 16 bytes of the
 * scan buffer and are zero-padded to the next multiple of 16.
 *
 * Subsequences and states.  Every segment is cut into subsequences of sub_bits bits (a multiple of 32, >= 64): segment s
 * has max(1, ceil(8 * byte_len / sub_bits)) of them and one thread owns one.  The decoder's state at a subsequence
 * boundary is off | blk << 8 | z << 16: `off` (0..31) the bits between the boundary and the start of the first symbol
 * behind it (a symbol is a Huffman code plus its extra bits, at most 32 bits), `blk` the block index within the MCU, `z`
 * the zigzag index of the next coefficient (0: a DC symbol is next).  FDET_JPEG_HUFF_END stands for "the bits ran out".
 * Per subsequence g the state buffer holds three 8-byte words: [3g] its exit state, [3g+1] the blocks it completed, [3g+2]
 * 1 + the entry state it was last decoded from (0: never; the caller zero-fills the buffer before the first pass, which
 * also makes every exit state the guess (0, 0, 0)).  Subsequence 0 of a segment enters with (0, 0, 0).
 *
 * One parse step (the same in sync and emit), at bit p of a segment of B = 8 * byte_len bits, bits behind B reading as 0:
 *   code   the component's DC table when z = 0, else its AC table: the 9-bit lookahead, then maxcode / valoffset / vals
 *          for lengths 1..16 (build_huff's canonical form).  No length matches, or the value index is outside the table:
 *          event NOCODE, p += 1, nothing else changes.  The code is longer than B - p: the subsequence ends in END.
 *   DC     s = symbol; s > 16: event DCCAT, s = 0.  code + s bits > B - p: END.  The difference (receive-extend of the s
 *          bits) goes to natural position 0 of the block; z = 1.
 *   AC     r = symbol >> 4, s = symbol & 15.  s != 0: k = z + r; k > 63: event RUN, the block closes, only the code is
 *          consumed; else code + s > B - p: END; else the value goes to kNatural[k], z = k + 1 and the block closes at 64.
 *          s = 0, r = 15: z += 16, the block closes at z > 63 (no event, as in the host decoder).  s = 0, r < 15: the
 *          block closes.  Closing a block: count + 1, blk = (blk + 1) mod blocks-per-MCU, z = 0.
 * A thread parses the symbols that START inside its subsequence (p < min((k + 1) * sub_bits, B)); its exit state is
 * (p - (k + 1) * sub_bits, blk, z) when p reached the boundary and END otherwise.  An entry of END gives exit END, count 0.
 * No step stops at an event and no state carries one, which is what lets wrong guesses re-synchronise within a few
 * subsequences.
 *
 * Trailing bits.  The emit parse stops at the segment's block count.  Behind the image's last segment anything may follow,
 * as for the host decoder.  Behind any other segment the host decoder refills its 64-bit window ONCE and expects the
 * restart marker where that leaves it: with p the bit behind the segment's last block it accepts exactly when B - p <= 64
 * (its window holds floor((p + 64) / 8) bytes after any refill).  The thread that closes the segment's last block sets
 * FDET_JPEG_HUFF_TRAILING when B - p > 64, so that such a stream is the host decoder's to refuse.
 *
 * Every loop is bounded by the bits of one subsequence, every table index is masked or range-checked, every bit position
 * is checked against the segment's length and every store against the segment's block count and the plane's range; no
 * thread waits for another.  Neither entry point synchronises or allocates. */
#define FDET_JPEG_HUFF_HOST 1            /* fdet_jpeg_scan_prepare: a valid header, but decode this image on the host */
#define FDET_JPEG_HUFF_END 0x80000000u   /* the state "the bits ran out" */
#define FDET_JPEG_HUFF_NOCODE 1u         /* flag bits of an image: no matching code */
#define FDET_JPEG_HUFF_RUN 2u            /* a coefficient run past 63 */
#define FDET_JPEG_HUFF_DCCAT 4u          /* a DC category above 16 */
#define FDET_JPEG_HUFF_EXHAUSTED 8u      /* a segment's bits ended before its block count */
#define FDET_JPEG_HUFF_TRAILING 16u      /* more than 64 bits behind the blocks of a segment that is not the image's last */

typedef struct fdet_jpeg_huff_table {    /* build_huff's canonical form as a POD */
  uint8_t look_nbits[512], look_sym[512];/* 9-bit lookahead: code length (0: longer than 9 bits) and symbol */
  int32_t maxcode[18], valoffset[18];    /* per length 1..16: largest code (-1: none), value index - code */
  uint8_t vals[256];
  int32_t nvals, reserved;
} fdet_jpeg_huff_table;                  /* 1432 bytes */

typedef struct fdet_jpeg_huff_tables {
  fdet_jpeg_huff_table dc[3], ac[3];     /* per COMPONENT (the scan header's selectors resolved) */
} fdet_jpeg_huff_tables;                 /* 8592 bytes */

typedef struct fdet_jpeg_huff_segment {
  int64_t byte_offset;                   /* first unstuffed byte in the scan buffer, a multiple of 16 (prepare: relative to
                                            scan_out; the caller adds the image's base) */
  int32_t byte_len;                      /* unstuffed bytes, < 2^27 */
  int32_t first_mcu, mcu_count;          /* raster MCU index of the segment's first MCU; its MCUs */
  int32_t image;                         /* index into `images` (the caller fills this and the two below) */
  int32_t sub_first, sub_count;          /* its subsequences in the state buffer: max(1, ceil(8 * byte_len / sub_bits)) */
} fdet_jpeg_huff_segment;                /* 32 bytes */

typedef struct fdet_jpeg_huff_image {
  int64_t coef_offset[3];                /* as fdet_jpeg_desc: first int16 of component c's plane, a multiple of 8 */
  int32_t ncomp, hs, vs;                 /* luma sampling (chroma 1x1), 1x1 for ncomp = 1: fdet_jpeg_reconstruct's set */
  int32_t mcus_x, mcus_y;
  int32_t seg_first, seg_count;          /* its segments: consecutive, covering MCU 0 .. mcus_x * mcus_y - 1 in order */
  int32_t sub_first, sub_count;          /* its subsequences: those of its segments, consecutive */
  int32_t wg_first;                      /* its first workgroup of 256 subsequences: the sum of ceil(sub_count / 256) over the
                                            images before it (a workgroup finds its image by a search over these) */
  int32_t reserved[2];
} fdet_jpeg_huff_image;                  /* 72 bytes */

/* HOST, thread-safe, no HIP call.  Parses the headers as fdet_jpeg_info does (the same FDET_JPEG_UNSUPPORTED /
 * FDET_JPEG_ECORRUPT for what that refuses), fills `tables` and unstuffs the scan into segments (byte_offset, byte_len,
 * first_mcu, mcu_count; the other fields 0).  *scan_bytes receives the bytes used at scan_out (a multiple of 16), *n_segs
 * the segments.  FDET_JPEG_HUFF_HOST: out of the ordinary, decode on the host -- RSTn out of sequence, a marker other than
 * the expected RSTn or the end of the file before the last segment, a segment of 2^27 bytes or more.  FDET_EWORKSPACE: a
 * capacity is too small (align16(n) + 16 * ceil(mcus / interval) bytes and ceil(mcus / interval) segments always do).  No
 * read past bytes + n, no write past the capacities. */
int fdet_jpeg_scan_prepare(const uint8_t* bytes, size_t n, uint8_t* scan_out, size_t scan_capacity, size_t* scan_bytes,
                           fdet_jpeg_huff_segment* segs, int seg_capacity, int* n_segs, fdet_jpeg_huff_tables* tables);

/* ONE synchronisation pass on `stream`: thread k of a segment reads the exit state of k - 1 ((0, 0, 0) for k = 0); if it
 * equals the entry k was last decoded from it does nothing, else it parses its subsequence without writing coefficients,
 * stores exit state, block count and entry, and stores 1 to changed[image].  The caller zero-fills `changed` (DEVICE,
 * n_images words) before a pass and repeats passes until one leaves it all zero: that state is the unique fixed point,
 * every entry state the sequential decoder's.  Correct states advance at least one subsequence per pass, so the largest
 * sub_count of a segment (+ 1 pass to see nothing change) is enough.  scan / tables / images / segs / state are DEVICE
 * memory, h_images / h_segs the HOST copies everything is validated on before the launch: sub_bits not a multiple of 32
 * or below 64, a segment outside scan_bytes, misaligned offsets, sub counts that do not follow from byte_len, ranges that
 * are not consecutive or leave n_subs, a wg_first that is not that sum, geometry outside the supported set return FDET_EINVAL and nothing is written. */
int fdet_jpeg_huffman_sync(const uint8_t* scan, size_t scan_bytes, const fdet_jpeg_huff_tables* tables,
                           const fdet_jpeg_huff_image* images, const fdet_jpeg_huff_image* h_images, int n_images,
                           const fdet_jpeg_huff_segment* segs, const fdet_jpeg_huff_segment* h_segs, int n_segs,
                           int sub_bits, uint64_t* state, size_t n_subs, uint32_t* changed, void* stream);

/* After the passes converged, on `stream`: (1) an exclusive scan of the block counts per segment -> first_block (DEVICE,
 * n_subs words of workspace); a segment whose counts sum to less than its blocks sets FDET_JPEG_HUFF_EXHAUSTED; (2)
 * hipMemsetAsync of the coef_count int16 at `coef`; (3) every thread parses its subsequence again from its entry state and
 * stores each coefficient at coef_offset[c] + ((my * vs_c + v) * blocks_w[c] + mx * hs_c + h) * 64 + kNatural[z], the DC
 * position holding the DIFFERENCE, stopping at the segment's block count; events OR into flags[image] (DEVICE, n_images
 * words, zero-filled by the caller); (4) a prefix sum per (segment, component) over the blocks in scan order turns the
 * differences into DC values modulo 2^16.  Validation as in fdet_jpeg_huffman_sync, plus every plane inside coef_count. */
int fdet_jpeg_huffman_emit(const uint8_t* scan, size_t scan_bytes, const fdet_jpeg_huff_tables* tables,
                           const fdet_jpeg_huff_image* images, const fdet_jpeg_huff_image* h_images, int n_images,
                           const fdet_jpeg_huff_segment* segs, const fdet_jpeg_huff_segment* h_segs, int n_segs,
                           int sub_bits, const uint64_t* state, size_t n_subs, uint32_t* first_block, int16_t* coef,
                           size_t coef_count, uint32_t* flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * Int8 inference: the PoolResnet residual trunk post-training-quantised, on the integer matrix cores
 * (v_mfma_i32_16x16x64_i8).  Inference only.  The reference has no such path (it ships pruner.py and ONNX / TorchScript
 * export for deployment); the arithmetic below is this project's contract, restated in numpy by tests/q8_cpu_ref.py, and
 * the GPU results equal that restatement bit for bit.  Resnet shares the trunk (its blocks pool while the map is larger than
 * S) and enters it through an integer stem of its own, fdet_stem3_fwd_q8_u8 at the end of this block (restated by
 * tests/q8_resnet_cpu_ref.py): with it the network is integer from the frame bytes to the head's input.  PoolResnet has the
 * same kind of stem as an option, fdet_stem10_fwd_q8_u8 (restated by tests/q8_pool_stem_cpu_ref.py).
 *
 * Quantisation is symmetric: q = clamp(rintf(x * (1.0f / s)), -127, 127) (round half to even, NaN -> 0, -128 never
 * produced), x = float(q) * s.  Activation scales are per tensor, weight scales per output channel.
 *
 * Activation layout ("Q8"): int8 [N][H+2][W+2][C], channel innermost, with a one-pixel halo of ZEROS round every image
 * (0 is the real zero of a symmetric code, so a conv reads its padding from the halo and tests no bounds).  The caller
 * zero-fills a buffer once; every producer below writes real pixels only, so a buffer reused for the SAME shape keeps its
 * halo.  A buffer reused for another shape must be zero-filled again.  Base pointers are 16-byte aligned.
 *
 * Packed weights: int8 [9 taps ky*3+kx][C/64][Cout][64] -- for each tap and chunk of 64 input channels, the 64 input-channel
 * bytes of every output channel in a row (a plain permutation of [Cout][Cin][3][3]; quantize.py does it with torch).
 * ------------------------------------------------------------------------------------- */

/* 1 when Q8 tensors and fdet_q8_conv3x3 take this shape: C a multiple of 64 up to 256, 1 <= H, W <= 4096. */
int fdet_q8_supported(int C, int H, int W);

/* Bytes of a Q8 tensor, N * (H+2) * (W+2) * C; 0 for an unsupported shape or 2^31 bytes and more. */
size_t fdet_q8_act_bytes(int N, int C, int H, int W);

/* x fp32 [N,C,H,W] -> q (Q8), q = clamp(rintf(x * (1.0f / scale)), -127, 127); a NaN product (a NaN input, or 0 * inf under a
 * scale so small that its reciprocal overflows) -> 0.  Real pixels only. */
int fdet_q8_quantize(const float* x, float scale, int8_t* q, int N, int C, int H, int W, void* stream);

/* q (Q8) -> x fp32 [N,C,H,W] = float(q) * scale (what fdet_head_fwd takes).  With scale 1 the two converters carry exact
 * integers in and out. */
int fdet_q8_dequantize(const int8_t* q, float scale, float* x, int N, int C, int H, int W, void* stream);

/* 3x3 convolution, pad 1, C -> C channels, with the requantising epilogue in registers:
 *     acc = bias[co] + sum x_q * w_q                       int32, exact
 *     t   = float(acc) * mul[co]                           (int -> float RNE, one multiply)
 *     t   = t >= 0 ? t : t * slope
 *     t   = t + float(skip_q) * skip_mul                   (skip != NULL only; one multiply, one add, not fused)
 *     q   = clamp(rintf(t), -127, 127)
 *     y   = pool ? max of q over each 2x2 window : q       (pool: even H and W; y is a Q8 tensor of H/2 x W/2)
 *   x, skip [N,C,H,W] Q8; wpk packed weights (9*C*C bytes); bias [C] int32; mul [C] fp32; y Q8, not aliasing x or skip.
 * One kernel family for every supported shape: a wave computes 64 output channels of 4 rows x 16 columns, its block keeps
 * the 64 channels' weights in LDS. */
int fdet_q8_conv3x3(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, const int8_t* skip,
                    float skip_mul, int8_t* y, int N, int C, int H, int W, int pool, float slope, void* stream);

/* The un-pooled tail of the trunk in one launch: nblocks (1..16) residual blocks of 64 channels on maps of at most 16 x 16.
 *     for k = 0 .. nblocks - 1:   a = conv(h; wpk1[k], b1[k], mul1[k])
 *                                 h = conv(a; wpk2[k], b2[k], mul2[k], skip = h, skip_mul[k])
 * with conv the un-pooled fdet_q8_conv3x3 above, element for element: the result equals nblocks pairs of fdet_q8_conv3x3
 * calls byte for byte.  A workgroup keeps one image's two planes and two layers' packed weights in LDS for the whole chain.
 *   x          Q8 [N][H+2][W+2][64] with its halo of zeros; no output may alias it
 *   h_*        HOST arrays (nblocks entries) of DEVICE pointers / floats; they travel to the kernel by value, nothing is
 *              copied to the device, so the call can be captured in a HIP graph
 *   h_out      HOST array of DEVICE Q8 tensors, block k's output where h_out[k] != NULL (real pixels only); the array
 *              itself may be NULL
 *   out_f32    optional fp32 [N,64,H,W] = float(q of the last block) * out_scale, bit for bit fdet_q8_dequantize
 * At least one of h_out[nblocks - 1] and out_f32 is given; every device pointer is 16-byte aligned.
 * fdet_q8_chain_supported: 1 for C == 64 and 1 <= H, W <= 16 (launches nothing). */
int fdet_q8_chain_supported(int C, int H, int W);
int fdet_q8_chain(const int8_t* x, const int8_t* const* h_wpk1, const int32_t* const* h_b1, const float* const* h_mul1,
                  const int8_t* const* h_wpk2, const int32_t* const* h_b2, const float* const* h_mul2,
                  const float* h_skip_mul, int8_t* const* h_out, float* out_f32, float out_scale, int nblocks, int N, int C,
                  int H, int W, float slope, void* stream);

/* The PoolResnet stem on the uint8 frames (fdet_stem_fwd_ps_u8's kernel and shapes: F = 64, 3 channels, k10 s8 p2,
 * W % 4 == 0, W <= 512) with the quantiser in its epilogue: q (Q8 [N][Ho+2][Wo+2][64], 16-byte aligned) receives
 * clamp(rintf(t), -127, 127), NaN -> 0, of t = (acc + bias) * (1.0f / scale) -- the bytes of fdet_u8_to_f32_norm ->
 * fdet_stem_fwd_bf16x3 -> fdet_q8_quantize(scale).  Real pixels only: the halo is untouched.  Large batches run as
 * consecutive launches over image chunks.  fdet_stem_fwd_q8_ok: the entry point accepts N images of this shape (launches
 * nothing). */
int fdet_stem_fwd_q8_u8(const unsigned char* frames, const float* w, const float* bias, float scale, int8_t* q,
                        int N, int Cin, int F, int H, int W, int k, int stride, int pad, void* stream);
int fdet_stem_fwd_q8_ok(int N, int Cin, int F, int H, int W, int k, int stride, int pad);

/* The Resnet stem (3x3, stride 2, pad 1, 3 -> F channels) on the uint8 frames in INTEGER arithmetic, on the integer matrix
 * cores (v_mfma_i32_16x16x32_i8): the network is integer from the frame bytes to the head's input.  The input is the frame
 * itself, codes x_u8 in 0..255 with the fixed scale s_in = 1.0f / 255.0f, and the weights are prepared exactly as for a
 * trunk conv, (w_q, b_q, mul) from (conv1.weight, conv1.bias, s_in, s_out):
 *     acc = b_q[co] + sum over (ci,ky,kx) of x_u8[ci][2oy+ky-1][2ox+kx-1] * w_q[co][ci][ky][kx]    int32, exact; outside
 *                                                                                                   the image: 0
 *     t   = float(acc) * mul[co]                            (int -> float RNE, one fp32 multiply)
 *     q   = clamp(rintf(t), -127, 127)                      (half to even; no LeakyReLU: the reference's stem has none)
 *   frames  planar uint8 [N][3][H][W]
 *   w_q     int8 [F][32], k = (ci*3+ky)*3+kx, bytes 27..31 of every row ZERO (a plain reshape and pad of [F][3][3][3];
 *           quantize.py does it with torch)
 *   b_q     int32 [F];  mul fp32 [F]
 *   q       Q8 [N][Ho+2][Wo+2][F] with Ho = H / 2, Wo = W / 2: real pixels only, the halo is untouched
 * Accepted: Cin == 3, F a multiple of 64 up to 256, H and W even, 2 <= H, W <= 4096, q under 2^31 bytes; w_q, b_q, mul and q
 * 16-byte aligned.  (The kernel stages the rows as x - 128 for the signed MFMA and folds 128 * sum(w_q[co]) into the bias:
 * internal, exact, the entry takes the plain contract values.)  Large batches run as consecutive launches over image chunks.
 * fdet_stem3_fwd_q8_ok: the entry point accepts N images of this shape (launches nothing). */
int fdet_stem3_fwd_q8_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                         int N, int Cin, int F, int H, int W, void* stream);
int fdet_stem3_fwd_q8_ok(int N, int Cin, int F, int H, int W);

/* The PoolResnet stem (10x10, stride 8, pad 2, 3 -> F channels) on the uint8 frames in the same INTEGER arithmetic, on
 * v_mfma_i32_16x16x64_i8 (restated by tests/q8_pool_stem_cpu_ref.py).  The input is the frame itself at the fixed scale
 * s_in = 1.0f / 255.0f, (w_q, b_q, mul) are prepared exactly as for a trunk conv from (conv1.weight, conv1.bias, s_in, s_out):
 *     acc = b_q[co] + sum over (ci,ky,kx) of x_u8[ci][8oy+ky-2][8ox+kx-2] * w_q[co][ci][ky][kx]    int32, exact; outside
 *                                                                                                   the image: 0
 *     t   = float(acc) * mul[co]                            (int -> float RNE, one fp32 multiply)
 *     q   = clamp(rintf(t), -127, 127)                      (half to even; no LeakyReLU: the reference's stem has none)
 *   frames  planar uint8 [N][3][H][W]
 *   w_q     int8 [F][32][16]: row kr = ci*10+ky (rows 30 and 31 ZERO), slot kx (slots 10..15 ZERO) -- 512 bytes per output
 *           channel, a plain permutation of [F][3][10][10] plus zero padding (hotpath.q8_pack_stem10_weights does it with torch)
 *   b_q     int32 [F];  mul fp32 [F]
 *   q       Q8 [N][Ho+2][Wo+2][F] with Ho = (H - 6) / 8 + 1, Wo = (W - 6) / 8 + 1 (integer division): real pixels only, the
 *           halo is untouched, nothing is written past the tensor
 * Accepted: Cin == 3, F a multiple of 64 up to 256, 6 <= H, W <= 4096 (no alignment requirement on W: rows are read as
 * bytes where W % 4 != 0 or the frame pointer is not 4-byte aligned), q under 2^31 bytes; w_q, b_q, mul and q 16-byte
 * aligned.  (The kernel stages the rows as x - 128 for the signed MFMA and folds 128 * sum(w_q[co]) into the bias: internal,
 * exact, the entry takes the plain contract values.)  Large batches run as consecutive launches over image chunks.
 * fdet_stem10_fwd_q8_ok: the entry point accepts N images of this shape (launches nothing). */
int fdet_stem10_fwd_q8_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                          int N, int Cin, int F, int H, int W, void* stream);
int fdet_stem10_fwd_q8_ok(int N, int Cin, int F, int H, int W);

/* ---------------------------------------------------------------------------------------
 * Int8 inference: the separable block of SeparableCNN (csrc/fdet_q8_sep.hip; restated by tests/q8_sep_cpu_ref.py, and the GPU
 * results equal that restatement bit for bit).  The reference block (models/SeparableCNN.py, no bias anywhere) is
 *     pw1 1x1 -> LeakyReLU -> depthwise 3x3 pad 1 -> LeakyReLU -> pw2 1x1 -> + skip -> MaxPool2d(2) iff pooled
 * With the symmetric quantisation, the Q8 layout and the single-rounding float steps of "Int8 inference" above (int -> float
 * is RNE, each float operation is one fp32 operation and never fused, rintf rounds half to even, the clamp is to +-127, NaN
 * cannot arise):
 *     acc1[co] = sum_ci h_q[ci] * w1_q[co][ci]                          int32, exact
 *     a_q      = clamp(rintf(lrelu(float(acc1) * mul1[co])))
 *     acc2[c]  = sum_{ky,kx} a_q[c][y+ky-1][x+kx-1] * wd_q[c][ky][kx]   int32, exact; a_q outside the image is 0
 *     b_q      = clamp(rintf(lrelu(float(acc2) * mul2[c])))
 *     acc3[co] = sum_c b_q[c] * w2_q[co][c]                             int32, exact
 *     t        = float(acc3) * mul3[co] + float(h_q[co]) * skip_mul     (two multiplies, one add)
 *     q        = clamp(rintf(t));   y = pool ? max of q over each 2x2 window : q
 * with lrelu(t) = t >= 0 ? t : t * slope.  For block k with activation scales s_h[k] (input), s_a[k], s_b[k] (the two
 * intermediates) and s_h[k+1] (output): mul1 = (s_w1 * s_h[k]) / s_a[k], mul2 = (s_wd * s_a[k]) / s_b[k],
 * mul3 = (s_w2 * s_b[k]) / s_h[k+1], skip_mul = s_h[k] / s_h[k+1]; weight scales are per output channel (per channel for
 * the depthwise filter), absmax / 127, 1 for a channel of zeros, exactly as for a trunk conv and with no bias term.
 *   x        Q8 [N][H+2][W+2][C] with its halo of zeros
 *   w1, w2   int8 [Cout][Cin] rows
 *   wd       int8 [9][C], tap ky*3+kx major (a plain permutation of [C][1][3][3]; hotpath.q8_pack_sep_dw does it with torch)
 *   mul1..3  fp32 [C]
 *   y        Q8 [N][H+2][W+2][C], or [N][H/2+2][W/2+2][C] when pooled (even H and W): real pixels only; may not alias x
 * Every pointer is 16-byte aligned.  One launch: a workgroup owns one image x one tile of tile_rows x tile_cols pixels.
 * tile_rows = tile_cols = 0 lets the planner choose (fdet_q8_sepblock_plan); non-zero values force a tiling (both even when
 * pooled; FDET_EINVAL when the tile does not fit the 160 KB of LDS) -- same bytes, for tests that put band and segment seams
 * on small maps.
 * fdet_q8_sepblock_supported: 1 for C in {64, 128} and 1 <= H, W <= 4096 (launches nothing).
 * fdet_q8_sepblock_plan: the planner's tile and its LDS bytes; 1, or 0 for an unsupported shape (or odd H, W when pooled). */
int fdet_q8_sepblock_supported(int C, int H, int W);
int fdet_q8_sepblock_plan(int C, int H, int W, int pool, int* rows, int* cols, size_t* lds_bytes);
int fdet_q8_sepblock(const int8_t* x, const int8_t* w1, const float* mul1, const int8_t* wd, const float* mul2, const int8_t* w2,
                     const float* mul3, float skip_mul, int8_t* y, int N, int C, int H, int W, int pool, int tile_rows,
                     int tile_cols, float slope, void* stream);

/* nblocks (1..16) un-pooled separable blocks of 64 channels on maps of at most 16 x 16 in one launch: the result equals
 * nblocks calls of fdet_q8_sepblock byte for byte.  A workgroup keeps one image's planes and the blocks' parameters in LDS
 * for the whole chain.
 *   h_*        HOST arrays (nblocks entries) of DEVICE pointers / floats, as for fdet_q8_chain: they travel to the kernel by
 *              value, so the call can be captured in a HIP graph
 *   h_out      HOST array of DEVICE Q8 tensors, block k's output where h_out[k] != NULL (real pixels only); may be NULL
 *   out_f32    optional fp32 [N,64,H,W] = float(q of the last block) * out_scale, bit for bit fdet_q8_dequantize
 * At least one of h_out[nblocks - 1] and out_f32 is given; no output may alias x; every device pointer is 16-byte aligned.
 * fdet_q8_sepchain_supported: 1 for C == 64 and 1 <= H, W <= 16 (launches nothing). */
int fdet_q8_sepchain_supported(int C, int H, int W);
int fdet_q8_sepchain(const int8_t* x, const int8_t* const* h_w1, const float* const* h_mul1, const int8_t* const* h_wd,
                     const float* const* h_mul2, const int8_t* const* h_w2, const float* const* h_mul3, const float* h_skip_mul,
                     int8_t* const* h_out, float* out_f32, float out_scale, int nblocks, int N, int C, int H, int W, float slope,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * Int8 inference: mixed widths -- the SSD detector (csrc/fdet_q8.hip, the stem in csrc/fdet_stem_q8.hip; restated by
 * tests/q8_ssd_cpu_ref.py, and the GPU results equal that restatement bit for bit).  SSD(filters = 16) has 16, 32, 64, 128 and 256 channels, blocks whose width
 * changes (each with a 1x1 skip conv), a floor pool 15 -> 7, four Linear(C,5) heads and a 16-filter stem: none of it fits
 * the entries above, which keep their shapes and refusals.  Quantisation, the Q8 layout, the preparation of (w_q, b_q, mul)
 * and the single-rounding float steps are those of "Int8 inference" above; accumulation is exact int32 (Cin <= 256:
 * |acc| < 2^26 + |b_q|).
 *
 * Here a Q8 tensor has C any multiple of 16 up to 256 (fdet_q8x_supported / fdet_q8x_act_bytes; the old helpers keep their
 * answers).
 *
 * Packed weights ("Q8X"): flatten K tap-major, channel-minor, k = tap * Cin + ci (tap = ky*3+kx; a 1x1 conv has the one tap
 * and k = ci), zero-pad K to a multiple of 64, lay out as int8 [K/64][Cout][64] -- a plain permutation of [Cout][Cin][3][3]
 * plus zero bytes (hotpath.q8x_pack_weights does it with torch).  For Cin a multiple of 64 this is the packed order of
 * fdet_q8_conv3x3.
 * ------------------------------------------------------------------------------------- */

/* 1 when Q8 tensors of this shape exist for the entries below: C a multiple of 16 up to 256, 1 <= H, W <= 4096. */
int fdet_q8x_supported(int C, int H, int W);

/* Bytes of such a tensor, N * (H+2) * (W+2) * C; 0 for an unsupported shape or 2^31 bytes and more. */
size_t fdet_q8x_act_bytes(int N, int C, int H, int W);

/* 3x3 convolution, pad 1, Cin -> Cout channels, with the epilogue of fdet_q8_conv3x3 element for element:
 *     acc = bias[co] + sum x_q * w_q                       int32, exact
 *     t   = float(acc) * mul[co]
 *     t   = t >= 0 ? t : t * slope
 *     t   = t + float(skip_q) * skip_mul                   (skip != NULL only; skip has Cout channels)
 *     q   = clamp(rintf(t), -127, 127)
 *     y   = pool ? max of q over each 2x2 window : q
 * The pool is a FLOOR pool: y is H/2 x W/2 by integer division, and an odd last row or column takes part in no window
 * (15 -> 7); for even maps it is the pool of fdet_q8_conv3x3.
 *   x [N,Cin,H,W] Q8; skip [N,Cout,H,W] Q8 or NULL; wpk Q8X packed weights; bias [Cout] int32; mul [Cout] fp32;
 *   y Q8 [N,Cout,H,W] or [N,Cout,H/2,W/2], real pixels only, not aliasing x or skip.
 * Accepted: Cin and Cout multiples of 16 up to 256, 1 <= H, W <= 4096 (at least 2 x 2 when pooled), every tensor under 2^31
 * bytes and 16-byte aligned.  A block computes 16, 32 or 64 output channels (no channel is computed and thrown away).
 * fdet_q8x_conv3x3_ok: the entry accepts this shape (launches nothing). */
int fdet_q8x_conv3x3_ok(int N, int Cin, int Cout, int H, int W, int pool);
int fdet_q8x_conv3x3(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, const int8_t* skip,
                     float skip_mul, int8_t* y, int N, int Cin, int Cout, int H, int W, int pool, float slope, void* stream);

/* The 1x1 skip conv of a block whose width changes, Cin -> Cout, identity activation:
 *     q = clamp(rintf(float(bias[co] + sum_ci x_q[ci] * w_q[co][ci]) * mul[co]), -127, 127)
 * written as a Q8 tensor of Cout channels (real pixels only; y may not alias x).  wpk: Q8X packed [Cout][Cin][1][1].  Same
 * acceptance as fdet_q8x_conv3x3 without pool.  fdet_q8x_pointwise_ok launches nothing. */
int fdet_q8x_pointwise_ok(int N, int Cin, int Cout, int H, int W);
int fdet_q8x_pointwise(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, int8_t* y, int N, int Cin, int Cout,
                       int H, int W, void* stream);

/* Linear(C,5) at every position of a Q8 map:
 *     z[n][o][y][x] = float(b_q[o] + sum_c h_q[c] * w_q[o][c]) * m[o]         (int -> float RNE, one fp32 multiply)
 * with m = s_w * s_in (one fp32 multiply on the host) and b_q = rint(b / (s_w * s_in)).  z is fp32 [N,5,H,W], what
 * fdet_ssd_head_pack_fwd takes (CP = 5): sigmoid and priors stay the float kernel.
 *   x Q8 [N,C,H,W]; w_q int8 [5][C] rows; b_q int32 [5]; m fp32 [5]; every pointer 16-byte aligned.
 * fdet_q8x_head_ok launches nothing. */
int fdet_q8x_head_ok(int N, int C, int H, int W);
int fdet_q8x_head_f32(const int8_t* x, const int8_t* w_q, const int32_t* b_q, const float* m, float* z, int N, int C, int H, int W,
                      void* stream);

/* fdet_stem3_fwd_q8_u8's contract, unchanged, for F a multiple of 16 up to 256 (the SSD stem has 16 filters): uint8 frames
 * as codes of scale 1 / 255, 27 taps, t = float(acc) * mul[co], no LeakyReLU, Q8 output of H/2 x W/2, w_q int8 [F][32].  For
 * F % 64 == 0 it is the existing entry.  fdet_stem3_fwd_q8x_ok launches nothing. */
int fdet_stem3_fwd_q8x_ok(int N, int Cin, int F, int H, int W);
int fdet_stem3_fwd_q8x_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                          int N, int Cin, int F, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDET_H */
