/*
 * libunflow_hip.so — C ABI of the MI355X-native UnFlow training-step kernels.
 *
 * This is the drop-in boundary for the reference's operator layer
 * (src/e2eflow/ops.py:69-107 and the host launchers declared in
 * ops/correlation_op.cc:22-36, ops/backward_warp_op.cc:22-31,
 * ops/forward_warp_op.cc:23-30, ops/downsample_op.cc:21-23), widened — as the
 * north star asks — to the conv/deconv stacks (slim.conv2d / conv2d_transpose in
 * src/e2eflow/core/flownet.py), image_warp (core/image_warp.py) and the loss
 * terms (core/losses.py) that the reference leaves to TensorFlow.
 *
 * Conventions
 *  - All tensors are device pointers to fp32 (the reference's ops are
 *    `float`-only: REGISTER_OP(... ": float") in every ops/[name]_op.cc).
 *  - The caller allocates every output and workspace; the library never
 *    allocates, frees or synchronises (TF's allocate_output replaced by
 *    caller-owned buffers).  Every entry takes a hipStream_t (as void*) and is
 *    fully asynchronous and re-entrant.  The only process-wide state is the
 *    option table below (kernel selection / planning switches), written solely
 *    through unflow_set_option; the library never reads the environment.
 *  - Return value: 0 on success, a negative UNFLOW_ERR_* otherwise; on error
 *    nothing is launched (mirrors OP_REQUIRES -> InvalidArgument).
 *  - Layouts at the op boundary are the reference's: correlation NCHW
 *    (correlation_op.cc:53-56,64), warps / downsample NHWC with flow channel
 *    0 = x/u, 1 = y/v (backward_warp_op.cu.cc:26-28).  The *_nhwc entry points
 *    and the conv/loss entry points are channels-last with an explicit channel
 *    stride ("ld") so that producers write straight into channel slices of a
 *    consumer's concat buffer.
 */
#ifndef UNFLOW_HIP_H_
#define UNFLOW_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* unflow_stream_t; /* hipStream_t */
typedef struct unflow_planes unflow_planes; /* 16-bit operand planes of a tensor (defined with the conv entry points) */

#define UNFLOW_OK 0
#define UNFLOW_ERR_NULL (-1)          /* null pointer argument                                   */
#define UNFLOW_ERR_EMPTY_OUTPUT (-2)  /* correlation_op.cc:60-61 "Invalid correlation settings"   */
#define UNFLOW_ERR_EVEN_KERNEL (-3)   /* correlation_op.h:16-17  "kernel_size must be odd"         */
#define UNFLOW_ERR_NOT_DIVISIBLE (-4) /* downsample_op.cc:37-40                                    */
#define UNFLOW_ERR_SHAPE (-5)         /* correlation_op.cc:47-48 "Input shapes have to be the same" and other shape errors */
#define UNFLOW_ERR_UNSUPPORTED (-7)   /* configuration outside what the kernels implement          */
#define UNFLOW_ERR_LAUNCH (-8)        /* hipGetLastError() after launch                            */
#define UNFLOW_ERR_WORKSPACE (-9)     /* workspace too small                                       */

const char* unflow_status_string(int status);
int unflow_version(void);

/* Library options (csrc/options.h lists them with their defaults): integer switches that select kernels and split
 * planning — e.g. "conv_math_fp32", "halo", "gather_max_split".  They replace what the reference fixes at build time
 * through its JIT compile flags (src/e2eflow/ops.py:21-48); set them once after loading the library, before the first
 * launch (a later change applies to the launches planned after it).  UNFLOW_ERR_UNSUPPORTED: no such option.
 * unflow_option_names: the names, '\n'-separated. */
int unflow_set_option(const char* name, int value);
int unflow_get_option(const char* name, int* value);
const char* unflow_option_names(void);

/* ===================================================================== */
/* Correlation — replaces Correlation()/CorrelationGrad()                 */
/* (ops/correlation_op.cc:22-36; kernels ops/correlation_op.cu.cc:30-248) */
/* ===================================================================== */

/* out3 = {out_channels, out_height, out_width}; geometry of correlation_op.h:36-51. */
int unflow_correlation_out_shape(int H, int W, int kernel_size, int max_displacement, int pad,
                                 int stride_1, int stride_2, int* out3);

/* Bytes of scratch the NCHW entry points ask for: channels-last fp32 staging copies (in0, in1, g0, g1, dout: the minimum they
 * accept) + room for the two inputs' bf16 x 3 operand planes where the matrix-core kernels take the shape (kernel_size 1,
 * stride_1 1, pad >= max_displacement, C % 16 == 0).  With the full size the entry points build the planes and run the
 * kernels of the training step (81-channel +-4 volume, 8 x 256 x 96 x 128: 271 / 652 us forward / backward instead of
 * 912 / 1298); with the minimum they run the fp32-input kernels. */
size_t unflow_correlation_workspace_bytes(int B, int C, int H, int W, int kernel_size,
                                          int max_displacement, int pad, int stride_1, int stride_2);

/* NCHW in, NCHW out (output 0 of the reference op; padded_0/1 are not materialised). */
int unflow_correlation_fwd(const float* in0, const float* in1, float* out, int B, int C, int H, int W,
                           int kernel_size, int max_displacement, int pad, int stride_1, int stride_2,
                           void* workspace, size_t workspace_bytes, unflow_stream_t stream);

/* CorrelationGrad (ops.py:94-104): (dOut, in0, in1) -> (grad0, grad1), all NCHW. */
int unflow_correlation_bwd(const float* dout, const float* in0, const float* in1, float* grad0, float* grad1,
                           int B, int C, int H, int W, int kernel_size, int max_displacement, int pad,
                           int stride_1, int stride_2, void* workspace, size_t workspace_bytes,
                           unflow_stream_t stream);

/* Channels-last form used inside the step.  in0/in1: [B,H,W,ld_in] (C channels used);
 * sample n of in0 is paired with sample (n + pair_shift) % B of in1 (pair_shift = B/2 with
 * in0 == in1 runs both flow directions of a [im1-features; im2-features] batch in one launch).
 * out: [B,oh,ow,ld_out], oc channels written. */
int unflow_correlation_nhwc_fwd(const float* in0, const float* in1, int ld_in, int pair_shift, float* out,
                                int ld_out, int B, int C, int H, int W, int kernel_size, int max_displacement,
                                int pad, int stride_1, int stride_2, unflow_stream_t stream);

/* grad0[n] = d/d in0[n]; grad1[m] = d/d in1[m] with m = (n + pair_shift) % B.
 * If accumulate_g1_into_g0 != 0 (requires in0 == in1 storage), both are summed into grad0
 * (grad1 may be NULL): the gradient wrt the shared feature tensor. */
int unflow_correlation_nhwc_bwd(const float* dout, int ld_dout, const float* in0, const float* in1, int ld_in,
                                int pair_shift, float* grad0, float* grad1, int ld_grad,
                                int accumulate_g1_into_g0, int B, int C, int H, int W, int kernel_size,
                                int max_displacement, int pad, int stride_1, int stride_2, unflow_stream_t stream);

/* ===================================================================== */
/* Warps / downsample — replace BackwardWarp(), BackwardWarpGrad(),        */
/* ForwardWarp(), ForwardWarpGrad(), Downsample()                          */
/* ===================================================================== */

/* ops/backward_warp_op.cu.cc:14-68: zero outside the image, floorf(float(x)+u). */
int unflow_backward_warp_fwd(const float* images, const float* flows, float* out, int B, int H, int W, int C,
                             unflow_stream_t stream);
/* ops/backward_warp_op.cu.cc:70-138: gradient wrt flows only (ops.py:80-84). */
int unflow_backward_warp_bwd(const float* dout, const float* images, const float* flows, float* dflows,
                             int B, int H, int W, int C, unflow_stream_t stream);
/* (x0,y0) integer tap corner per pixel, [B,H,W,2] int32 — for bit-exact index checks. */
int unflow_backward_warp_indices(const float* flows, int* xy0, int B, int H, int W, unflow_stream_t stream);

/* src/e2eflow/core/image_warp.py:4-76: clamp-to-edge, x + int(floor(u)); what the training graph uses.
 * im: [B_im,H,W,ld_im] (C channels used); output sample n reads image sample (n + pair_shift) % B. */
int unflow_image_warp_fwd(const float* im, int ld_im, const float* flow, float flow_scale, float* out,
                          int* idx4 /* optional [B,H,W,4] gather indices, may be NULL */, int pair_shift,
                          int B, int H, int W, int C, unflow_stream_t stream);
/* TF autodiff of that graph: d_im (scatter-add; may be NULL; must be zero-filled by the caller or
 * hold a running sum) and d_flow (multiplied by flow_scale, the derivative of flow*flow_scale). */
int unflow_image_warp_bwd(const float* dout, const float* im, int ld_im, const float* flow, float flow_scale,
                          float* d_im, float* d_flow, int accumulate_d_flow, int pair_shift, int B, int H, int W,
                          int C, unflow_stream_t stream);

/* ops/forward_warp_op.cu.cc:16-65.  deterministic == 0: float-atomic scatter like the reference
 * (summation order varies run to run).  deterministic != 0: the same scatter accumulated in 2^31-scaled
 * 64-bit integers (order-independent, bit-reproducible); needs workspace >= 8*B*H*W bytes.
 * With workspace >= unflow_forward_warp_workspace_bytes (either mode) sources whose 9 x 9 footprint leaves their
 * tile's LDS window are binned by target tile and gathered without global atomics (flows of tens of pixels: 10x faster);
 * with less, the same sums are formed with global atomics. */
size_t unflow_forward_warp_workspace_bytes(int B, int H, int W, int deterministic);
int unflow_forward_warp_fwd(const float* flows, float* out, int B, int H, int W, int deterministic,
                            void* workspace, size_t workspace_bytes, unflow_stream_t stream);
int unflow_forward_warp_bwd(const float* dout, const float* flows, float* dflows, int B, int H, int W,
                            unflow_stream_t stream);
/* {x_lo,x_hi,y_lo,y_hi} splat footprint per pixel ([B,H,W,4] int32; -1 when rejected). */
int unflow_forward_warp_ranges(const float* flows, int* ranges, int B, int H, int W, unflow_stream_t stream);

/* ops/downsample_op.cu.cc:15-49 (box mean); H,W must be divisible by scale (downsample_op.cc:37-40). */
int unflow_downsample_fwd(const float* images, float* out, int B, int H, int W, int C, int scale,
                          unflow_stream_t stream);
/* tf.image.resize_area(images, [out_h, out_w]) (core/util.py:12-14 and the odd-size branch of util.downsample, :26): area-weighted
 * mean of the source rectangle of every output pixel, NHWC. */
int unflow_resize_area(const float* images, float* out, int B, int H, int W, int C, int out_h, int out_w,
                       unflow_stream_t stream);
/* The loss pyramid's image chain downsample(., 4), downsample(., 2) x 4 (unsupervised.py:99-100,145-146) on 3-channel images in
 * one launch; levels[k] = [N, H / (4 << k), W / (4 << k), 3], k = 0..4, each bit-identical to the chained unflow_downsample_fwd
 * calls.  H, W multiples of 64 (UNFLOW_ERR_NOT_DIVISIBLE otherwise). */
int unflow_image_pyramid5(const float* images, float* const* levels, int N, int H, int W, unflow_stream_t stream);

/* ===================================================================== */
/* conv / deconv stacks — slim.conv2d / slim.conv2d_transpose of           */
/* src/e2eflow/core/flownet.py:89-237, channels-last, TF 'SAME' padding.   */
/* Channel counts of the gathered operand must be multiples of 4 (pad the  */
/* buffers; padded weights stay zero).                                     */
/* ===================================================================== */

/* y[b,oy,ox,0:Cout] = act(bias + sum_{ky,kx,ci} x[b,oy*s-pt+ky, ox*s-pl+kx, ci] * w[ky,kx,ci,co])
 * x: [B,H,W,ldx] (Cin used), w: HWIO [k,k,Cin,Cout], y: [B,ceil(H/s),ceil(W/s),ldy].
 * leaky != 0 applies max(0.1*v, v) (flownet.py:84-86). bias may be NULL. */
int unflow_conv2d_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int B,
                      int H, int W, int Cin, int Cout, int k, int stride, int leaky, void* workspace,
                      size_t workspace_bytes, unflow_stream_t stream);

/* dx[.,0:Cin] (+)= conv-transpose of dz with w.  Epilogue: if accumulate, adds the existing dx first;
 * then, for channels c in [act_lo, act_hi), multiplies by leaky'(act_src[., c]) (1 if >0 else 0.1),
 * turning d(output) of the producing layer into d(pre-activation).  act_src may be NULL. */
int unflow_conv2d_bwd_data(const float* dz, int lddz, const float* w, float* dx, int lddx, int B, int H, int W,
                           int Cin, int Cout, int k, int stride, int accumulate, const float* act_src,
                           int ld_act, int act_lo, int act_hi, void* workspace, size_t workspace_bytes,
                           unflow_stream_t stream);

/* dw[k,k,Cin,Cout] = sum over sites; dbias[Cout] (may be NULL) = column sums of dz.  Deterministic
 * (split partials in workspace, fixed-order reduce). */
int unflow_conv2d_bwd_filter(const float* x, int ldx, const float* dz, int lddz, float* dw, float* dbias, int B,
                             int H, int W, int Cin, int Cout, int k, int stride, void* workspace,
                             size_t workspace_bytes, unflow_stream_t stream);

/* slim.conv2d_transpose(k=4, stride=2, SAME): y is [B,2H,2W,ldy]; w: [4,4,Cout,Cin] (TF layout). */
int unflow_conv2d_transpose_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
                                int B, int H, int W, int Cin, int Cout, int leaky, void* workspace,
                                size_t workspace_bytes, unflow_stream_t stream);
int unflow_conv2d_transpose_bwd_data(const float* dz, int lddz, const float* w, float* dx, int lddx, int B, int H,
                                     int W, int Cin, int Cout, int accumulate, const float* act_src, int ld_act,
                                     int act_lo, int act_hi, void* workspace, size_t workspace_bytes,
                                     unflow_stream_t stream);
int unflow_conv2d_transpose_bwd_filter(const float* x, int ldx, const float* dz, int lddz, float* dw, float* dbias,
                                       int B, int H, int W, int Cin, int Cout, void* workspace,
                                       size_t workspace_bytes, unflow_stream_t stream);

/* All bias gradients of a step in two launches: out[i][c] = sum over the npix[i] rows of x[i][., c]
 * (x[i]: [npix[i], ld[i]] slice with C[i] columns).  The pointer/size arrays are HOST arrays, n <= 32.
 * Deterministic (fixed-order chunked reduction). */
size_t unflow_colsum_batched_workspace_bytes(int n, const int* C);
int unflow_colsum_batched(int n, const float* const* x, const int* ld, const long* npix, const int* C,
                          float* const* out, void* workspace, size_t workspace_bytes, unflow_stream_t stream);

/* Exact workspace requirement of the conv/deconv entry points above for these dimensions. */
size_t unflow_conv_workspace_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride);

/* dz[., c] = dy[., c] * leaky'(y[., c]) in place over a [npix, C] slice (stand-alone form of the epilogue). */
int unflow_leaky_bwd_inplace(float* dy, int lddy, const float* y, int ldy, long npix, int C, unflow_stream_t stream);

/* ===================================================================== */
/* loss terms — src/e2eflow/core/losses.py, fused per pyramid level.        */
/* A "directed batch" holds both flow directions: samples [0,B) forward,    */
/* [B,2B) backward; image sample n is paired with (n + B) % 2B.             */
/* ===================================================================== */

/* gray[b,y,x] = 255 * (0.2989 R + 0.5870 G + 0.1140 B)  (losses.py:94, tf.image.rgb_to_grayscale). */
int unflow_rgb_to_gray255(const float* im, int ld_im, float* gray, long npix, unflow_stream_t stream);

/* image_warp of a 3-channel image followed by the grayscale above, fused (losses.py:22-23,94);
 * taps are re-derived in the backward pass. out_gray: [N,H,W]. */
int unflow_warp_gray_fwd(const float* im, int ld_im, const float* flow, float flow_scale, float* out_gray,
                         int pair_shift, int N, int H, int W, unflow_stream_t stream);
/* d_flow (+)= flow_scale * d(gray_warped)/d(flow) * d_gray. */
int unflow_warp_gray_bwd(const float* d_gray, const float* im, int ld_im, const float* flow, float flow_scale,
                         float* d_flow, int accumulate, int pair_shift, int N, int H, int W,
                         unflow_stream_t stream);

/* ternary_loss (losses.py:90-122) on gray images: per pixel soft-Hamming distance of the census
 * transforms, Charbonnier (alpha .45, eps 1e-3), masked by mask*interior(max_distance), summed into
 * loss_acc[0] scaled by `weight`/(normalizer).  dist_out [N,H,W] receives d(weighted loss)/d(distance) per
 * pixel (mask, interior and weight folded in) — the only thing the backward pass needs.  mask: [N_mask,H,W] with
 * sample n using mask[n % N_mask].  max_distance <= 4 (the reference uses 1..3, unsupervised.py:88). */
int unflow_ternary_fwd(const float* gray1, const float* gray2w, const float* mask, int n_mask, float* dist_out,
                       float* loss_acc, float weight, float normalizer, int max_distance, int N, int H, int W,
                       unflow_stream_t stream);
/* d_gray2w = d(weight * loss)/d(gray2w)  (gather form, no atomics); `dist` is dist_out of unflow_ternary_fwd (the
 * mask / weight arguments are kept for signature symmetry and ignored). */
int unflow_ternary_bwd(const float* gray1, const float* gray2w, const float* mask, int n_mask,
                       const float* dist, float* d_gray2w, float weight, float normalizer, int max_distance,
                       int N, int H, int W, unflow_stream_t stream);

/* Fused forms the step driver uses (same arithmetic, fewer launches per pyramid level):
 * unflow_gray_pair        = unflow_rgb_to_gray255(im) + unflow_warp_gray_fwd(im, flow) in one launch;
 * unflow_ternary_warp_bwd = unflow_ternary_bwd followed by unflow_warp_gray_bwd, without materialising d_gray2w
 *                           (`dist` = the per-pixel weights left by unflow_ternary_fwd). */
int unflow_gray_pair(const float* im, int ld_im, const float* flow, float flow_scale, float* gray1, float* gray2w,
                     int pair_shift, int N, int H, int W, unflow_stream_t stream);
int unflow_ternary_warp_bwd(const float* gray1, const float* gray2w, const float* dist, const float* im, int ld_im,
                            const float* flow, float flow_scale, float* d_flow, int accumulate, int pair_shift,
                            int max_distance, int N, int H, int W, unflow_stream_t stream);

/* second_order_loss (losses.py:258-295) on flow*flow_scale; loss_acc[0] += weight * sum/normalizer;
 * d_flow (+)= gradient wrt the raw flow (includes flow_scale).  Either output may be NULL. */
int unflow_second_order_fwd_bwd(const float* flow, float flow_scale, float* loss_acc, float* d_flow,
                                int accumulate, float weight, float normalizer, int N, int H, int W,
                                unflow_stream_t stream);

/* Masks and the non-data terms of compute_losses (losses.py:25-73) in one pass over the directed batch:
 *   mask = base_mask (broadcast over n_base samples; the down-sampled border mask) or, when base_mask is NULL,
 *          create_outgoing_mask(flow*flow_scale) (losses.py:347-366);
 *   fb_occ = |f + w|^2 > 0.01(|f|^2 + |w|^2) + 0.5 with w = warped_other*flow_scale (losses.py:43-49);
 *   disocc_other = fwarp[(n+pair_shift)%N] < 0.8 (forward_warp of the partner's flow, losses.py:28-29);
 *   occlusion_mode 0: none, 1: 'fb' (mask *= 1-fb_occ), 2: 'disocc' (mask *= 1-disocc_other) (losses.py:51-56);
 *   loss_acc += occ_weight*charb(1-mask) + sym_weight*charb((1-mask)-disocc_other) + fb_weight*charb(f+w, mask),
 *   each with the reference's normaliser (batch_per_direction*H*W*channels).
 * mask_out [N,H,W] (may be NULL) receives the final mask for the data terms.  Only 'fb' is differentiable:
 * d_flow (+)= its gradient wrt the raw flow, d_warped = its gradient wrt warped_other (feed to
 * unflow_image_warp_bwd).  warped_other / fwarp may be NULL when no term needs them. */
int unflow_mask_terms(const float* flow, const float* warped_other, const float* fwarp, const float* base_mask,
                      int n_base, float flow_scale, int occlusion_mode, float* mask_out, float* loss_acc, float* d_flow,
                      float* d_warped, int accumulate, float fb_weight, float occ_weight, float sym_weight,
                      int batch_per_direction, int pair_shift, int N, int H, int W, unflow_stream_t stream);

/* compute_losses with the DEFAULT terms (ternary/census + second-order smoothness, config.ini [train]) over the whole
 * loss pyramid (unsupervised.py:85-147) in four launches instead of four per level.  Same arithmetic as
 * unflow_second_order_fwd_bwd + unflow_gray_pair + unflow_ternary_fwd + unflow_ternary_warp_bwd per level.
 * ternary_scale / smooth_scale are the complete factors layer_weight * term_weight / normaliser of the level.
 * loss_acc[0] += the weighted loss; with_grad: d_flow of every level is OVERWRITTEN with d loss / d flow. */
#define UNFLOW_MAX_PYR_LEVELS 7
typedef struct unflow_pyr_level {
  const float* im;      /* [N,H,W,3] images in [0,1] of this level */
  const float* flow;    /* [N,H,W,2] raw network flow of this level */
  float* gray1;         /* [N,H,W] scratch */
  float* gray2w;        /* [N,H,W] scratch */
  const float* mask;    /* [n_mask,H,W] */
  float* dist;          /* [N,H,W] scratch (per-pixel census weights) */
  float* d_flow;        /* [N,H,W,2] out (may be NULL when with_grad == 0) */
  int H, W, n_mask, max_distance;
  float flow_scale, ternary_scale, smooth_scale;
} unflow_pyr_level;
/* sizeof(unflow_pyr_level) as compiled into the library (bindings check their struct layout against it) */
int unflow_sizeof_pyr_level(void);
int unflow_loss_pyramid_default(const unflow_pyr_level* levels, int n_levels, int N, int pair_shift, float* loss_acc,
                                int with_grad, unflow_stream_t stream);

/* photometric_loss (losses.py:198-199): charbonnier(im1 - image_warp(im2, flow), mask, beta=255), fused with the warp;
 * loss_acc[0] += weight*sum/normalizer; d_flow (+)= gradient wrt the raw flow.  mask: [n_mask,H,W]. */
int unflow_photometric_fwd_bwd(const float* im, int ld_im, const float* flow, float flow_scale, const float* mask,
                               int n_mask, float* loss_acc, float* d_flow, int accumulate, float weight, float normalizer,
                               int pair_shift, int N, int H, int W, unflow_stream_t stream);

/* charbonnier_loss (losses.py:298-322), the stand-alone form: loss_acc[0] += weight * sum(min(mask * ((x*beta)^2 +
 * epsilon^2)^alpha, truncate)) / (npix*C) over x [npix, C]; mask [npix, mask_channels], mask_channels 1 or C, or NULL;
 * truncate < 0: none.  length_sq (losses.py:12-13): out[i] = sum_c x[i,c]^2. */
int unflow_charbonnier_loss(const float* x, const float* mask, int mask_channels, float truncate, float alpha, float beta,
                            float epsilon, float* loss_acc, float weight, long npix, int C, unflow_stream_t stream);
int unflow_length_sq(const float* x, float* out, long npix, int C, unflow_stream_t stream);

/* smoothness_loss (losses.py:206-255): first-order forward differences of flow*flow_scale, Charbonnier. */
int unflow_smooth_1st_fwd_bwd(const float* flow, float flow_scale, float* loss_acc, float* d_flow, int accumulate,
                              float weight, float normalizer, int N, int H, int W, unflow_stream_t stream);

/* gradient_loss (losses.py:225-247): Sobel-gradient constancy between im1 and the warped second image [N,H,W,3].
 * fwd writes gdiff [N,H,W,6] = d(weighted loss)/d(diff); bwd turns it into d/d(im2_warped) [N,H,W,3]
 * (then unflow_image_warp_bwd gives the flow gradient). */
int unflow_gradient_loss_fwd(const float* im1, int ld_im1, const float* im2_warped, const float* mask, int n_mask,
                             float* gdiff, float* loss_acc, float weight, float normalizer, int N, int H, int W,
                             unflow_stream_t stream);
int unflow_gradient_loss_bwd(const float* gdiff, float* d_im2_warped, int N, int H, int W, unflow_stream_t stream);

/* ===================================================================== */
/* step plumbing                                                           */
/* ===================================================================== */

/* net input: out[n,y,x,0:3] = im[n,y,x,:]/255 - mean[c]/255, out[...,3] = 0 ([N,H,W,4]);
 * loss image: out01[n,y,x,0:3] = im/255 (unsupervised.py:29-32,69-70). out01 may be NULL. */
int unflow_prepare_images(const float* im_u8range, float* net_in4, float* out01, const float* mean3, long npix,
                          unflow_stream_t stream);

/* Both frames in one launch: im1 -> samples [0, B), im2 -> samples [B, 2B) of the directed batch (npix_each = B*H*W each);
 * net_pl (may be NULL): also the 16-bit operand planes of net_in4 (row length net_pl->ld = 4 or 8). */
int unflow_prepare_image_pair(const float* im1, const float* im2, long npix_each, float* net_in4, float* out01,
                              const float* mean3, const unflow_planes* net_pl, unflow_stream_t stream);

/* Elementwise helpers of the step driver (what the TF graph does with tf.multiply / tf.add_n / tf.zeros between ops):
 * y = s*x; y *= x; y += x (n floats); stream-ordered zero fill and device-to-device copy. */
int unflow_scale(const float* x, float s, float* y, long n, unflow_stream_t stream);
int unflow_mul_inplace(float* y, const float* x, long n, unflow_stream_t stream);
int unflow_add_inplace(float* y, const float* x, long n, unflow_stream_t stream);
int unflow_zero(void* p, size_t bytes, unflow_stream_t stream);
int unflow_copy(void* dst, const void* src, size_t bytes, unflow_stream_t stream);

/* ---- augmentation ---------------------------------------------------------------------- */

/* Spatial-transformer resampling of core/spatial_transformer.py:56-175 as used by random_affine
 * (core/augment.py:50-55): out[b,i,j,:] = bilinear sample of U[b % n_u] at theta[b % n_theta] @ (x_t, y_t, 1),
 * x_t/y_t = linspace(-1,1,out_w/out_h), source coords (x_s+1)*W/2, indices clipped to the image BEFORE the
 * weights are formed (:84-87,113-120).  theta: DEVICE [n_theta,2,3] row-major.  U channels-last with channel
 * stride ld_u; out with ld_out.  No gradient (the reference wraps the result in stop_gradient, augment.py:54). */
int unflow_stn_affine_fwd(const float* U, int n_u, int ld_u, const float* theta, int n_theta, float* out, int ld_out,
                          int B, int H, int W, int C, int out_h, int out_w, unflow_stream_t stream);

/* random_photometric (core/augment.py:78-108) given its draws, fused with the mean subtraction of
 * core/unsupervised.py:67-68: out[n,y,x,c] = pow(clamp((im*(contrast+1)+brightness)*colour[c], 0, 1), 1/gamma)
 * + noise - mean3[c]/255, c < 3; channels 3..ld_out-1 are written as 0.  contrast/brightness/gamma/noise: DEVICE
 * [n_par], colour3: DEVICE [n_par,3]; sample n uses draw n % n_par.  mean3: HOST [3] in [0,255], or NULL. */
int unflow_photometric_augment(const float* im, int ld_in, float* out, int ld_out, const float* contrast,
                               const float* brightness, const float* colour3, const float* gamma, const float* noise,
                               int n_par, const float* mean3, int N, int H, int W, unflow_stream_t stream);

/* Geometric + photometric augmentation of the supervised step with its ground truth, one launch (csrc/augment_flow.hip).
 * mats: DEVICE [B][3][6] fp32, per sample the affine PIXEL maps M1, M2, M2^-1 (rows [a b c; d e f]: x' = (a x + b y) + c),
 * where A(theta; H, W) is unflow_stn_affine_fwd's map written on pixel coordinates, M1 = A(theta_global) and
 * M2 = A(theta_global) A(theta_local).  For output pixel p of sample b, s1 = M1 p and s2 = M2 p:
 *   im01 [2B,H,W,3]       rows b / b + B = im1 at s1 / im2 at s2 with unflow_stn_affine_fwd's tap rule (floor, indices clipped
 *                         before the weights, its add order) on the taps v / 255 (im1, im2: [B,H,W,3] in [0,255]);
 *   x0 [2B,H,W,ld_out]    unflow_photometric_augment's expression on those values (sample row n uses draw n % n_par; mean3:
 *                         HOST [3] in [0,255] or NULL), channels 3..ld_out-1 zero: bit-identical to that entry run on im01;
 *   flow_out [B,H,W,2], mask_out [B,H,W]  from flow_gt [B,H,W,2] and mask_gt [B,H,W] (NULL = ones):
 *     mode 0 (bilinear): f = convex bilinear of the four flow taps around s1 (a + (b - a) * alpha per row, then across the
 *                        rows), valid = the four taps lie inside the map and all their masks are > 0.5;
 *     mode 1 (nearest):  f = the tap at r = floor(s1 + 0.5), valid = r inside and mask(r) > 0.5 (sparse maps);
 *     q = M2^-1 (s1 + f); flow_out = q - p and mask_out = 1 where valid, else +0 and 0 by selection — a non-finite or marker
 *     value under an invalid tap never reaches an output.
 * The sources are gathered while the targets are written: flow_gt / mask_gt / im1 / im2 must not be the output buffers
 * (UNFLOW_ERR_UNSUPPORTED, as for mode outside {0, 1}); n_par <= 0, H or W <= 0, ld_out < 3: UNFLOW_ERR_SHAPE. */
int unflow_supervised_geo_augment(const float* im1, const float* im2, const float* flow_gt, const float* mask_gt,
                                  const float* mats, const float* contrast, const float* brightness, const float* colour3,
                                  const float* gamma, const float* noise, int n_par, const float* mean3, float* im01, float* x0,
                                  int ld_out, float* flow_out, float* mask_out, int mode, int B, int H, int W,
                                  unflow_stream_t stream);

/* Input tensor of a FlowNetS stage (flownet.py:46-59), channels-last with stride ld_out (pad channels untouched):
 * [first, second] (6 ch) when prev_flow2 == NULL, else [first, second, flow, warp(second, flow), |warp - first|]
 * (14 ch) with flow = resize_bilinear(prev_flow2 [N,h,w,2]) * flow_scale (= 4 * FLOW_SCALE).  Forward only: the
 * reference stops the gradient here unless train_all (flownet.py:51-54). */
int unflow_stack_input(const float* net_in4, const float* prev_flow2, float* out, int ld_out, int pair_shift, int N,
                       int H, int W, int h, int w, float flow_scale, unflow_stream_t stream);

/* Gradient of unflow_stack_input wrt prev_flow2 for train_all (flownet.py:51-54 without the stop_gradient): d_out is
 * the gradient wrt the 14-channel stage input (channel stride ld_out); d_prev_flow2 [N,h,w,2] is ACCUMULATED with
 * float atomics (zero it first).  The images receive no gradient (they are data). */
int unflow_stack_input_bwd(const float* d_out, int ld_out, const float* net_in4, const float* prev_flow2,
                           float* d_prev_flow2, int pair_shift, int N, int H, int W, int h, int w, float flow_scale,
                           unflow_stream_t stream);

/* ===================================================================== */
/* 16-bit operand planes (csrc/conv_planes.hip)                            */
/* The conv / conv_transpose layers above can take their operands from,     */
/* and write their results to, "operand planes": the tensor once more as    */
/* n_planes arrays of 16-bit values with the tensor's [pixel][channel]      */
/* layout (channel stride ld, a multiple of 4; plane p at base +            */
/* p*plane_stride elements):                                                */
/*   n_planes == 3: bf16 hi/mid/lo with x = hi + mid + lo exactly — the     */
/*     products are summed from six bf16 MFMA terms with fp32 accumulation, */
/*     fp32-class accuracy (the default training mode);                     */
/*   n_planes == 1: fp16 (fp16 activations/weights in, fp32 accumulate).    */
/* `base` points at channel 0 of the slice the fp32 pointer addresses.  A   */
/* consumed slice of C channels is walked in groups of 8: channels          */
/* C .. round_up_8(C)-1 of the plane rows must exist (ld >= that) and be 0. */
/* Every *_pl entry point falls back to the fp32-operand kernel of the      */
/* same op when the planes are NULL / unusable, and still writes the        */
/* output planes (y_pl / dx_pl; may be NULL).                               */
/* ===================================================================== */
typedef struct unflow_planes {
  void* base;
  long plane_stride;
  int ld;
  int n_planes;
  float scale; /* the planes hold scale * value (0 = 1).  fp16 planes of GRADIENT tensors carry a power-of-two scale so that
                  small gradients stay in fp16's normal range; producers multiply, consumers divide their sums.  Must be 1
                  (or 0) for bf16 x 3 planes, which have fp32's exponent range. */
} unflow_planes;

/* unflow_correlation_nhwc_fwd with the features' operand planes (n_planes == 3, kernel_size 1, stride_1 1, C % 16 == 0):
 * the products run on the bf16 matrix cores (six terms, fp32 accumulation).  Falls back to the fp32 entry point when the
 * planes are NULL / unusable (then in0 / in1 must be given). */
int unflow_correlation_nhwc_fwd_pl(const float* in0, const float* in1, int ld_in, const unflow_planes* in0_pl,
                                   const unflow_planes* in1_pl, int pair_shift, float* out, int ld_out, int B, int C,
                                   int H, int W, int kernel_size, int max_displacement, int pad, int stride_1,
                                   int stride_2, unflow_stream_t stream);

/* unflow_correlation_nhwc_bwd with the features' operand planes (n_planes == 3, kernel_size 1, stride_1 1, C % 64 == 0): the
 * feature operand of the banded products comes from the planes (LDS-DMA + transposing reads), the band operand is split in
 * registers; six terms on the bf16 matrix cores, fp32 accumulation.  Falls back to the fp32 entry point otherwise. */
int unflow_correlation_nhwc_bwd_pl(const float* dout, int ld_dout, const float* in0, const float* in1, int ld_in,
                                   const unflow_planes* in0_pl, const unflow_planes* in1_pl, int pair_shift, float* grad0,
                                   float* grad1, int ld_grad, int accumulate_g1_into_g0, int B, int C, int H, int W,
                                   int kernel_size, int max_displacement, int pad, int stride_1, int stride_2,
                                   unflow_stream_t stream);

/* fp32 [npix][ldx] (C channels) -> planes; plane channels C .. C_fill-1 are zero-filled (C <= C_fill <= round_up_8(C),
 * C_fill a multiple of 4: a slice that ends the buffer row before the next multiple of 8 passes the row's end). */
int unflow_planes_from_f32(const float* x, int ldx, long npix, int C, int C_fill, const unflow_planes* out,
                           unflow_stream_t stream);

/* Planes of weight tensors W[taps][R][Cc] (conv: HWIO, R = Cin, Cc = Cout; conv_transpose: R = Cout, Cc = Cin):
 *   direct[i]     [p][tap][R][round_up_8(Cc)]  — operand of conv2d_bwd_data_pl and conv2d_transpose_fwd_pl
 *   transposed[i] [p][tap][Cc][round_up_8(R)]  — operand of conv2d_fwd_pl and conv2d_transpose_bwd_data_pl
 * (either may be NULL), plane stride = unflow_weight_planes_elems(...).  One launch for the whole table. */
size_t unflow_weight_planes_elems(int taps, int R, int Cc, int transposed);
int unflow_weight_planes_batched(int n, const float* const* w, const int* taps, const int* R, const int* Cc,
                                 void* const* direct, void* const* transposed, int n_planes, unflow_stream_t stream);

/* The optimizer update of train.py:151-152 (unflow_adam_step's arithmetic, bit-identical parameters) and the re-split of the
 * updated weights into their planes in ONE pass over a table of tensors W[taps][R][Cc] that live inside the flat buffers P / G /
 * M / V (identical layouts; w[i] points into P): 64 x 64 tiles, the new values go from the tile to both plane copies without a
 * second read.  direct[i] / transposed[i] may be NULL (a tensor without planes — the Cout = 2 layers, or the bias block as one
 * pseudo-tensor with taps = R = 1); regularized[i] != 0 adds l2_scale * p to the gradient (and, with loss_acc, l2_scale * 0.5 * p^2
 * of the PRE-update values to loss_acc[0], like unflow_adam_step_regloss).  n_planes 0: no tensor of the table has planes. */
int unflow_adam_planes_batched(int n, float* const* w, const int* taps, const int* R, const int* Cc, void* const* direct,
                               void* const* transposed, const int* regularized, int n_planes, float* P, const float* G, float* M,
                               float* V, float grad_scale, float l2_scale, float lr_t, float beta1, float beta2, float eps,
                               float* loss_acc, unflow_stream_t stream);

size_t unflow_conv_pl_workspace_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride, int n_planes);

/* Every Cout = 2 filter gradient of a refinement decoder (flownet.py:89-131: flowN = conv k3 -> 2, flowN_upM =
 * conv2d_transpose 2 -> 2) in one batch of two launches.  kind[i] 0: flowN head — x [B,H,W,Cin] (ldx), dz [B,H,W,2] (lddz),
 * dw [3,3,Cin,2]; kind[i] 1: flowN_upM — x [B,H,W,2], dz [B,2H,2W,2], dw [4,4,2,2] (Cin[i] = 2).  n <= 16.
 * UNFLOW_ERR_UNSUPPORTED when a layer has no strip form (W % 4 != 0): use the per-layer entry points then. */
size_t unflow_flow_wgrad_batched_workspace_bytes(int n, const int* kind, const int* B, const int* H, const int* W, const int* Cin);
int unflow_flow_wgrad_batched(int n, const int* kind, const float* const* x, const int* ldx, const float* const* dz,
                              const int* lddz, float* const* dw, const int* B, const int* H, const int* W, const int* Cin,
                              void* workspace, size_t workspace_bytes, unflow_stream_t stream);

/* Test hook (host only, no GPU): the (M tile, N tile, parity class, K split) each workgroup of a gather / halo launch decodes from
 * its linear id — XCD-contiguous remap + work order 0 / 1 / 2 of csrc/conv_planes.hip — 4 ints per workgroup, M tile = -1 for
 * the padding workgroups of order 2.  Returns the grid size (out == NULL: query only). */
int unflow_debug_work_order(int mt, int nt, int ncls, int nsplit, int order, int xcd, int* out, int out_blocks);

/* ---- gradient exchange (csrc/comm_rccl.hip): replaces average_gradients, src/e2eflow/core/train.py:388-422 ----------------
 * One process per GPU; the flat fp32 gradient buffer is summed over the ranks by RCCL (ncclAllReduce over xGMI) on the
 * caller's stream, the 1 / world factor rides in unflow_adam_step's grad_scale.  RCCL is resolved at run time:
 * unflow_comm_available() returns its version code (> 0) or 0, and without it the other calls return UNFLOW_ERR_UNSUPPORTED.
 * Bootstrap: rank 0 calls unflow_comm_unique_id (128 bytes) and passes the id to every rank out of band; every rank then
 * calls unflow_comm_init(id, nranks, rank, &comm) with its GPU current (collective: returns when all ranks have joined). */
int unflow_comm_available(void);
int unflow_comm_unique_id(void* id128);
int unflow_comm_init(const void* id128, int nranks, int rank, void** comm);
int unflow_comm_info(void* comm, int* nranks, int* rank);
/* buf[0 .. n) <- sum over the ranks, in place, enqueued on `stream`; same n and call order on every rank. */
int unflow_allreduce_sum_f32(float* buf, long n, void* comm, unflow_stream_t stream);
int unflow_comm_destroy(void* comm);

/* Persistent stream-K halo kernel (csrc/conv_streamk.hip).  Test hook (host only, no GPU) for a launch of `ncls` tap classes x
 * nt N tiles x mtp M tile pairs, every item nchunk chunks x ntaps[class] K tiles, the item list ordered M group (ngroups of
 * them) > class > N tile > pair and laid end to end in K tiles: range_pos[w] (G + 1 ints) = the first K-tile position of
 * workgroup w's range; decoded[4 i .. 4 i + 3] = (class, N tile, M pair, K tile inside the item) of position pos[i].  Returns 0,
 * or UNFLOW_ERR_SHAPE for arguments outside the kernel's limits. */
int unflow_debug_streamk_plan(int G, int mtp, int nt, int nchunk, int ncls, const int* ntaps, int ngroups, int* range_pos, int npos,
                              const int* pos, int* decoded);
/* ... and the number of bounded spins of those kernels that gave up since the last call (reads and clears a device counter:
 * must be 0; a result computed past a timeout is wrong). */
int unflow_debug_streamk_timeouts(void);

/* w_pl: the `transposed` planes of w (ld = round_up_8(Cin)). */
int unflow_conv2d_fwd_pl(const float* x, int ldx, const unflow_planes* x_pl, const float* w, const unflow_planes* w_pl,
                         const float* bias, float* y, int ldy, const unflow_planes* y_pl, int B, int H, int W, int Cin,
                         int Cout, int k, int stride, int leaky, void* workspace, size_t workspace_bytes,
                         unflow_stream_t stream);
/* w_pl: the `direct` planes of w (ld = round_up_8(Cout)); dx_pl receives channels [pl_lo, pl_hi) of dx (the range whose
 * values are final after this call, i.e. [act_lo, act_hi)).  The leaky-ReLU derivative of [act_lo, act_hi) is taken from
 * act_src (the fp32 activation) or, when act_src is NULL, from the first plane of act_pl (the sign of the activation is the
 * sign of its bf16 / fp16 leading plane).  Planes-only tensors: y (forward) / dx (data gradient, accumulate == 0) may be NULL
 * when the corresponding planes are given — a tensor that only convolutions read need not exist in fp32. */
int unflow_conv2d_bwd_data_pl(const float* dz, int lddz, const unflow_planes* dz_pl, const float* w,
                              const unflow_planes* w_pl, float* dx, int lddx, const unflow_planes* dx_pl, int pl_lo,
                              int pl_hi, int B, int H, int W, int Cin, int Cout, int k, int stride, int accumulate,
                              const float* act_src, int ld_act, const unflow_planes* act_pl, int act_lo, int act_hi,
                              void* workspace, size_t workspace_bytes, unflow_stream_t stream);
int unflow_conv2d_bwd_filter_pl(const float* x, int ldx, const unflow_planes* x_pl, const float* dz, int lddz,
                                const unflow_planes* dz_pl, float* dw, int B, int H, int W, int Cin, int Cout, int k,
                                int stride, void* workspace, size_t workspace_bytes, unflow_stream_t stream);
/* conv_transpose k4 s2: w [4,4,Cout,Cin]; fwd takes the `direct` planes (ld = round_up_8(Cin)), bwd_data the
 * `transposed` ones (ld = round_up_8(Cout)). */
int unflow_conv2d_transpose_fwd_pl(const float* x, int ldx, const unflow_planes* x_pl, const float* w,
                                   const unflow_planes* w_pl, const float* bias, float* y, int ldy,
                                   const unflow_planes* y_pl, int B, int H, int W, int Cin, int Cout, int leaky,
                                   void* workspace, size_t workspace_bytes, unflow_stream_t stream);
int unflow_conv2d_transpose_bwd_data_pl(const float* dz, int lddz, const unflow_planes* dz_pl, const float* w,
                                        const unflow_planes* w_pl, float* dx, int lddx, const unflow_planes* dx_pl,
                                        int pl_lo, int pl_hi, int B, int H, int W, int Cin, int Cout, int accumulate,
                                        const float* act_src, int ld_act, const unflow_planes* act_pl, int act_lo,
                                        int act_hi, void* workspace, size_t workspace_bytes, unflow_stream_t stream);
int unflow_conv2d_transpose_bwd_filter_pl(const float* x, int ldx, const unflow_planes* x_pl, const float* dz, int lddz,
                                          const unflow_planes* dz_pl, float* dw, int B, int H, int W, int Cin, int Cout,
                                          void* workspace, size_t workspace_bytes, unflow_stream_t stream);

/* tf.image.resize_bilinear (TF1 legacy, align_corners=False) * scale (unsupervised.py:103-104). */
int unflow_resize_bilinear_tf1(const float* in, float* out, int B, int H, int W, int C, int out_h, int out_w,
                               float scale, unflow_stream_t stream);

/* Supervised flow loss of one network (supervised.py:50-62), forward and backward in one launch (csrc/supervised.hip):
 * loss_acc[0] += weight * sum(mask * ((flow_scale * up(flow) - flow_gt)^2 + 1e-6)^0.45) / (B*H*W*2), where up() is the TF1
 * legacy bilinear resize of flow [B,h,w,2] to [H,W] with unflow_resize_bilinear_tf1's fp32 expression order (r = H/h = W/w
 * in {1, 2, 4, 8}, else UNFLOW_ERR_SHAPE); flow_gt [B,H,W,2]; mask_gt [B,H,W,1] or NULL (= ones), broadcast over u and v.
 * d_flow [B,h,w,2] (may be NULL: no gradient) receives d loss / d flow at the coarse resolution — written (accumulate = 0)
 * or added (accumulate = 1), as a gather without float atomics (bit-reproducible). */
int unflow_supervised_flow_loss(const float* flow, int h, int w, const float* flow_gt, const float* mask_gt, float flow_scale,
                                float weight, float* loss_acc, float* d_flow, int accumulate, int B, int H, int W,
                                unflow_stream_t stream);

/* Stage input of a FlowNetS refinement network of the one-direction (supervised) engine: unflow_stack_input with
 * first = first4[n], second = second4[n] ([N,H,W,4] each, e.g. the two halves of the network input), and its train_all
 * gradient wrt prev_flow2 (ACCUMULATED with float atomics, like unflow_stack_input_bwd). */
int unflow_stack_input_pair(const float* first4, const float* second4, const float* prev_flow2, float* out, int ld_out, int N,
                            int H, int W, int h, int w, float flow_scale, unflow_stream_t stream);
int unflow_stack_input_pair_bwd(const float* d_out, int ld_out, const float* first4, const float* second4,
                                const float* prev_flow2, float* d_prev_flow2, int N, int H, int W, int h, int w,
                                float flow_scale, unflow_stream_t stream);

/* Fused L2-regularised TF-form Adam over a flat parameter vector (train.py:151-152; flownet.py:176):
 * g = grad*grad_scale + (i < n_regularized ? l2_scale * p : 0);
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr_t * m / (sqrt(v) + eps). */
int unflow_adam_step(float* p, const float* grad, float* m, float* v, long n, long n_regularized, float grad_scale,
                     float l2_scale, float lr_t, float beta1, float beta2, float eps, unflow_stream_t stream);

/* Same update, and additionally loss_acc[0] += l2_scale * 0.5 * sum(p[0:n_regularized]^2) of the PRE-update
 * parameters: the regularisation term of this step's loss (unsupervised.py:149) rides on the pass Adam makes over
 * the parameters anyway, instead of a separate unflow_l2_loss launch. */
int unflow_adam_step_regloss(float* p, const float* grad, float* m, float* v, long n, long n_regularized,
                             float grad_scale, float l2_scale, float lr_t, float beta1, float beta2, float eps,
                             float* loss_acc, unflow_stream_t stream);

/* loss_acc[0] += scale * 0.5 * sum(p[0:n]^2)  (tf.nn.l2_loss via slim.l2_regularizer). */
int unflow_l2_loss(const float* p, long n, float scale, float* loss_acc, unflow_stream_t stream);

/* sum/mean helpers for metrics: out[0] = sum(|f1-f2|_2 * mask), out[1] = sum(mask)  (flow_util.py:98-103). */
int unflow_flow_error_sums(const float* f1, const float* f2, const float* mask /* may be NULL = ones */,
                           float* out2, long npix, unflow_stream_t stream);

/* ===================================================================== */
/* forward-only inference (csrc/inference.hip, core/inference.py)          */
/* ===================================================================== */

/* Per-sample geometry of both inference kernels: a DEVICE table desc[B][8] of int32 =
 *   {h, w, y0, x0, nmaps, u8, 0, 0}: the frame's size, its origin in its staging row (may be negative: a frame taller / wider
 *   than the staging buffer was centre-cropped into it), the ground-truth maps staged for it (0..2), and whether its staged
 *   frames are uint8 (1) or fp32 (0) — the same for every sample of a launch.  h = 0: an unused slot of a short batch.
 *   16-byte aligned.  The host rewrites the table between launches; a captured graph keeps its address. */

/* frames [2][B][Hmax][Wmax][3] (uint8 or fp32, [0, 255], per desc u8) -> net_in4 [2B][H][W][4]: rows [0, B) from frame 0
 * (im1), [B, 2B) from frame 1 (im2), each the TF1 legacy bilinear resample of the sample's (h, w) region at (y0, x0) (pixels
 * outside the buffer read zero) to (H, W), then /255 - mean3/255 (unflow_prepare_image_pair's arithmetic; mean3 is a HOST
 * pointer); channel 3 = 0.  A slot with h = 0 writes zeros.  net_pl (may be NULL): the operand planes as in
 * unflow_prepare_image_pair. */
int unflow_inference_input(const void* frames, const int* desc, int B, int Hmax, int Wmax, int H, int W, float* net_in4,
                           const float* mean3, const unflow_planes* net_pl, unflow_stream_t stream);

/* Sequence mode (FlowEstimator(..., sequence=True)), one frame per row: frames [F][Hmax][Wmax][3] (uint8 or fp32 per desc u8),
 * desc [F][8] -> net_in4 [F][H][W][4], row r from frame r with desc slot r.  net_in4 and net_pl point at the FIRST row to write
 * (the estimator passes row 1 of the engine's F + 1 input rows); exactly F rows are written, nothing else.  The value of every
 * pixel and of its operand planes is unflow_inference_input's: a row is bit-identical to the row that entry writes for the
 * same frame and desc.  A slot with h = 0 writes zeros. */
int unflow_inference_input_frames(const void* frames, const int* desc, int F, int Hmax, int Wmax, int H, int W, float* net_in4,
                                  const float* mean3, const unflow_planes* net_pl, unflow_stream_t stream);

/* One buffer of unflow_sequence_carry: sample rows of `pixels` pixels, `stride` bytes apart, starting at base (row 0); of every
 * pixel the first `bytes` bytes are copied (bytes < stride: one channel segment of a wider concat buffer, the other channels
 * are left alone).  base, bytes and stride must be even; 16-byte vector accesses are used where all three are multiples of 16
 * (else 8, 4 or 2 bytes). */
typedef struct {
  void* base;
  long pixels;
  int bytes;
  int stride;
} unflow_carry_buf;
#define UNFLOW_CARRY_MAX 16

/* Sequence mode: in each of the n_bufs (<= UNFLOW_CARRY_MAX) buffers of the HOST array bufs, copy sample row src to row 0, in
 * one launch.  src = *src_row is read from DEVICE memory at run time (an int32 the host rewrites with the desc tables; a
 * captured graph keeps its address): 0 = nothing to carry, a no-op, as is a value outside [1, max_row] (max_row: the last row
 * every buffer has).  Rows other than row 0 are never written. */
int unflow_sequence_carry(const unflow_carry_buf* bufs, int n_bufs, const int* src_row, int max_row, unflow_stream_t stream);

/* Bidirectional sequence mode (FlowEstimator(..., sequence='bidirectional')): in each of the n_bufs (<= UNFLOW_CARRY_MAX)
 * buffers of the HOST array bufs, copy the n consecutive sample rows [src0, src0 + n) to rows [dst0, dst0 + n), in one launch
 * (bytes < stride: one channel segment; the other channels of the destination rows, and every other row, are left alone).  The
 * vector width is chosen per buffer as for unflow_sequence_carry.  max_row: the last row every buffer has.  UNFLOW_ERR_SHAPE,
 * and nothing is launched, when n < 1, a row lies outside [0, max_row] or the two ranges overlap. */
int unflow_sequence_mirror(const unflow_carry_buf* bufs, int n_bufs, int src0, int dst0, int n, int max_row,
                           unflow_stream_t stream);

/* Tracks along a clip (FlowEstimator(..., sequence=True | 'bidirectional', track=...); csrc/track.hip): advance N
 * tracks through the valid pairs of one sequence replay, in slot order, one launch.  A track is a pixel (x, y) of the clip's first
 * frame (its anchor), the displacement disp = (u, v) to where it is now, and alive: still inside the frame and never occluded.
 * flow_fw [B][Hmax][Wmax][2]: the frame-size forward flow per pair slot (unflow_inference_output); occ_fw [B][Hmax][Wmax] uint8
 * (unflow_inference_occlusion's forward mask) or NULL: the one-direction estimator, no track is ever occluded.  tab: the DEVICE
 * int32 tables of the replay (sequence_tables): the pair table [B][8] at word 8B (a slot with h = 0, or with h > Hmax or w > Wmax,
 * is not a pair), the carry source at word 16B, and at words 16B + 2 and 16B + 3 the grid stride S and the number of tracks N —
 * read on the device like the carry source, so a captured graph keeps addresses only.  N above Ncap is clamped to Ncap.
 * Anchors: anchors [N][2] int32 (x, y) in DEVICE memory; or NULL: the dense grid of stride S over a slot's (h, w), track n at
 * (S * (n % gw), S * (n / gw)) with gw = ceil(w / S) (S < 1: nothing is tracked, nothing is written).
 * State, Ncap tracks, kept by the caller from one replay of a clip to the next and updated in place: disp [Ncap][2] fp32, alive
 * [Ncap] uint8.  Carry source 0 (a clip's first replay): every track starts from disp = 0, alive = 1, whatever the state holds,
 * and is then advanced; above 0: from the state.  So the state needs no initialisation, and an estimator's first replay ever,
 * which runs the launch twice with carry source 0 (the eager pass, then the captured graph's first replay), gives what one run
 * gives.  One step, for pair slot i of size (h, w), on an alive track (a dead one keeps disp and alive = 0 for good):
 *   an anchor outside [0, w) x [0, h) ends the track;
 *   t = image_warp's taps of (x, y) displaced by (u, v), clamped to (h, w), rows Wmax apart (csrc/image_warp.h: fp32 floorf);
 *   with occ_fw: occluded — occ[ia], or yw > 0 and occ[ib], or xw > 0 and occ[ic], or xw > 0 and yw > 0 and occ[id], i.e. any tap of
 *     non-zero weight — ends the track where it is: disp is not advanced;
 *   disp += ((wa*a + wb*b) + wc*c) + wd*d per component, a..d slot i's flow at the taps, every product and sum rounded on its own
 *     (unflow_image_warp_fwd's value, then one fp32 add);
 *   the new disp outside the frame ends the track, which keeps that disp: inside iff 0 <= xi and (xi < w - 1 or (xi == w - 1 and
 *     xw == 0)) with xi = x + (int)floorf(u), xw = u - floorf(u), likewise in y — integer decisions; a component that is not
 *     finite or of magnitude >= 1e6 ends it too, tested before any conversion to an integer.
 * After every valid slot i: out_disp[i][n] = disp, out_alive[i][n] = alive ([B][Ncap][2] fp32, [B][Ncap] uint8); slots that are
 * not pairs and rows n >= N are not written.  Tracks are independent and each touches its own state element: deterministic, no
 * atomics.  UNFLOW_ERR_SHAPE, and nothing is launched, for B < 1, Ncap < 1, Hmax or Wmax < 1 or Hmax * Wmax above 2^31 - 1. */
int unflow_sequence_track(const float* flow_fw, const unsigned char* occ_fw, const int* tab, int B, int Hmax, int Wmax,
                          const int* anchors, int Ncap, float* disp, unsigned char* alive, float* out_disp,
                          unsigned char* out_alive, unflow_stream_t stream);

/* Ground truth along a clip (FlowEstimator(..., sequence=..., track=..., ground_truth=True); csrc/track_score.hip):
 * chain the ground-truth flow of the replay's valid pairs into ground-truth tracks, and score this replay's tracks against them,
 * per pair slot, one launch behind unflow_sequence_track.  gt_flow [2][B][Hmax][Wmax][2] fp32 and gt_mask [2][B][Hmax][Wmax] fp32:
 * the staged ground truth of unflow_inference_output, map-major, pair slot i's at [.][i], at the origin.  tab, anchors, Ncap and
 * the track numbering: unflow_sequence_track's; word 4 of a pair's table row is m = nmaps, its number of maps (above 2: 2).
 * out_disp [B][Ncap][2], out_alive [B][Ncap]: what unflow_sequence_track wrote for this replay (read only).
 * State, kept by the caller along a clip and updated in place: gt_disp [Ncap][2] fp32, gt_alive [Ncap] uint8.  Carry source 0
 * starts every ground-truth track from disp = 0, alive = 1, whatever the state holds (unflow_sequence_track's rule).
 * One step, for valid pair slot i, is unflow_sequence_track's step — anchor test, image_warp's taps, any tap of non-zero weight,
 * the fp32 adds rounded one by one, the integer in-frame test, the 1e6 / non-finite rule — with
 *   flow = gt_flow[0][i] (map 0 is the full flow; map 1 is zero under occlusions and is never read);
 *   a tap is "occluded" iff gt_mask[m - 1][i][tap] == 0: with two maps invalid or occluded, with one map invalid;
 *   m < 1 on a valid pair ends every live ground-truth track at that slot (nothing is read).
 * After every valid slot i: out_gt_disp[i][n], out_gt_alive[i][n] ([B][Ncap][2] fp32, [B][Ncap] uint8) for n < N, and the slot's
 * score over the tracks n < N, with (du, dv) = out_disp[i][n] - gt disp (fp32 subtractions) and d2 = du*du + dv*dv, the products
 * and the sum rounded separately; the predicted displacement is used as it is (frozen where that track is dead), a NaN compares
 * false.  scores [B][16] int32, T = {1, 4, 16, 64, 256}:
 *   0 n_gt (ground-truth track alive)   1 n_pred (out_alive)   2 n_both
 *   3..7 within_gt[k]: gt alive and d2 < T[k]            8..12 within_both[k]: both alive and d2 < T[k]
 *   13 n_agree: out_alive == gt alive                    14 N as used (after the clamp to Ncap)        15 0
 * err [B] fp64: the sum over the both-alive tracks of (double)sqrtf(d2), reduced in a fixed order (per-wave cells, per-block
 * partials, the last block found by an integer ticket, a fixed lane-to-partial assignment and a fixed tree; no float atomics):
 * two launches of one grid on the same inputs give the same bytes.  Slots that are not pairs and rows n >= N are not written.
 * workspace: unflow_sequence_track_score_workspace_bytes(B, Ncap) bytes (0 for arguments the entry refuses), 8-byte aligned, ZERO
 * on entry of the first launch; every launch leaves it zero.  UNFLOW_ERR_NULL for a NULL pointer other than anchors;
 * UNFLOW_ERR_SHAPE, and nothing is launched, for what unflow_sequence_track refuses and for B above 512 (the block's LDS). */
size_t unflow_sequence_track_score_workspace_bytes(int B, int Ncap);
int unflow_sequence_track_score(const float* gt_flow, const float* gt_mask, const int* tab, int B, int Hmax, int Wmax,
                                const int* anchors, int Ncap, const float* out_disp, const unsigned char* out_alive,
                                float* gt_disp, unsigned char* gt_alive, float* out_gt_disp, unsigned char* out_gt_alive,
                                int* scores, double* err, void* workspace, unflow_stream_t stream);

/* flow [B][fh][fw][2] (the last network's flow2, or flow0 at (H, W) with full_res) -> for every sample b with desc h > 0 and
 * every frame pixel (y < h, x < w):
 *   f = resize_tf1(resize_tf1(flow, H, W) * flow_scale, h, w) (full_res: resize_tf1(flow * flow_scale, h, w)),
 *   u *= fp32(w / W), v *= fp32(h / H)  (resize_output_flow),
 * bit-identical to unflow_resize_bilinear_tf1(flow, .., H, W, flow_scale) -> unflow_resize_bilinear_tf1(., .., h, w, 1) -> the
 * per-axis multiply.  out_flow [B][Hmax][Wmax][2] (may be NULL) at (b, y, x); out_u16 [B][Hmax][Wmax][3] (may be NULL):
 * uint16(max(0, min(f * 64 + 32768, 65535))) truncated, third channel 1.  gt_flow [2][B][Hmax][Wmax][2] and gt_mask
 * [2][B][Hmax][Wmax] (both NULL: no metrics) staged like the frames (frame pixel (y, x) at (y + y0, x + x0), zero outside);
 * for the desc's nmaps maps k: sums[b][k][0] = sum |gt - f| * m, sums[b][k][1] = sum m (fp64), counts[b][k] = #(|gt - f| * m
 * >= max(3, 0.05 |gt|)).  Fixed-order reduction: partial = B * unflow_inference_output_blocks(Hmax, Wmax) * 6 doubles of
 * scratch, ticket = B zero-initialised uint32 (left zero by every launch). */
int unflow_inference_output_blocks(int Hmax, int Wmax);
int unflow_inference_output(const float* flow, int fh, int fw, float flow_scale, int H, int W, const int* desc, int B, int Hmax,
                            int Wmax, float* out_flow, unsigned short* out_u16, const float* gt_flow, const float* gt_mask,
                            double* partial, unsigned* ticket, double* sums, int* counts, unflow_stream_t stream);

/* flow_fw, flow_bw [B][Hmax][Wmax][2]: the frame-size forward and backward flows of unflow_inference_output -> for every sample b
 * with desc h > 0 and every frame pixel (y < h, x < w), losses.occlusion (losses.py:125-134) in both directions:
 *   bw_warped = image_warp(bw, fw), fw_warped = image_warp(fw, bw)  (clamped to the sample's (h, w), rows Wmax apart),
 *   occ_fw = |fw + bw_warped|^2 > 0.01 (|fw|^2 + |bw|^2) + 0.5, occ_bw likewise with the roles swapped (unwarped magnitudes),
 * every product and sum rounded on its own as the chained torch ops do.  occ_fw / occ_bw uint8 [B][Hmax][Wmax] get 0 / 1 at
 * (b, y, x); nothing else is written.  gt_mask [2][B][Hmax][Wmax] (may be NULL), staged as for unflow_inference_output (map 0:
 * occ, map 1: noc): for a sample with desc nmaps = 2, counts[b] = {TP, FP, FN} of occ_fw over the pixels with mask_occ = 1,
 * positive where mask_noc = 0 (this project's KITTI occlusion scores).  counts [B][3] int32 (required with gt_mask) is zeroed
 * on the stream first (by a one-block launch: no memset node in a captured graph); exact integer sums. */
int unflow_inference_occlusion(const float* flow_fw, const float* flow_bw, const int* desc, int B, int Hmax, int Wmax,
                               const float* gt_mask, unsigned char* occ_fw, unsigned char* occ_bw, int* counts,
                               unflow_stream_t stream);

/* ===================================================================== */
/* flow visualisation (csrc/visual.hip, core/flow_util.py, core/inference.py) */
/* ===================================================================== */

/* Every image is fp32 [..][3] in [0, 1] (out_f32) and / or uint8 (out_u8), at least one of them:
 *   byte = floor(min(max(x * 255, 0), 255) + 0.5), round to nearest, evaluated exactly (fp64) from the fp32 value. */

/* flow_util.py:5-43 on dense tensors: flow [B,H,W,2], mask [B,H,W,1] or NULL (= ones) -> out [B,H,W,3]:
 *   hue = floormod(angle / 2 pi + 1, 1) with the reference's atan2 table (u == 0: +-pi; u == v == 0: hue 0, the pixel is white),
 *   saturation = clip(|flow| * 8 / max_flow, 0, 1) (max_flow == 0: 0), value 1, tf.image.hsv_to_rgb, times mask.
 * max_flow: a HOST pointer to the scale (used as max(max_flow[0], 1)), or NULL: max |flow * mask| over the whole batch, formed on
 * the stream in max_bits (an integer max of bit patterns: exact, order-free): two DEVICE uint32 of scratch, required then,
 * zero-initialised and left zero by every launch. */
int unflow_flow_to_color(const float* flow, const float* mask, const float* max_flow, int B, int H, int W, float* out_f32,
                         unsigned char* out_u8, unsigned* max_bits, unflow_stream_t stream);

/* flow_util.py:46-95: flow_1, flow_2 (the ground truth) [B,H,W,2], mask_occ [B,H,W,1], mask_noc [B,H,W,1] or NULL (= ones).
 * log_colors != 0: error = min(|f1 - f2| / 3, 20 |f1 - f2| / |f2|) (|f2| == 0: the first term) -> the KITTI devkit's ten-bin colour
 * map ([lo, hi) -> rgb / 255; black from 1e9 on), halved where mask_noc == 0, times mask_occ.  log_colors == 0:
 * e = min(|f1 - f2|, 5) / 5 * mask_occ -> (e, e * mask_noc, e * mask_noc). */
int unflow_flow_error_image(const float* flow_1, const float* flow_2, const float* mask_occ, const float* mask_noc, int log_colors,
                            int B, int H, int W, float* out_f32, unsigned char* out_u8, unflow_stream_t stream);

/* The pictures of one inference batch, geometry from desc: frames as for unflow_inference_input, flow [B][Hmax][Wmax][2] the
 * frame-size flow of unflow_inference_output, gt_flow / gt_mask as for unflow_inference_output (both NULL: none).  For every
 * sample b with desc h > 0 and every frame pixel (y < h, x < w), into image k of out [UNFLOW_VISUAL_IMAGES][B][Hmax][Wmax][3]
 * (nothing else is written):
 *   0 overlay            (0.5 im1 + 0.5 im2) / 255, im = the frame resized to (H, W) and back to (h, w) (eval_gui.py:125-134),
 *                        bit-identical to two unflow_resize_bilinear_tf1 launches;
 *   1 brightness error   |im1 - image_warp(im2, flow)| / 255, unflow_image_warp_fwd's taps and tap order;
 *   2 flow colours       flow_to_color(flow), max_flow per sample;
 * and for a sample with desc nmaps > 0 (map 0: flow_occ / mask_occ, map 1: mask_noc; one map: mask_noc = ones):
 *   3 error image        flow_error_image(flow, flow_occ, mask_occ, mask_noc), log colours;
 *   4 gt colours         flow_to_color(flow_occ, mask_occ), max_flow per sample.
 * shown: scratch of 2 * B * Hmax * Wmax * 4 floats (the resized frames, 16-byte aligned); max_bits: 3 * B uint32 of scratch (two
 * maxima per sample, then B tickets), zero-initialised and left zero by every launch (graph replays included: the last block
 * of a sample cleans up, no memset node).  Deterministic: no float atomics. */
#define UNFLOW_VISUAL_IMAGES 5
int unflow_inference_visual(const void* frames, const int* desc, int B, int Hmax, int Wmax, int H, int W, const float* flow,
                            const float* gt_flow, const float* gt_mask, float* shown, unsigned* max_bits, unsigned char* out_u8,
                            float* out_f32, unflow_stream_t stream);

/* The pictures of one sequence replay (FlowEstimator(..., sequence=True | 'bidirectional', visual='sequence')), every frame of the
 * clip resampled once.  frames [B][Hmax][Wmax][3]: the up to B NEW staged frames, as for unflow_inference_input_frames.  tab: the
 * DEVICE int32 tables of the replay (core/inference.py sequence_tables): frame table [B][8] at word 0, pair table [B][8] at
 * word 8B (pair i = engine rows i, i + 1; h = 0: not a pair of the clip), the carry source at word 16B and at word 16B + 1 the
 * bit pattern of a clip-wide max_flow (0: every pair is coloured with its own maximum).  flow_fw [B][Hmax][Wmax][2]: the
 * frame-size flow of unflow_inference_output per pair slot; flow_bw (the backward flow, the same layout) and occ_fw
 * [B][Hmax][Wmax] uint8 (unflow_inference_occlusion's forward mask): both given or both NULL.
 * shown: (B + 1) * Hmax * Wmax * 4 floats, 16-byte aligned, one shown frame (resized to (H, W) and back) per engine row; it must
 * survive from one replay of a clip to the next.  Three launches:
 *   unflow_sequence_carry on shown: row `carry source` (the previous replay's last frame) -> row 0 (0: nothing carried);
 *   a frames kernel: staged frame j (frame-table slot j, h > 0) -> shown row j + 1, unflow_inference_visual's expression, and
 *     max |flow_fw|, max |flow_bw| of pair slot j (not formed with a clip-wide max_flow);
 *   an images kernel: for every pair i with h > 0 and every pixel (y < h, x < w), into image k of out
 *     [UNFLOW_VISUAL_IMAGES][B][Hmax][Wmax][3] (nothing else is written), im1 = shown row i, im2 = shown row i + 1:
 *       0 overlay, 1 brightness error, 2 flow colours of flow_fw: bit-identical to unflow_inference_visual on that pair;
 *     and with flow_bw / occ_fw (without them images 3 and 4 are not written):
 *       3 backward flow colours   flow_to_color(flow_bw), its own maximum per pair (eval_gui.py:166, commented out there);
 *       4 non-occluded brightness error   image 1 where occ_fw == 0, exactly 0 where it is not.
 * The max_flow of images 2 and 3 is the clip-wide one when word 16B + 1 is non-zero.  max_bits: 3 * B uint32 of scratch (the
 * forward and backward maximum per pair slot, then B tickets), zero-initialised and left zero by every launch.  Deterministic:
 * no float atomics.  Hmax * Wmax above 2^31 - 1 (2^28 - 1 for the carry): UNFLOW_ERR_SHAPE. */
int unflow_sequence_visual(const void* frames, const int* tab, int B, int Hmax, int Wmax, int H, int W, const float* flow_fw,
                           const float* flow_bw, const unsigned char* occ_fw, float* shown, unsigned* max_bits,
                           unsigned char* out_u8, float* out_f32, unflow_stream_t stream);

/* In-between frames along a clip (FlowEstimator(..., sequence=True | 'bidirectional', interpolate=n); csrc/interpolate.hip,
 * DESIGN 7.16): n frames, 1 <= n <= 7, between the two frames of every valid pair of one sequence replay, motion-compensated:
 * the colours of frame 0 are splatted forward along the forward flow and, with both directions, those of frame 1 along the
 * backward flow; the sums are normalised by the splatted weight.  This definition is part of the ABI; tests/mid_ref.py mirrors it
 * step by step and the kernels are held to equality.
 * Setting.  tab: the DEVICE int32 tables of the replay (sequence_tables), read on the device, so a captured graph keeps addresses
 * only: frame table [B][8] at word 0, pair table [B][8] at word 8B (a slot with h = 0, or with h > Hmax or w > Wmax, is not a
 * pair; neither is slot 0 while the carry source is 0), the carry source at word 16B.  frames [B][Hmax][Wmax][3]: the up to B NEW
 * staged frames, uint8 or fp32 in [0, 255] per the tables' u8 field, taken as fp32 — the staged frames, not the resampled "shown"
 * ones.  Pair slot i of size (h, w), rows Wmax apart: im0 = staged frame i - 1 (slot 0: prev), im1 = staged frame i, fw =
 * flow_fw[i] ([B][Hmax][Wmax][2], unflow_inference_output).  Both directions: bw = flow_bw[i] and occ_fw / occ_bw [B][Hmax][Wmax]
 * uint8, the two masks of unflow_inference_occlusion; flow_bw, occ_fw, occ_bw are all given or all NULL.  In-between frame j =
 * 1..n is at t = (float)j / (float)(n + 1), with s = (float)(n + 1 - j) / (float)(n + 1), both fp32.
 * Arithmetic.  Every fp32 product and sum is rounded on its own (the library is built with -ffp-contract=off); all weights and all
 * sums are integers.
 * Pass A, for every pixel (x, y) of frame 0:
 *   (u, v) = fw(x, y); a component that is not finite, or of magnitude >= 1e6, contributes nothing — tested before any conversion
 *     to an integer, as unflow_sequence_track does;
 *   c1 = image_warp(im1, fw)(x, y): csrc/image_warp.h's taps, clamped to (h, w), tap order ((wa*a + wb*b) + wc*c) + wd*d;
 *   c = im0(x, y) where occ_fw(x, y) != 0 (both directions only; c1 is then not read), otherwise c = s * im0(x, y) + t * c1;
 *   cq = (long)rintf(min(max(c, 0), 255) * 256) per channel;
 *   px = (float)x + t * u, ix = (int)floorf(px), qx = (int)((px - floorf(px)) * 64), a 6-bit fraction; likewise in y;
 *   the four targets (ix + dx, iy + dy) get the tap weight W = wx * wy * a, wx = 64 - qx for dx = 0 and qx for dx = 1, wy
 *     likewise, a = n + 1 - j; a target outside [0, w) x [0, h), or of weight 0, is dropped — not clamped;
 *   each kept target adds W * cq to its three colour sums and W to its weight sum, 64-bit integers.
 * Pass B, both directions only, for every pixel of frame 1, the roles swapped: (u, v) = bw(x, y); c0 = image_warp(im0, bw)(x, y);
 *   c = im1(x, y) where occ_bw != 0, otherwise s * c0 + t * im1(x, y); position (float)x + s * u; direction weight a = j.
 * Normalise, per target pixel with weight sum Sw and colour sums Sc:
 *   Sw >= 1024: out = (Sc + Sw * 128) / (Sw * 256) by integer division, per channel;
 *   Sw < 1024, a HOLE (less than a quarter of one source pixel's weight in the weaker direction): the temporal blend
 *     ((n + 1 - j) * q(im0) + j * q(im1) + (n + 1) * 128) / ((n + 1) * 256), q the quantisation of cq; it is counted.
 * Outputs: out_mid [n][B][Hmax][Wmax][3] uint8, frame j of pair slot i at [j - 1][i]; out_holes [n][B] int32, the exact number of
 * holes.  Nothing is written for slots that are not pairs, nor outside (h, w).
 * prev [Hmax][Wmax][3] in the staged dtype (Hmax * Wmax * 12 bytes hold either), kept by the caller from one replay of a clip to
 * the next: the host overwrites frames before each replay, so a launch of its own, BEHIND the splat and the normalisation, copies
 * the (h, w) corner of the last frame-table slot with h > 0 into prev.  The copy depends on frames and tab alone, so an estimator's
 * first replay ever, which runs the entry twice (the eager pass, then the captured graph's first replay), gives what one run
 * gives.  prev is never read while the carry source is 0, and needs no initialisation.
 * workspace: unflow_sequence_interpolate_workspace_bytes(n, B, Hmax, Wmax) bytes (0 for arguments the entry refuses), 16-byte
 * aligned: the sums, four 64-bit integers per pixel of out_mid.  Zero on entry and left zero by every launch — the normalisation
 * cleans what it reads, graph replays included, no memset node (the convention of the stream-K flags and max_bits).
 * Deterministic: integer atomics only, no float atomics; the order of arrival cannot change a bit.
 * Known limits: a foreground and a background that collide in a target are averaged, there is no depth order; holes are filled by
 * the temporal blend, not inpainted.
 * UNFLOW_ERR_SHAPE, and nothing is launched, for n outside 1..7, B < 1, Hmax or Wmax < 1, Hmax * Wmax above 2^31 - 1, or flow_bw /
 * occ_fw / occ_bw neither all given nor all NULL. */
size_t unflow_sequence_interpolate_workspace_bytes(int n, int B, int Hmax, int Wmax);
int unflow_sequence_interpolate(const void* frames, const int* tab, int B, int Hmax, int Wmax, int n, const float* flow_fw,
                                const float* flow_bw, const unsigned char* occ_fw, const unsigned char* occ_bw, void* prev,
                                void* workspace, unsigned char* out_mid, int* out_holes, unflow_stream_t stream);

/* In-between frames, consistency-ordered (FlowEstimator(..., interpolate=n, interpolate_order=k); csrc/interpolate.hip, DESIGN
 * 7.19): unflow_sequence_interpolate's arguments, workspace (the same unflow_sequence_interpolate_workspace_bytes, zero on entry,
 * left zero, no memset node), outputs and prev, plus order, 0..4.  order = 0 is unflow_sequence_interpolate, byte for byte.  For
 * order = k >= 1 its definition changes in the places below and nowhere else; this text is part of the ABI,
 * tests/mid_order_ref.py mirrors it step by step and the kernels are held to equality.
 * Per source pixel, passes A and B alike.  here = the pixel's own colour (im0(x, y) in pass A, im1(x, y) in pass B); wp = the
 *   other frame warped by the flow (c1 in pass A, c0 in pass B: the same image_warp taps and tap order);
 *   e = fminf((|here.r - wp.r| + |here.g - wp.g|) + |here.b - wp.b|, 765.f), every fp32 difference, absolute value and sum rounded
 *     on its own; a NaN gives 765, by fminf's rule;
 *   d = min(((int)e) >> (6 - k), 6);  conf = 64 >> d: 64 where the two frames agree along the flow, 1 at the floor.  At k = 1
 *     conf halves per 32 summed grey levels of disagreement, at k = 4 per 4.
 *   A pixel whose occlusion mask is non-zero (both directions): conf = 1 and its own colour; as in unflow_sequence_interpolate its
 *     warp taps are not read.  A pixel with d == 6: its own colour, unblended, as if it were masked.  Every other pixel: the blend
 *     of unflow_sequence_interpolate (s * im0 + t * c1, or s * c0 + t * im1).
 *   Tap weight W = wx * wy * a * conf, the same W into the three colour sums and the weight sum.  The targets, the dropping rule,
 *     the flow test, the 8.8 quantisation and the 6-bit fractions are unflow_sequence_interpolate's.
 * Normalise.  Sw and Sc are the sums of W and W * cq; Sw0 is the sum of the conf-less weights wx * wy * a of the same taps.  A
 *   target is a HOLE iff Sw0 < 1024, so the set of holes is exactly unflow_sequence_interpolate's at every order: a hole is a
 *   target that too little of the source lands on, however well that little agrees (with the test on Sw, which conf lifts up to
 *   64-fold, a sliver of a consistent pixel would close a hole with its colour alone).  Not a hole: out = (Sc + Sw * 128) /
 *   (Sw * 256), as there.  A hole with both directions: the temporal blend, as there.  A hole in one direction: the byte of the
 *   LATER frame, (q(im1) + 128) / 256 — a pixel nothing lands on was uncovered by the motion, and im1 is where it is visible.
 *   Holes are counted as there.
 *   No fifth sum: the weight word of the workspace holds Sw in bits [0, 46) and Sw0 mod 2^18 above them, one atomic add of
 *   W + ((wx * wy * a) << 46) per tap.  Sw0 <= Sw <= 64 Sw0, so Sw < 1024 is a hole and Sw >= 65536 is none whatever the top bits
 *   say, and in between Sw0 <= Sw < 2^16 has not wrapped: the test is exact.  Sw < 2^24 taps * 4096 * 7 * 64 < 2^45.
 * Range.  One tap adds at most 4096 * 7 * 64 * 65280 < 2^37 to a colour sum, and a target gets at most one tap per source pixel
 *   and direction.  With order >= 1 the entry returns UNFLOW_ERR_SHAPE for Hmax * Wmax > 2^23 (tested first, before the NULL
 *   checks): up to 2^26 taps fit a signed 64-bit sum, and a 3840 x 2160 frame passes.
 * The ordered splat reads nothing unflow_sequence_interpolate's does not read.  Deterministic in the same way: integer atomics only.
 * UNFLOW_ERR_SHAPE, and nothing is launched, for order outside 0..4 and for everything unflow_sequence_interpolate refuses. */
int unflow_sequence_interpolate_ordered(const void* frames, const int* tab, int B, int Hmax, int Wmax, int n, const float* flow_fw,
                                        const float* flow_bw, const unsigned char* occ_fw, const unsigned char* occ_bw, void* prev,
                                        void* workspace, unsigned char* out_mid, int* out_holes, int order, unflow_stream_t stream);

/* Held-out scores of the in-between frames (FlowEstimator(..., sequence=..., interpolate=n, held_out=True);
 * csrc/interpolate_score.hip): the frames that unflow_sequence_interpolate made, and two candidates that need no flow,
 * against the frames that were left out of the clip, by squared error and by SSIM.  Launched behind unflow_sequence_interpolate.
 * This definition is part of the ABI; tests/mid_score_ref.py mirrors it.
 * Setting.  frames, tab, B, Hmax, Wmax, n: unflow_sequence_interpolate's.  out_mid [n][B][Hmax][Wmax][3] uint8: what that entry
 * wrote (read only).  truth [n][B][Hmax][Wmax][3] in the staged dtype (the tables' u8 field): truth frame j of pair slot i at
 * [j - 1][i], at the origin, rows Wmax apart.  A pair slot is scored iff it is a pair by unflow_sequence_interpolate's rule AND
 * word 6 of its pair-table row, `held`, is non-zero.  For pair slot i of size (h, w): im0 = staged frame i - 1 (slot 0: this
 * entry's own prev), im1 = staged frame i.
 * Bytes.  q(c) = (long)rintf(min(max(c, 0), 255) * 256) is unflow_sequence_interpolate's quantisation (one definition,
 * csrc/mid_common.h; fminf / fmaxf return their other operand for a NaN, so a NaN colour is 0).  The byte of a staged value is
 * (q(c) + 128) / 256 by integer division — for a uint8 frame the byte itself.  T is the truth's byte.  Three candidates X per (j,
 * slot), kind
 *   0 interpolated  out_mid[j - 1][i];
 *   1 blend         ((n + 1 - j) q(im0) + j q(im1) + 128 (n + 1)) / (256 (n + 1)): what unflow_sequence_interpolate gives a hole;
 *   2 nearest       the byte of im0 where 2 j <= n + 1, else the byte of im1.
 * Scores per (j, slot, kind):
 *   sse   int64, the sum over the h w pixels and 3 channels of (X - T)^2, exact;
 *   ssim  fp64, the sum over the channels and over every 8 x 8 window wholly inside (h, w) — (h - 7)(w - 7) positions, none and
 *         the sum 0 if h < 8 or w < 8 — of the window's SSIM: with the integer window sums Sx, Sy, Sxx, Syy, Sxy (x the
 *         candidate, y the truth), as 64-bit integers vx = 64 Sxx - Sx^2, vy = 64 Syy - Sy^2, cxy = 64 Sxy - Sx Sy, then
 *           a1 = (double)(2 Sx Sy) + c1,  a2 = (double)(2 cxy) + c2,  b1 = (double)(Sx^2 + Sy^2) + c1,  b2 = (double)(vx + vy) + c2,
 *           ssim = (a1 * a2) / (b1 * b2),   c1 = 26634.24 = 4096 (0.01 * 255)^2,  c2 = 239708.16 = 4096 (0.03 * 255)^2,
 *         every fp64 operation rounded on its own (-ffp-contract=off); the integers are below 2^53, their conversions exact.
 * Outputs: out_sse [n][B][3] int64, out_ssim [n][B][3] fp64, (j, slot, kind) at [j - 1][slot][kind].  Nothing is written for a
 * slot that is not scored.  The pixel and window counts are the host's, from (h, w).
 * The fp64 sums are reduced in a fixed order — a thread's terms, a tree per wave, the waves, the block's tiles, per-block partials,
 * an integer ticket, the last block over the partials by a fixed lane assignment and a tree; no float atomics — so two launches and
 * two graph replays give the same bytes.  The integer sums use integer atomics.
 * prev [Hmax][Wmax][3] in the staged dtype (Hmax * Wmax * 12 bytes hold either), this entry's own (unflow_sequence_interpolate has
 * overwritten its prev with this replay's last frame by now), kept by the caller along a clip: a launch behind the scoring one
 * copies the (h, w) corner of the last frame-table slot with h > 0 into it.  It is never read while the carry source is 0 and
 * needs no initialisation.
 * workspace: unflow_sequence_interpolate_score_workspace_bytes(n, B, Hmax, Wmax) bytes (0 for arguments the entry refuses), 8-byte
 * aligned, zero on entry and left zero by every launch (no memset node in a captured graph).
 * UNFLOW_ERR_NULL for a NULL pointer; UNFLOW_ERR_SHAPE, and nothing is launched, for n outside 1..7, B < 1 or above 65535 (the
 * grid's rows), Hmax or Wmax < 1, Hmax * Wmax above 2^31 - 1. */
size_t unflow_sequence_interpolate_score_workspace_bytes(int n, int B, int Hmax, int Wmax);
int unflow_sequence_interpolate_score(const void* frames, const int* tab, int B, int Hmax, int Wmax, int n,
                                      const unsigned char* out_mid, const void* truth, void* prev, void* workspace,
                                      long long* out_sse, double* out_ssim, unflow_stream_t stream);

/* Camera motion along a clip (csrc/stabilise.hip): per valid pair slot i of a sequence replay, of size (h, w), a robust
 * affine fit to the forward flow, the residual of every pixel against it, the camera path composed along the clip and the pair's
 * LATER frame (frame-table slot i of `frames`, uint8 or fp32 per word 5 of the pair row) resampled along that path.  tab: the
 * device tables of the replay (frame table at word 0, pair table at word 8 B, carry source at word 16 B).  A pair slot with h <= 0,
 * w <= 0, h > Hmax or w > Wmax — and slot 0 while the carry source is 0, unflow_sequence_interpolate's rule — is not a pair:
 * nothing is written for it, and nothing outside (h, w) for any slot.
 * Everything is integer but the solve; >> is an arithmetic shift of an int64.
 *   Quantise.  (u, v) = flow_fw[i](x, y).  VALID: both components finite and of magnitude < 4096 (tested before any integer
 *     conversion).  U = rintf(u * 64), V likewise.  X = 2 x - (w - 1), Y = 2 y - (h - 1): half pixels about the frame centre.
 *     ELIGIBLE: valid, and occ_fw NULL or occ_fw[i](x, y) == 0.
 *   Model.  P = {Tu, Lux, Luy, Tv, Lvx, Lvy} int64, T in 2^-16 px, L in 2^-24 per pixel.  pred_u = Tu + ((Lux X + Luy Y + 256) >>
 *     9), r_u = (U << 10) - pred_u, v likewise; e = |r_u| + |r_v|, the L1 residual in 2^-16 px.
 *   Fit.  P = 0, status = 1; iterations r = 0 .. iters (R).  The weight g of an eligible pixel is 1 for r = 0; for r >= 1, with e
 *     under the current P, k_r = max(0, tol - (R - r)), d = min(e >> (17 - k_r), 6), g = d >= 6 ? 0 : 64 >> d.  Others weigh 0.
 *     Thirteen int64 sums over the slot: g, gX, gY, gXX, gXY, gYY, gU, gXU, gYU, gV, gXV, gYV and n = #{g > 0}.  The solve, fp64,
 *     every operation rounded on its own, A the symmetric matrix of the first six sums in the order (1, X, Y): degenerate if n <
 *     16; a00 = A00 must be > 0; m1 = A10 / a00, m2 = A20 / a00; a11 = A11 - m1 A01, a12 = A12 - m1 A02, a22 = A22 - m2 A02; a11
 *     must be > 0; m3 = a12 / a11, a22 = a22 - m3 a12; a22 must be > 0 (a comparison with a NaN is false: degenerate); per right-hand
 *     side (b0, b1, b2) — the U sums, then the V sums — b1' = b1 - m1 b0, b2' = (b2 - m2 b0) - m3 b1', p2 = b2' / a22, p1 = (b1' -
 *     a12 p2) / a11, p0 = ((b0 - A01 p1) - A02 p2) / a00; T = rint(p0 * 1024) clamped to +-2^28, L = rint(p1 * 2^19), rint(p2 *
 *     2^19) clamped to +-2^23 (the clamp: not below the upper limit -> the upper limit, then below the lower -> the lower).  A
 *     degenerate iteration ends the loop and keeps P; a successful one replaces P and sets status = 0.
 *     out_motion[i] = {P[0..5], status | (successful iterations << 8), n of the last successful iteration}.
 *   Path.  D(p) = c + Dt + Dl (p - c) maps stabilised to later-frame coordinates, Dt in 2^-16 px, Dl in 2^-24; the state path[8] =
 *     {Dt_x, Dl_xx, Dl_xy, Dt_y, Dl_yx, Dl_yy, 0, 0} is kept by the caller along a clip and needs no initialisation: with carry
 *     source 0 the clip starts from the identity (Dt = 0, Dl = 2^24 I) whatever it holds (unflow_sequence_track's rule).  Per valid
 *     slot in order, Ml = 2^24 I + L: Dt' = T + ((Ml Dt + 2^23) >> 24), Dl' = (Ml Dl + 2^23) >> 24 (each entry the sum of two
 *     products, then one rounding).  follow = s >= 1: per word, E = D' - identity, D = identity + E - (E >> s); s = 0: D = D' (lock
 *     mode: every frame in the first frame's coordinates).  Dt is clamped to +-2^30, Dl to +-2^26.  out_path[i] = D; after the last
 *     valid slot path = D; a replay without a valid pair leaves path alone.
 *   Residual map.  Under the final P, out_resid = min(255, e >> 14), quarter pixels; an invalid pixel gives 255.
 *   Stabilised frame.  Px = 2 (Dt_x + ((Dl_xx X + Dl_xy Y + 256) >> 9)) + ((w - 1) << 16) in 2^-17 px, Py likewise.  COVERED: 0 <=
 *     Px <= (w - 1) << 17 and the same in y.  ix = Px >> 17, qx = (Px >> 9) & 255, the neighbour min(ix + 1, w - 1); colours in 8.8
 *     fixed point (unflow_sequence_interpolate's rule); byte = (sum of (256 - qx | qx)(256 - qy | qy) colour + 2^23) >> 24.  An
 *     uncovered pixel is (0, 0, 0).
 *   out_counts[i] = {valid, valid but not eligible, eligible with min(e >> (17 - tol), 6) = 6 under the final P, uncovered}.
 * Ranges.  Hmax, Wmax <= 4096: |X|, |Y| < 2^13, g <= 2^6, |U| <= 2^18, so a term is below 2^(6 + 13 + 18) = 2^37 and a sum over
 * 2^24 pixels below 2^61.  |T| <= 2^28, |L| <= 2^23: |L X + L Y + 256| < 2^38, |pred| < 2^30, e < 2^32.  |Ml| < 2^25, |Dt| <= 2^30,
 * |Dl| <= 2^26: a sum of two products is below 2^57.  |Dl X + Dl Y + 256| < 2^41, |Px| < 2^33; a tap sum is below 2^16 2^16 = 2^32.
 * Outputs: out_motion, out_path [B][8] int64, out_resid [B][Hmax][Wmax], out_stab [B][Hmax][Wmax][3], out_counts [B][4].
 * workspace: unflow_sequence_stabilise_workspace_bytes(B) bytes (0 for a B the entry refuses), zero on entry of the first launch
 * and left zero by every launch (no memset node in a captured graph); workspace, path, out_motion, out_path and flow_fw 8-byte aligned
 * (UNFLOW_ERR_UNSUPPORTED otherwise).  The sums use 64-bit integer atomics; no float atomics, no float reductions: two launches and
 * two graph replays give the same bytes.  UNFLOW_ERR_NULL for a NULL pointer other than occ_fw; UNFLOW_ERR_SHAPE for B < 1 or
 * above 65535 (the grid's rows), Hmax or Wmax outside 1..4096, tol or iters outside 0..4, follow outside 0..8.  A refused call
 * launches and writes nothing. */
size_t unflow_sequence_stabilise_workspace_bytes(int B);
int unflow_sequence_stabilise(const void* frames, const int* tab, int B, int Hmax, int Wmax, const float* flow_fw,
                              const unsigned char* occ_fw, int tol, int iters, int follow, long long* path, void* workspace,
                              long long* out_motion, long long* out_path, unsigned char* out_resid, unsigned char* out_stab,
                              int* out_counts, unflow_stream_t stream);

/* Temporal denoising along a clip (csrc/denoise.hip): per valid pair slot i of a bidirectional sequence replay, of size
 * (h, w), the pair's LATER frame averaged with its own history fetched along the backward flow — a recursive, motion-compensated
 * filter.  This definition is part of the ABI; tests/denoise_ref.py mirrors it step by step and the kernels are held to equality.
 * Setting.  frames, tab, B, Hmax, Wmax: unflow_sequence_stabilise's, and so is the pair rule: a pair slot with h <= 0, w <= 0, h >
 *   Hmax or w > Wmax — and slot 0 while the carry source is 0 — is not a pair.  For pair slot i: im1 = staged frame i (frame-table
 *   slot i of `frames`, uint8 or fp32 per word 5 of the pair row), bw = flow_bw[i] ([B][Hmax][Wmax][2], the backward flow on the
 *   later frame's grid), occ = occ_bw[i] ([B][Hmax][Wmax] uint8, unflow_inference_occlusion's backward mask).  All three are
 *   required: the entry has no one-direction form (the history would have to be splatted forward).
 * State.  state [Hmax][Wmax][4] uint16: per pixel the history colour A in 8.8 fixed point (three words, 0..65280) and the history
 *   count n (one word, 1..depth), kept by the caller from one replay of a clip to the next; it needs no initialisation.  With
 *   carry source 0 the clip starts here: before any pair is processed the history is A = q(frame-table slot 0), n = 1 on that
 *   slot's (h, w) (a slot 0 with h <= 0, w <= 0, h > Hmax or w > Wmax initialises nothing), whatever state holds —
 *   unflow_sequence_track's rule, so an estimator's first replay ever, which runs the entry twice (the eager pass, then the
 *   graph's first replay), gives what one run gives.  q is csrc/mid_common.h's quantisation, (long)rintf(min(max(c, 0), 255) *
 *   256).  A slot changes the history on its (h, w) alone.  After the launch state is the history behind the last valid slot; with
 *   carry source 0 and no pair it is the initial history of slot 0; with a carried frame and no pair it is unchanged.
 * Per valid slot in order, per pixel (x, y) of im1 — integers but for the flow test and one rintf per component; / is integer
 * division of non-negative integers, >> a shift of a non-negative integer:
 *   cur = q(im1(x, y)) per channel.  (u, v) = bw(x, y).  VALID: both components finite and of magnitude < 4096, tested before any
 *     conversion.  PX = (x << 6) + (int)rintf(u * 64), PY likewise.  INSIDE: 0 <= PX <= (w - 1) << 6 and the same in y.
 *   FRESH: not VALID, or not INSIDE, or occ(x, y) != 0.  Otherwise: ix = PX >> 6, qx = PX & 63, the neighbour min(ix + 1, w - 1),
 *     the same in y; pred = (sum over the four taps of wx wy A_prev + 2048) >> 12 per channel, wx = 64 - qx | qx, wy likewise;
 *     np = the minimum of the four taps' n_prev, clamped and zero-weight taps included; e = |pred.r - cur.r| + |pred.g - cur.g| +
 *     |pred.b - cur.b|; E = min(e >> 8, 255).
 *   Noise level.  hist: the 256-bin histogram of E over the slot's pixels that are not FRESH, eligible their number.  M = the
 *     smallest m with hist[0] + .. + hist[m] >= (eligible + 1) / 2; M = 0 when eligible = 0.
 *   Tolerance.  t = tol for tol in 0..4; tol = -1 (automatic): the smallest t in 0..4 with (8 << t) >= 2 M, else 4.
 *   Update.  d = min(e >> (11 + t), 6).  neff = 0 for a FRESH pixel and for d == 6 (REJECTED), else np >> d.  A' = (neff pred +
 *     cur + ((neff + 1) >> 1)) / (neff + 1) per channel, n' = min(neff + 1, depth), out_den[i](x, y) = (A' + 128) >> 8 per channel.
 *   A_prev and n_prev are the history BEFORE this slot: the taps are read at displaced positions, so the update is not in place.
 *   The entry keeps two history slabs in its workspace that take turns — slot i reads slab i & 1 and writes the other, pixels
 *   outside (h, w) and slots that are no pairs are copied across — filled from state by a launch in front and copied back to state
 *   by one behind (unflow_sequence_interpolate's prev is kept the same way).
 * Outputs: out_den [B][Hmax][Wmax][3] uint8; out_stats [B][8] int32 = {t, M, eligible, FRESH, REJECTED, the sum of n', 0, 0}.
 * Nothing is written for a slot that is no pair, nor outside (h, w).
 * workspace: unflow_sequence_denoise_workspace_bytes(B, Hmax, Wmax) bytes (0 for arguments the entry refuses), 8-byte aligned:
 *   first B * 256 int32, the histograms — zero on entry of the first launch and left zero by every launch, no memset node in a
 *   captured graph — then the two slabs, [2][Hmax][Wmax] 8-byte words, which need not be zero.  state and flow_bw are 8-byte
 *   aligned too (UNFLOW_ERR_UNSUPPORTED otherwise).
 * Ranges.  |rintf(u * 64)| <= 2^18 and x < 2^12: PX fits an int.  A, pred <= 65280 and neff <= 64 on a state this entry wrote; on
 *   any state the words are below 2^16, a tap sum is below 2^12 2^16 and neff pred + cur + 2^15 below 2^32: unsigned 32-bit
 *   arithmetic is exact.  The sum of n' is at most 64 * 2^24.
 * Integer LDS and global atomics for the histogram and the three counts; no float atomics, no float reductions: two launches and
 * two graph replays give the same bytes.  2 B + 2 launches.
 * UNFLOW_ERR_NULL for any NULL pointer; UNFLOW_ERR_SHAPE for B < 1 or above 65535, Hmax or Wmax outside 1..4096, tol outside
 * -1..4, depth outside 1..64.  A refused call launches and writes nothing. */
size_t unflow_sequence_denoise_workspace_bytes(int B, int Hmax, int Wmax);
int unflow_sequence_denoise(const void* frames, const int* tab, int B, int Hmax, int Wmax, const float* flow_bw,
                            const unsigned char* occ_bw, int tol, int depth, void* state, void* workspace,
                            unsigned char* out_den, int* out_stats, unflow_stream_t stream);

/* ===================================================================== */
/* PNG decode on the device (csrc/png_decode.hip, core/png_device.py)      */
/* ===================================================================== */

/* Per-image geometry of both entries: a DEVICE table desc[n][8] of int64 =
 *   {src, dst, h, w, bpp, sample_bytes, oy, ox}: byte offset of the image's inflated stream in `raw` (h rows of 1 + w * bpp
 *   bytes, the filter byte 0..4 first), byte offset of its decoded bytes in `decoded` (h * w * bpp, tightly packed), its size,
 *   bytes per pixel (1, 2, 3, 4, 6 or 8: 8 / 16-bit grey, grey + alpha, RGB, RGBA), bytes per sample (1 or 2; channels = bpp /
 *   sample_bytes) and the crop origin of unflow_png_to_batch.  unflow_png_unfilter reads the first five fields,
 *   unflow_png_to_batch all but the first.  Images of one launch may differ in every field.  An entry that does not fit its
 *   buffers (or whose crop leaves the frame) is skipped by the kernels; the caller validates the table, and the filter bytes,
 *   on the host (core/png_device.py). */

/* Rows of one image that unflow_png_unfilter decodes together (its skewed wavefront; bands of this many rows run one after
 * another).  Host only. */
int unflow_png_unfilter_rows(void);

/* PNG scanline reconstruction (filters None, Sub, Up, Average, Paeth) of n images in one launch, one workgroup per image:
 * raw [raw_bytes] -> decoded [decoded_bytes], both DEVICE buffers, geometry from desc.  Exact: every byte equals the PNG
 * specification's reconstruction (mod 256, Average on the 9-bit sum, Paeth ties in the order left, up, upper left). */
int unflow_png_unfilter(const unsigned char* raw, long raw_bytes, unsigned char* decoded, long decoded_bytes, const long* desc,
                        int n, unflow_stream_t stream);

/* decoded frames (unflow_png_unfilter's output) -> out [n][H][W][3] fp32: image i is the (H, W) window at (oy, ox) of frame i
 * (zero origin with (H, W) = (h, w): the whole frame) under read_png_image's channel rule — grey is replicated to RGB, alpha is
 * dropped, a 16-bit sample gives its high byte.  mean3 (a HOST pointer, may be NULL = no normalisation): out = (v - mean3[c]) /
 * stddev in fp32 with a correctly rounded division, bit-identical to numpy's float32 (a - mean) / stddev. */
int unflow_png_to_batch(const unsigned char* decoded, long decoded_bytes, const long* desc, int n, int H, int W,
                        const float* mean3, float stddev, float* out, unflow_stream_t stream);

/* The window entries read the same table with oy, ox SIGNED: output pixel (y, x) of image i, y < Hs, x < Ws, is frame pixel
 * (y + oy, x + ox) where that lies inside (h, w) and 0 elsewhere — a crop (oy, ox >= 0), the zero padding of
 * resize_image_with_crop_or_pad (oy = -pad) and any mix of the two per axis.  An entry that does not fit `decoded` (or has
 * the wrong bpp / sample_bytes) is skipped and its output left untouched; the caller validates on the host.
 *
 * unflow_png_to_window: unflow_png_to_batch's channel rule and normalisation on such a window -> out [n][Hs][Ws][3] fp32.  A
 * padded pixel is 0 BEFORE the normalisation (it comes out as (0 - mean3[c]) / stddev), as Input._preprocess_image pads first. */
int unflow_png_to_window(const unsigned char* decoded, long decoded_bytes, const long* desc, int n, int Hs, int Ws,
                         const float* mean3, float stddev, float* out, unflow_stream_t stream);

/* KITTI flow maps, 16-bit RGB only (bpp = 6, sample_bytes = 2): flow [n][Hs][Ws][2] = (u16 - 32768) / 64 of channels 0 and 1,
 * mask [n][Hs][Ws] = float(channel 2) (the raw sample, as read_kitti_flow_png returns it); both exact in fp32.  A padded pixel
 * has flow 0 and mask 0. */
int unflow_png_to_flow_gt(const unsigned char* decoded, long decoded_bytes, const long* desc, int n, int Hs, int Ws, float* flow,
                          float* mask, unflow_stream_t stream);

/* .flo ground truth (csrc/flo_decode.hip): Middlebury / FlyingChairs / Sintel flow files on a window of the same table.  A
 * .flo row has src = the byte offset in `raw` of the file's first float (behind its 12-byte header: h * w pairs of
 * little-endian fp32), bpp = 8 and sample_bytes = 4; dst is unused, and such a row never goes through unflow_png_unfilter.
 * oy, ox are signed as above.  An entry whose src is not a multiple of 4, whose 8 * h * w bytes do not fit raw_bytes, or
 * whose bpp / sample_bytes differ is skipped and its output left untouched; the caller validates on the host.  `raw` itself
 * must be 4-byte aligned.  Plain vector loads and stores; nothing is accumulated.
 *
 * unflow_flo_to_flow_gt — the Middlebury / Chairs rule: flow [n][Hs][Ws][2] holds the file's floats bit for bit (the 1e10
 * "unknown" marker, infinities and NaN payloads are kept), mask [n][Hs][Ws] = (u < 1e9 && v < 1e9) ? 1 : 0 as fp32
 * comparisons (NaN gives 0).  A padded pixel has flow +0 and mask 0. */
int unflow_flo_to_flow_gt(const unsigned char* raw, long raw_bytes, const long* desc, int n, int Hs, int Ws, float* flow,
                          float* mask, unflow_stream_t stream);

/* unflow_sintel_gt — Sintel's composition of a .flo file with its `invalid` and `occlusions` PNGs, fused.  desc holds 3 n rows,
 * column-major: rows [0, n) the .flo files (in `raw`), [n, 2n) the invalid PNGs and [2n, 3n) the occlusion PNGs, both in
 * `decoded` as unflow_png_unfilter leaves them (8 / 16-bit grey, grey + alpha, RGB or RGBA; the sample read is channel 0, a
 * 16-bit sample's high byte).  With inv = sample != 0 and occ = sample != 0 (0 or 1, 0 in the padding):
 *   flow [2][n][Hs][Ws][2]: map 0 (occluded) = the file's floats, map 1 (non-occluded) = flow * (1 - occ), an fp32 product
 *                           (-0 under an occluded negative component);
 *   mask [2][n][Hs][Ws]:    map 0 = 1 - inv, map 1 = (1 - inv) * (1 - occ).
 * The padding is applied before the composition: a padded pixel has flow 0 and both masks 1.  An example with any of its
 * three rows invalid is skipped whole. */
int unflow_sintel_gt(const unsigned char* raw, long raw_bytes, const unsigned char* decoded, long decoded_bytes, const long* desc,
                     int n, int Hs, int Ws, float* flow, float* mask, unflow_stream_t stream);

/* ===================================================================== */
/* PNG encode on the device (csrc/png_encode.hip, core/png_device.py)      */
/* ===================================================================== */

/* A surface says where the raw bytes of a run of images come from, so no staging copy is made: `images` images, image_stride
 * ELEMENTS apart, each an (H, W) allocation of `channels` interleaved samples per pixel with rows row_stride elements apart
 * (row_stride >= W * channels, image_stride >= (H - 1) * row_stride + W * channels).  The image a table entry names sits at
 * the origin of its allocation and may be smaller than (H, W).  kind is the sample:
 *   UNFLOW_PNG_U8     uint8 elements, written as they are (the pictures: 3 channels; bytes per pixel = channels);
 *   UNFLOW_PNG_U8X255 uint8 elements times 255 mod 256 (the occlusion masks: 0 / 1 -> 0 / 255, 1 channel);
 *   UNFLOW_PNG_U16BE  16-bit elements (int16 or uint16 bit patterns; base 2-byte aligned), written high byte first, PNG's
 *                     16-bit samples (out_u16: 3 channels, 6 bytes per pixel). */
#define UNFLOW_PNG_U8 0
#define UNFLOW_PNG_U8X255 1
#define UNFLOW_PNG_U16BE 2
typedef struct {
  const void* base;
  long image_stride;
  long row_stride;
  int images, H, W;
  int channels; /* 1 .. 4 */
  int kind;
} unflow_png_surface;
#define UNFLOW_PNG_SURFACES_MAX 16
#define UNFLOW_PNG_FILTER_FIELDS 8
#define UNFLOW_PNG_FILTER_MAX_ROW_BYTES 32512 /* w * bytes per pixel of one row: two rows of it live in LDS */

/* PNG row filtering of n images in one launch, one workgroup per (image, row): for every entry of the DEVICE table
 * desc[n][UNFLOW_PNG_FILTER_FIELDS] of int64 = {surface, image, h, w, dst, 0, 0, 0} — image `image` of the HOST array
 * surfaces[surface], its top-left (h, w) pixels — the finished scanlines, h rows of 1 + w * bpp bytes with the filter byte first,
 * are written to out[dst ...] (a DEVICE byte buffer of out_bytes).  max_h >= every h and max_row_bytes >= every w * bpp
 * (<= UNFLOW_PNG_FILTER_MAX_ROW_BYTES, else UNFLOW_ERR_UNSUPPORTED).  An entry that does not fit its surface, max_row_bytes
 * or the output buffer is skipped and its bytes left untouched (rows at and beyond max_h are not written); the caller
 * validates the table, and that the ranges do not overlap, on the host (core/png_device.py).  Nothing outside the entries'
 * ranges is written.
 *
 * The filter rule, exact integer work: for a row, the five filtered rows of the PNG specification are formed — 0 None, 1 Sub,
 * 2 Up, 3 Average on the 9-bit sum, 4 Paeth with ties in the order left, up, upper left; a missing neighbour (left of the
 * first pixel, above the first row) is 0.  The cost of a candidate is the sum over its bytes b of (b < 128 ? b : 256 - b); the
 * filter of least cost is chosen, the lowest filter number on a tie.  So an all-zero row gets 0, and a first row where Sub
 * wins gets 1, never 4 (Paeth predicts `left` there).  No float arithmetic and no atomics: bit-reproducible. */
int unflow_png_filter(const unflow_png_surface* surfaces, int n_surfaces, const long* desc, int n, int max_h, int max_row_bytes,
                      unsigned char* out, long out_bytes, unflow_stream_t stream);

/* A non-blocking HIP stream on the current device that belongs to no framework's stream pool (host only, no launch): the
 * loader's side stream, see core/png_device.py::loader_stream.  The caller keeps it for the life of the process. */
int unflow_stream_create(unflow_stream_t* stream);

/* ---- deflate on the device (csrc/deflate.hip; tests/deflate_ref.py is the same rule in Python, equal byte for byte).
 *
 * The stream format, exact integer work.  A stream of `bytes` >= 1 bytes is cut into chunks of chunk_bytes (1 ..
 * UNFLOW_DEFLATE_CHUNK_MAX = 65535, so one stored block always covers a chunk; the last chunk is what is left).  Chunks are coded
 * independently — no match reaches before its chunk's first byte — each as ONE deflate block (RFC 1951), BFINAL set in the last
 * chunk's.  A chunk's segment is formed in three codings and the one of fewest segment BYTES is emitted, the lowest number on a
 * tie:
 *   0  stored: the byte BFINAL, LEN, NLEN, the chunk: 5 + n bytes.  Byte-aligned by itself, so it carries no marker.
 *   1  dynamic Huffman over the literals (and end-of-block) only.
 *   2  dynamic Huffman over literals and distance-1 matches.  A run is a maximal stretch of L bytes that equal their
 *      predecessor (the byte before the run is a literal).  L < 3: literals.  Otherwise L / 258 matches of length 258 from the
 *      run's start, and for the remainder r = L % 258 one match of r if r >= 3, else r literals.  So nothing of a run is lost.
 * A Huffman segment that is not the stream's last ends with the sync-flush marker — the three header bits of an empty stored
 * block, zero bits to the byte boundary, 00 00 FF FF — so segments concatenate without bit shifting; the last ends with zero
 * bits to the byte boundary.
 *
 * Code lengths, for the literal / length alphabet (286 symbols, limit 15) and the code-length alphabet (19 symbols, limit 7):
 * the symbols of non-zero count are sorted by (count, symbol).  One such symbol gets length 1.  Otherwise Moffat and Katajainen's
 * in-place minimum-redundancy construction on the sorted counts (a leaf is taken before an internal node of equal weight) gives
 * the number of leaves per depth; depths above the limit count at the limit; the repair rule: while the Kraft sum exceeds 1, one
 * leaf is taken from the limit's level and the deepest non-empty level below the limit hands one leaf to the next level as two
 * (each round lowers the sum by exactly one unit of 2^-limit).  The levels are then dealt out from the deepest: the least
 * (count, symbol) gets the longest code.  Codes are canonical (RFC 1951 3.2.2).
 *
 * The block header: HLIT = last used literal / length symbol - 256, HDIST = 0 — ONE distance code, of length 1, in both Huffman
 * codings (its code is the bit 0; distance 1 has no extra bits) — HCLEN = the last non-zero entry of the RFC's permuted order,
 * at least 4.  The HLIT + 257 + 1 code lengths are sent with the symbols 0 .. 15, 17 and 18 (never 16): a maximal run of z
 * zero lengths is cut greedily into pieces t = min(z, 138) while z >= 3 — symbol 18 for t >= 11, else 17 — and the 0 .. 2 zeros
 * left are sent as they are.  A Huffman segment therefore carries at most (17 + 57 + 287 * 7 + 15 + 7) / 8 + 5 = 268 bytes
 * beyond its coded literals and matches.
 *
 * The zlib stream is 78 01, the segments, Adler-32 big-endian.  Adler-32 is formed from per-chunk partials a = sum of b[i],
 * b = sum of (n - i) * b[i] (mod 65521), combined in chunk order: B += n * A + b, then A += a, from A = 1, B = 0.
 *
 * unflow_deflate: n streams in one launch pair, one workgroup per (stream, chunk).  DEVICE table desc[n][UNFLOW_DEFLATE_FIELDS]
 * of int64 = {src, bytes, dst, cap, scratch, meta, 0, 0}: the stream in[src .. src + bytes) becomes the zlib stream at
 * out[dst ...], which may take cap >= unflow_deflate_stream_bound(bytes, chunk_bytes) bytes; its size is written to sizes[k]
 * (DEVICE, n int64).  Working memory per stream: chunks * unflow_deflate_slot_bytes(chunk_bytes) bytes of `scratch` from the
 * offset `scratch` (a multiple of 16; the buffer itself 16-byte aligned) and `chunks` entries of `meta`
 * (int[meta_chunks][UNFLOW_DEFLATE_META] = {segment bytes, Adler a, Adler b, coding}) from entry `meta`.  max_chunks >= every
 * stream's chunk count (chunks beyond it are not coded).  An entry that leaves in, out, scratch or meta, or whose cap is below
 * the bound, is skipped and nothing of it is written; the caller validates the table, and that the ranges do not overlap, on
 * the host (core/png_device.py).  Nothing outside the entries' ranges is written; inside [dst, dst + cap) only the stream's
 * own bytes are.  `in` may start at any alignment.  Integer arithmetic, LDS atomic OR / ADD only: bit-reproducible.
 * chunk_bytes outside 1 .. 65535: UNFLOW_ERR_UNSUPPORTED. */
#define UNFLOW_DEFLATE_FIELDS 8
#define UNFLOW_DEFLATE_META 4
#define UNFLOW_DEFLATE_CHUNK_MAX 65535
#define UNFLOW_DEFLATE_CHUNK_DEFAULT 16384 /* DESIGN 7.12 has the A/B */
int unflow_deflate(const unsigned char* in, long in_bytes, const long* desc, int n, int max_chunks, int chunk_bytes,
                   unsigned char* scratch, long scratch_bytes, int* meta, long meta_chunks, unsigned char* out, long out_bytes,
                   long* sizes, unflow_stream_t stream);
/* Host only.  The most bytes a chunk's segment takes (stored: chunk_bytes + 5), the most a stream's zlib stream takes
 * (2 + bytes + 5 * chunks + 4), and the size of a chunk's scratch slot; -1 for arguments out of range. */
long unflow_deflate_segment_bound(int chunk_bytes);
long unflow_deflate_stream_bound(long bytes, int chunk_bytes);
long unflow_deflate_slot_bytes(int chunk_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UNFLOW_HIP_H_ */
