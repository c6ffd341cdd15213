// TEST INFRASTRUCTURE ONLY.  A C ABI over the seven GPU entry points of the reference's custom ops, compiled UNMODIFIED from the
// reference checkout for gfx950 (oracle/Makefile, target _ref/libref_ops.so) with the stand-in headers of oracle/ref_shim/.
// tests/test_reference_kernels_gpu.py runs these next to the CPU oracle (oracle/ops_ref.c) and the library's own kernels.
//
// The reference kernels check no bounds, so every entry validates sizes and geometry on the host and returns a status without
// launching when something does not fit.  Every entry takes DEVICE pointers, synchronises the device before and after (the
// reference's correlation launches on the null stream), and is as slow as that sounds.
//
// Correlation geometry is never restated here: CorrelationState, the reference's own constructor, computes it.
#include <hip/hip_runtime.h>

#include <tensorflow/core/framework/tensor_types.h>
#include <tensorflow/core/framework/op_kernel.h>
#include <correlation_op.h>

typedef Eigen::GpuDevice Dev;
typedef tensorflow::TTypes<float, 4>::Tensor Out4;
typedef tensorflow::TTypes<float, 4>::ConstTensor In4;

// defined in the reference's ops/*_op.cu.cc
void Correlation(const Dev&, In4, In4, Out4, Out4, Out4, CorrelationState);
void CorrelationGrad(const Dev&, In4, In4, In4, Out4, Out4, CorrelationState);
void BackwardWarp(const Dev&, In4, In4, Out4);
void BackwardWarpGrad(const Dev&, In4, In4, In4, Out4);
void ForwardWarp(const Dev&, In4, Out4);
void ForwardWarpGrad(const Dev&, In4, In4, Out4);
void Downsample(const Dev&, In4, Out4);

#define GLUE_OK 0
#define GLUE_NULL (-1)      // a null pointer
#define GLUE_ATTR (-2)      // a non-positive size, an even kernel, a stride or attribute out of range
#define GLUE_SIZE (-3)      // a buffer's element count is not what the geometry asks for
#define GLUE_GEOMETRY (-4)  // the kernels would index outside a buffer (or past 2^31, or past the launch limits)
#define GLUE_HIP (-5)       // the HIP runtime reported an error

namespace {

const long kIntMax = 2147483647L;

In4 view_in(const float* p, long a, long b, long c, long d) { return In4{p, {a, b, c, d}}; }
Out4 view_out(float* p, long a, long b, long c, long d) { return Out4{p, {a, b, c, d}}; }

int device_quiet() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? GLUE_OK : GLUE_HIP; }

struct CorrPlan {
  int status;
  CorrelationState st;
  long out_elems, padded_elems, in_elems;
};

// Attributes -> the reference's own state, plus every condition under which its kernels stay inside their buffers:
//  forward   reads padded rows  md - r*s2 .. md + (oh-1)*s1 + r*s2 + k - 1   (CorrelateData's y1, y2 + j), same for columns;
//  gradient  reads padded rows  pad - r*s2 .. pad + H - 1 + r*s2             (Backward0 / Backward1's m +- s2p), same for columns;
//  one block per output pixel and sample, k*k*C floats of dynamic LDS, all flat indices in int.
CorrPlan corr_plan(int B, int C, int H, int W, int k, int md, int pad, int s1, int s2, bool grad) {
  const bool bad = B <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || k % 2 == 0 || md < 0 || pad < 0 || s1 <= 0 || s2 <= 0 ||
                   s1 > 1000 || H > 30000 || W > 30000 || md > 30000 || pad > 30000 || k > 255;
  CorrelationAttrs at;
  at.kernel_size = k; at.max_displacement = md; at.pad_size = pad; at.stride_1 = s1; at.stride_2 = s2;
  if (bad) {  // the state of a harmless configuration: the constructor divides by the strides
    at.kernel_size = 1; at.max_displacement = 0; at.pad_size = 0; at.stride_1 = 1; at.stride_2 = 1;
  }
  CorrPlan p{bad ? GLUE_ATTR : GLUE_OK, bad ? CorrelationState(at, 1, 1, 1) : CorrelationState(at, H, W, C), 0, 0, 0};
  if (bad) return p;
  const CorrelationState& s = p.st;
  if (s.out_height <= 0 || s.out_width <= 0 || s.out_channels <= 0) { p.status = GLUE_ATTR; return p; }
  p.in_elems = (long)B * C * H * W;
  p.out_elems = (long)B * s.out_channels * s.out_height * s.out_width;
  p.padded_elems = (long)B * s.padded_height * s.padded_width * C;
  const int reach = s.neighborhood_grid_radius * s2;
  const bool fwd_inside = md - reach >= 0 && md + (s.out_height - 1) * s1 + reach + k - 1 < s.padded_height &&
                          md + (s.out_width - 1) * s1 + reach + k - 1 < s.padded_width;
  const bool grad_inside = pad - reach >= 0;
  const bool launchable = s.out_width <= 65535 && s.out_height <= 65535 && B <= 65535 && C <= 65535 &&
                          (long)k * k * C * (long)sizeof(float) <= 48 * 1024 && p.in_elems <= kIntMax && p.out_elems <= kIntMax &&
                          p.padded_elems <= kIntMax;
  if (!fwd_inside || (grad && !grad_inside) || !launchable) p.status = GLUE_GEOMETRY;
  return p;
}

int warp_sizes_ok(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return GLUE_ATTR;
  if ((long)B * H * W * (C > 2 ? C : 2) > kIntMax) return GLUE_GEOMETRY;
  return GLUE_OK;
}

}  // namespace

extern "C" {

// shape5 (may be NULL) receives {out_channels, out_height, out_width, padded_height, padded_width} of CorrelationState.
// With out == NULL the call only reports the shape.  in0 / in1 / out NCHW; padded0 / padded1 [B, ph, pw, C], written here and
// read by ref_glue_correlation_grad.
__attribute__((visibility("default"))) int ref_glue_correlation(
    const float* in0, const float* in1, float* out, float* padded0, float* padded1, long out_elems, long padded_elems, int B,
    int C, int H, int W, int kernel_size, int max_displacement, int pad, int stride_1, int stride_2, int* shape5) {
  const CorrPlan p = corr_plan(B, C, H, W, kernel_size, max_displacement, pad, stride_1, stride_2, false);
  if (p.status == GLUE_ATTR) return p.status;
  if (shape5) {
    shape5[0] = p.st.out_channels; shape5[1] = p.st.out_height; shape5[2] = p.st.out_width;
    shape5[3] = p.st.padded_height; shape5[4] = p.st.padded_width;
  }
  if (p.status != GLUE_OK) return p.status;
  if (!out) return GLUE_OK;
  if (!in0 || !in1 || !padded0 || !padded1) return GLUE_NULL;
  if (out_elems != p.out_elems || padded_elems != p.padded_elems) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  const CorrelationState& s = p.st;
  Correlation(Dev{nullptr}, view_in(in0, B, C, H, W), view_in(in1, B, C, H, W),
              view_out(out, B, s.out_channels, s.out_height, s.out_width),
              view_out(padded0, B, s.padded_height, s.padded_width, C), view_out(padded1, B, s.padded_height, s.padded_width, C), s);
  return device_quiet();
}

// dout NCHW [B, oc, oh, ow]; padded0 / padded1 as ref_glue_correlation left them; grad0 / grad1 NCHW [B, C, H, W].
__attribute__((visibility("default"))) int ref_glue_correlation_grad(
    const float* dout, const float* padded0, const float* padded1, float* grad0, float* grad1, long dout_elems,
    long padded_elems, long grad_elems, int B, int C, int H, int W, int kernel_size, int max_displacement, int pad, int stride_1,
    int stride_2) {
  const CorrPlan p = corr_plan(B, C, H, W, kernel_size, max_displacement, pad, stride_1, stride_2, true);
  if (p.status != GLUE_OK) return p.status;
  if (!dout || !padded0 || !padded1 || !grad0 || !grad1) return GLUE_NULL;
  if (dout_elems != p.out_elems || padded_elems != p.padded_elems || grad_elems != p.in_elems) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  const CorrelationState& s = p.st;
  CorrelationGrad(Dev{nullptr}, view_in(dout, B, s.out_channels, s.out_height, s.out_width),
                  view_in(padded0, B, s.padded_height, s.padded_width, C), view_in(padded1, B, s.padded_height, s.padded_width, C),
                  view_out(grad0, B, C, H, W), view_out(grad1, B, C, H, W), s);
  return device_quiet();
}

// images / out [B, H, W, C], flows [B, H, W, 2]
__attribute__((visibility("default"))) int ref_glue_backward_warp(const float* images, const float* flows, float* out,
                                                                  long image_elems, long flow_elems, int B, int H, int W, int C) {
  const int ok = warp_sizes_ok(B, H, W, C);
  if (ok != GLUE_OK) return ok;
  if (!images || !flows || !out) return GLUE_NULL;
  if (image_elems != (long)B * H * W * C || flow_elems != (long)B * H * W * 2) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  BackwardWarp(Dev{nullptr}, view_in(images, B, H, W, C), view_in(flows, B, H, W, 2), view_out(out, B, H, W, C));
  return device_quiet();
}

// dout / images [B, H, W, C], flows / dflows [B, H, W, 2]
__attribute__((visibility("default"))) int ref_glue_backward_warp_grad(const float* dout, const float* images, const float* flows,
                                                                       float* dflows, long image_elems, long flow_elems, int B,
                                                                       int H, int W, int C) {
  const int ok = warp_sizes_ok(B, H, W, C);
  if (ok != GLUE_OK) return ok;
  if (!dout || !images || !flows || !dflows) return GLUE_NULL;
  if (image_elems != (long)B * H * W * C || flow_elems != (long)B * H * W * 2) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  BackwardWarpGrad(Dev{nullptr}, view_in(dout, B, H, W, C), view_in(images, B, H, W, C), view_in(flows, B, H, W, 2),
                   view_out(dflows, B, H, W, 2));
  return device_quiet();
}

// flows [B, H, W, 2], out [B, H, W, 1]
__attribute__((visibility("default"))) int ref_glue_forward_warp(const float* flows, float* out, long flow_elems, long out_elems,
                                                                 int B, int H, int W) {
  const int ok = warp_sizes_ok(B, H, W, 1);
  if (ok != GLUE_OK) return ok;
  if (!flows || !out) return GLUE_NULL;
  if (flow_elems != (long)B * H * W * 2 || out_elems != (long)B * H * W) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  ForwardWarp(Dev{nullptr}, view_in(flows, B, H, W, 2), view_out(out, B, H, W, 1));
  return device_quiet();
}

// dout [B, H, W, 1], flows / dflows [B, H, W, 2]
__attribute__((visibility("default"))) int ref_glue_forward_warp_grad(const float* dout, const float* flows, float* dflows,
                                                                      long dout_elems, long flow_elems, int B, int H, int W) {
  const int ok = warp_sizes_ok(B, H, W, 1);
  if (ok != GLUE_OK) return ok;
  if (!dout || !flows || !dflows) return GLUE_NULL;
  if (flow_elems != (long)B * H * W * 2 || dout_elems != (long)B * H * W) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  ForwardWarpGrad(Dev{nullptr}, view_in(dout, B, H, W, 1), view_in(flows, B, H, W, 2), view_out(dflows, B, H, W, 2));
  return device_quiet();
}

// images [B, H, W, C] -> out [B, H / scale, W / scale, C]; the reference's op refuses sizes that scale does not divide
__attribute__((visibility("default"))) int ref_glue_downsample(const float* images, float* out, long image_elems, long out_elems,
                                                               int B, int H, int W, int C, int scale) {
  const int ok = warp_sizes_ok(B, H, W, C);
  if (ok != GLUE_OK) return ok;
  if (scale <= 0 || H % scale != 0 || W % scale != 0) return GLUE_ATTR;
  if (!images || !out) return GLUE_NULL;
  const int oh = H / scale, ow = W / scale;
  if (image_elems != (long)B * H * W * C || out_elems != (long)B * oh * ow * C) return GLUE_SIZE;
  if (device_quiet() != GLUE_OK) return GLUE_HIP;
  Downsample(Dev{nullptr}, view_in(images, B, H, W, C), view_out(out, B, oh, ow, C));
  return device_quiet();
}

}  // extern "C"
