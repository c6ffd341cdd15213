// Geometric augmentation of the supervised step for gfx950: the whole network input AND the transformed ground truth of a
// minibatch in one launch.  HBM-bound gather, one thread per output pixel of a sample, grid-stride.
//
// The host passes, per sample, three affine PIXEL maps [3][6] fp32 (core/augment.py::affine_pixel_maps, formed in fp64):
//   M1 = A(theta_global)                  output pixel p -> where frame 1 is read
//   M2 = A(theta_global) A(theta_local)   output pixel p -> where frame 2 is read (ONE resampling through the composed map)
//   M2^-1                                 frame-2 coordinate -> the output pixel that shows it
// A(theta; H, W) is stn_affine_kernel's map of csrc/augment.hip written on pixel coordinates.  A source point s1 = M1 p of
// frame 1 moves to s1 + f(s1) in frame 2, which the augmented second frame shows at q = M2^-1 (s1 + f): the new flow is q - p.
//
//   images      stn_affine_kernel's tap rule (floor, indices clipped BEFORE the weights, its add order) on taps scaled as
//               unflow_prepare_image_pair scales them (v / 255) -> im01 rows b and b + B
//   net input   photometric_augment_kernel's expression on those values, the same draws for both frames, minus mean / 255
//               -> x0 rows b and b + B, pad channels zero: bit-identical to unflow_photometric_augment of im01
//   mode 0      flow = convex bilinear of the four taps at s1, valid = all four taps inside and their masks > 0.5
//   mode 1      flow = the nearest tap floor(s1 + 0.5), valid = inside and its mask > 0.5 (sparse KITTI maps)
//               invalid pixels get flow +0 and mask 0 by SELECTION: the 1e10 markers, infinities and NaNs that the .flo
//               readers keep under mask 0 never reach an output
//
// No atomics, no LDS; plain vector loads and stores (8-byte flow pairs, 16-byte network-input pixels where aligned).
#include "common.h"

namespace {

struct GeoPhoto {
  const float *contrast, *brightness, *colour, *gamma, *noise;
  int n_par;
  float m0, m1, m2;
};

// stn_affine_kernel's taps at the pixel coordinate (x, y) of one [H, W, 3] frame in [0, 255]
__device__ __forceinline__ void geo_image_taps(const float* __restrict__ im, float x, float y, int H, int W, float out[3]) {
  const float Wf = (float)W, Hf = (float)H;
  const float fx = fminf(fmaxf(floorf(x), -4.0f), Wf + 4.0f), fy = fminf(fmaxf(floorf(y), -4.0f), Hf + 4.0f);
  const int x0 = min(max((int)fx, 0), W - 1), x1 = min(max((int)fx + 1, 0), W - 1);
  const int y0 = min(max((int)fy, 0), H - 1), y1 = min(max((int)fy + 1, 0), H - 1);
  const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
  const float wa = (x1f - x) * (y1f - y), wb = (x1f - x) * (y - y0f);
  const float wc = (x - x0f) * (y1f - y), wd = (x - x0f) * (y - y0f);
  const float* pa = im + (size_t)(y0 * W + x0) * 3;
  const float* pb = im + (size_t)(y1 * W + x0) * 3;
  const float* pc = im + (size_t)(y0 * W + x1) * 3;
  const float* pd = im + (size_t)(y1 * W + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; c++)
    out[c] = ((wa * (pa[c] / 255.0f) + wb * (pb[c] / 255.0f)) + wc * (pc[c] / 255.0f)) + wd * (pd[c] / 255.0f);
}

// photometric_augment_kernel's expression for draw s, then the store of one network-input pixel
template <bool X4>
__device__ __forceinline__ void geo_photo_store(const float v3[3], const GeoPhoto& ph, int s, float* __restrict__ o, int ld_out) {
  const float c1 = ph.contrast[s] + 1.0f, br = ph.brightness[s], ginv = 1.0f / ph.gamma[s], nz = ph.noise[s];
  const float mean[3] = {ph.m0, ph.m1, ph.m2};
  float r[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v = (v3[c] * c1 + br) * ph.colour[3 * s + c];
    v = fmaxf(0.0f, fminf(1.0f, v));
    v = powf(v, ginv);
    r[c] = (v + nz) - mean[c];
  }
  if (X4) {
    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], 0.f);
  } else {
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
    for (int c = 3; c < ld_out; c++) o[c] = 0.f;
  }
}

template <bool F8>
__device__ __forceinline__ float2 load_flow(const float* __restrict__ p) {
  if (F8) return *reinterpret_cast<const float2*>(p);
  return make_float2(p[0], p[1]);
}

// F8: the flow pointers are 8-byte aligned; X4: ld_out == 4 and x0 is 16-byte aligned
template <bool F8, bool X4>
__global__ __launch_bounds__(256) void supervised_geo_augment_kernel(
    const float* __restrict__ im1, const float* __restrict__ im2, const float* __restrict__ flow_gt,
    const float* __restrict__ mask_gt, const float* __restrict__ mats, GeoPhoto ph, float* __restrict__ im01,
    float* __restrict__ x0, int ld_out, float* __restrict__ flow_out, float* __restrict__ mask_out, int mode, int B, int H,
    int W) {
  const unsigned npx = (unsigned)B * H * W;
  const size_t frame = (size_t)H * W;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
    const Pix pp = decode_pix(i, W, H);
    const float* m = mats + (size_t)pp.n * 18;
    const float px = (float)pp.x, py = (float)pp.y;
    const float s1x = (m[0] * px + m[1] * py) + m[2], s1y = (m[3] * px + m[4] * py) + m[5];
    const float s2x = (m[6] * px + m[7] * py) + m[8], s2y = (m[9] * px + m[10] * py) + m[11];
    const size_t i2 = (size_t)i + (size_t)B * frame;         // the same pixel of row b + B

    // ---- images and network input
    float g1[3], g2[3];
    geo_image_taps(im1 + (size_t)pp.n * frame * 3, s1x, s1y, H, W, g1);
    geo_image_taps(im2 + (size_t)pp.n * frame * 3, s2x, s2y, H, W, g2);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      im01[(size_t)i * 3 + c] = g1[c];
      im01[i2 * 3 + c] = g2[c];
    }
    geo_photo_store<X4>(g1, ph, pp.n % ph.n_par, x0 + (size_t)i * ld_out, ld_out);
    geo_photo_store<X4>(g2, ph, (pp.n + B) % ph.n_par, x0 + i2 * ld_out, ld_out);

    // ---- ground truth
    const float* fb = flow_gt + (size_t)pp.n * frame * 2;
    const float* mb = mask_gt ? mask_gt + (size_t)pp.n * frame : nullptr;
    bool valid;
    float fu = 0.f, fv = 0.f;
    if (mode == 0) {
      const float fx = floorf(s1x), fy = floorf(s1y);
      valid = fx >= 0.0f && fx + 1.0f <= (float)(W - 1) && fy >= 0.0f && fy + 1.0f <= (float)(H - 1);
      if (valid) {        // all four taps lie inside: the loads are in bounds
        const size_t a = (size_t)((int)fy * W + (int)fx);
        if (mb) valid = mb[a] > 0.5f && mb[a + 1] > 0.5f && mb[a + W] > 0.5f && mb[a + W + 1] > 0.5f;
        const float2 t00 = load_flow<F8>(fb + a * 2), t01 = load_flow<F8>(fb + (a + 1) * 2);
        const float2 t10 = load_flow<F8>(fb + (a + W) * 2), t11 = load_flow<F8>(fb + (a + W + 1) * 2);
        const float ax = s1x - fx, ay = s1y - fy;
        const float u0 = t00.x + (t01.x - t00.x) * ax, u1 = t10.x + (t11.x - t10.x) * ax;
        const float v0 = t00.y + (t01.y - t00.y) * ax, v1 = t10.y + (t11.y - t10.y) * ax;
        fu = u0 + (u1 - u0) * ay;
        fv = v0 + (v1 - v0) * ay;
      }
    } else {
      const float rx = floorf(s1x + 0.5f), ry = floorf(s1y + 0.5f);
      valid = rx >= 0.0f && rx <= (float)(W - 1) && ry >= 0.0f && ry <= (float)(H - 1);
      if (valid) {
        const size_t a = (size_t)((int)ry * W + (int)rx);
        if (mb) valid = mb[a] > 0.5f;
        const float2 t = load_flow<F8>(fb + a * 2);
        fu = t.x;
        fv = t.y;
      }
    }
    const float tx = s1x + fu, ty = s1y + fv;
    const float qx = (m[12] * tx + m[13] * ty) + m[14], qy = (m[15] * tx + m[16] * ty) + m[17];
    // selection, not multiplication: whatever sits under an invalid tap (1e10, inf, NaN) stays out of the outputs
    const float ou = valid ? qx - px : 0.f, ov = valid ? qy - py : 0.f;
    if (F8) {
      *reinterpret_cast<float2*>(flow_out + (size_t)i * 2) = make_float2(ou, ov);
    } else {
      flow_out[(size_t)i * 2] = ou;
      flow_out[(size_t)i * 2 + 1] = ov;
    }
    mask_out[i] = valid ? 1.f : 0.f;
  }
}

}  // namespace

UNFLOW_API int unflow_supervised_geo_augment(const float* im1, const float* im2, const float* flow_gt, const float* mask_gt,
                                             const float* mats, const float* contrast, const float* brightness,
                                             const float* colour3, const float* gamma, const float* noise, int n_par,
                                             const float* mean3, float* im01, float* x0, int ld_out, float* flow_out,
                                             float* mask_out, int mode, int B, int H, int W, unflow_stream_t stream) {
  if (!im1 || !im2 || !flow_gt || !mats || !contrast || !brightness || !colour3 || !gamma || !noise || !im01 || !x0 ||
      !flow_out || !mask_out)
    return UNFLOW_ERR_NULL;
  if (B < 0 || H <= 0 || W <= 0 || ld_out < 3 || n_par <= 0) return UNFLOW_ERR_SHAPE;
  if (mode != 0 && mode != 1) return UNFLOW_ERR_UNSUPPORTED;
  // a gather: the sources are read while the targets are written, so they must be different buffers
  if (flow_gt == flow_out || mask_gt == mask_out || im1 == im01 || im2 == im01) return UNFLOW_ERR_UNSUPPORTED;
  const long npx = (long)B * H * W;
  if (npx == 0) return UNFLOW_OK;
  if (2 * npx > 0x7fffffffL) return UNFLOW_ERR_UNSUPPORTED;
  GeoPhoto ph{contrast, brightness, colour3, gamma, noise, n_par, mean3 ? mean3[0] / 255.0f : 0.f,
              mean3 ? mean3[1] / 255.0f : 0.f, mean3 ? mean3[2] / 255.0f : 0.f};        // mean3: HOST pointer or NULL
  const bool f8 = ((reinterpret_cast<uintptr_t>(flow_gt) | reinterpret_cast<uintptr_t>(flow_out)) & 7) == 0;
  const bool x4 = ld_out == 4 && (reinterpret_cast<uintptr_t>(x0) & 15) == 0;
  const int grid = stream_grid(npx);
#define GEO_LAUNCH(F8, X4)                                                                                                  \
  supervised_geo_augment_kernel<F8, X4><<<grid, 256, 0, as_stream(stream)>>>(im1, im2, flow_gt, mask_gt, mats, ph, im01, x0, \
                                                                             ld_out, flow_out, mask_out, mode, B, H, W)
  if (f8 && x4) GEO_LAUNCH(true, true);
  else if (f8) GEO_LAUNCH(true, false);
  else if (x4) GEO_LAUNCH(false, true);
  else GEO_LAUNCH(false, false);
#undef GEO_LAUNCH
  return launch_status();
}
