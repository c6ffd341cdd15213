// image_warp's bilinear taps (src/e2eflow/core/image_warp.py:4-76): clamp-to-edge, x + int(floor(u)).  One definition for every
// user — the image_warp kernels of csrc/ops_warp.hip and the occlusion kernel of csrc/inference.hip — so that a warped value
// formed with the tap order ((wa*a + wb*b) + wc*c) + wd*d is bit-identical between them.
#pragma once
#include <hip/hip_runtime.h>

struct IwTaps {
  long ia, ib, ic, id;  // pixel indices within the sample (sample-relative, in pixels)
  float xw, yw, wa, wb, wc, wd;
};

// The taps of pixel (px, py) displaced by (u, v), clamped to an H x W image whose rows are ld pixels apart.
__device__ __forceinline__ IwTaps iw_sample(int px, int py, float u, float v, int H, int W, int ld) {
  IwTaps t;
  const float fu = floorf(u), fv = floorf(v);
  t.xw = u - fu;
  t.yw = v - fv;
  t.wa = (1.f - t.xw) * (1.f - t.yw);
  t.wb = (1.f - t.xw) * t.yw;
  t.wc = t.xw * (1.f - t.yw);
  t.wd = t.xw * t.yw;
  const int xi = px + (int)fu, yi = py + (int)fv;
  const int x0 = min(max(xi, 0), W - 1), x1 = min(max(xi + 1, 0), W - 1);
  const int y0 = min(max(yi, 0), H - 1), y1 = min(max(yi + 1, 0), H - 1);
  t.ia = (long)y0 * ld + x0;
  t.ib = (long)y1 * ld + x0;
  t.ic = (long)y0 * ld + x1;
  t.id = (long)y1 * ld + x1;
  return t;
}

// A dense H x W image (row stride W).
__device__ __forceinline__ IwTaps iw_sample(int px, int py, float u, float v, int H, int W) {
  return iw_sample(px, py, u, v, H, W, W);
}
