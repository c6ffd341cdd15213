// The per-sample geometry table of the inference kernels (desc, include/unflow_hip.h) and the resample of a staged frame onto
// the network's size — one definition for csrc/inference.hip (the input kernel) and csrc/visual.hip (the frames the pictures
// show), so that both read a staged frame with the same taps and the same fp32 expression.
#pragma once
#include <hip/hip_runtime.h>

struct FrameDesc {
  int h, w, y0, x0, nmaps, u8, pad0, pad1;
};

__device__ __forceinline__ FrameDesc load_desc(const int* __restrict__ desc, int b) {
  const int4 a = reinterpret_cast<const int4*>(desc)[2 * b], c = reinterpret_cast<const int4*>(desc)[2 * b + 1];
  return FrameDesc{a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
}

// one staged RGB pixel of frame (fr, b) at staging row / column (r, c); zero outside the buffer
template <typename T>
__device__ __forceinline__ float3 staged_px(const T* __restrict__ base, int Hmax, int Wmax, int r, int c) {
  if (r < 0 || r >= Hmax || c < 0 || c >= Wmax) return make_float3(0.f, 0.f, 0.f);
  const T* p = base + ((long)r * Wmax + c) * 3;
  return make_float3((float)p[0], (float)p[1], (float)p[2]);
}

// resize_input at network pixel (oy, ox): the TF1 legacy bilinear resample of the sample's (h, w) frame region to (H, W) —
// resize_tf1_point's expression, the three channels at once (csrc/resize_tf1.h), values in [0, 255]
template <typename T>
__device__ __forceinline__ float3 frame_resample(const T* __restrict__ base, const FrameDesc& d, int Hmax, int Wmax, int H, int W,
                                                 int oy, int ox) {
  const float sy = (float)d.h / (float)H, sx = (float)d.w / (float)W;
  const float fy = (float)oy * sy, fx = (float)ox * sx;
  const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  const int y1 = min(y0 + 1, d.h - 1), x1 = min(x0 + 1, d.w - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float3 tl = staged_px(base, Hmax, Wmax, y0 + d.y0, x0 + d.x0), tr = staged_px(base, Hmax, Wmax, y0 + d.y0, x1 + d.x0);
  const float3 bl = staged_px(base, Hmax, Wmax, y1 + d.y0, x0 + d.x0), br = staged_px(base, Hmax, Wmax, y1 + d.y0, x1 + d.x0);
  float v[3];
  const float t0[3] = {tl.x, tl.y, tl.z}, t1[3] = {tr.x, tr.y, tr.z}, b0[3] = {bl.x, bl.y, bl.z}, b1[3] = {br.x, br.y, br.z};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float top = t0[c] + (t1[c] - t0[c]) * lx, bot = b0[c] + (b1[c] - b0[c]) * lx;
    v[c] = top + (bot - top) * ly;
  }
  return make_float3(v[0], v[1], v[2]);
}
