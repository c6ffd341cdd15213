// TF1 legacy bilinear resampling (tf.image.resize_bilinear, align_corners=False): src = dst * (in/out); lo = floor(src);
// hi = min(lo+1, in-1); lerp x then y.  One point of one channel, in the fp32 expression order every user shares
// (resize_bilinear_tf1_kernel of csrc/train_misc.hip, the inference output kernel of csrc/inference.hip): the same
// operations in the same order, so that a composed resize is bit-identical to the chained launches.
#pragma once
#include <hip/hip_runtime.h>

// base: channel c of sample b of an [.., H, W, C] tensor (in + b*H*W*C + c); sy = H / OH, sx = W / OW as fp32 quotients.
__device__ __forceinline__ float resize_tf1_point(const float* __restrict__ base, int H, int W, int C, int oy, int ox, float sy,
                                                  float sx) {
  const float fy = (float)oy * sy, fx = (float)ox * sx;
  const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float tl = base[((long)y0 * W + x0) * C], tr = base[((long)y0 * W + x1) * C];
  const float bl = base[((long)y1 * W + x0) * C], br = base[((long)y1 * W + x1) * C];
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  return top + (bot - top) * ly;
}
