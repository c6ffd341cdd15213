// What the in-between frames (csrc/interpolate.hip) and their held-out scores (csrc/interpolate_score.hip, DESIGN
// 7.18) share, one definition each so that the blend a hole gets and the blend that is scored cannot drift apart: the limits, the
// geometry of a pair slot, the two frames of a pair, the 8.8 quantisation of a colour and the launch that keeps a clip's last frame.
#pragma once
#include <hip/hip_runtime.h>

constexpr int MID_THREADS = 256;
constexpr int MID_MAX = 7;                             // in-between frames per pair

// The geometry of pair slot b of the tables, or h = 0: not a pair of the clip (slot 0 without a carried frame included)
struct MidPair {
  int h, w;
  bool u8;
};
__device__ __forceinline__ MidPair mid_pair(const int* __restrict__ tab, int B, int b, int Hmax, int Wmax) {
  const int* p = tab + 8 * (long)B + 8 * b;
  MidPair d{p[0], p[1], p[5] != 0};
  if (d.h <= 0 || d.w <= 0 || d.h > Hmax || d.w > Wmax || (b == 0 && tab[16 * (long)B] <= 0)) d.h = d.w = 0;
  return d;
}

// 8.8 fixed point of a colour in [0, 255] (a NaN is 0: fmaxf returns its other operand)
__device__ __forceinline__ long long mid_q(float c) { return (long long)rintf(fminf(fmaxf(c, 0.f), 255.f) * 256.f); }

// the two frames of pair slot b: frame 0 is the staged frame b - 1, or prev for slot 0; frame 1 the staged frame b
template <typename T>
__device__ __forceinline__ const T* mid_frame(const void* __restrict__ frames, const void* __restrict__ prev, long plane, int b,
                                              int which) {
  if (which == 0 && b == 0) return reinterpret_cast<const T*>(prev);
  return reinterpret_cast<const T*>(frames) + (long)(b - 1 + which) * plane * 3;
}

static inline bool mid_shape_ok(int n, int B, int Hmax, int Wmax) {
  return n >= 1 && n <= MID_MAX && B >= 1 && B <= 0x7fffffff / 16 && Hmax >= 1 && Wmax >= 1 && (long)Hmax * Wmax <= 0x7fffffffL;
}

namespace {

// the last frame-table slot with h > 0 -> prev, its (h, w) corner; idempotent: it depends on the frames and the tables alone
__global__ __launch_bounds__(MID_THREADS) void mid_prev_kernel(const void* __restrict__ frames, const int* __restrict__ tab, int B,
                                                               int Hmax, int Wmax, void* __restrict__ prev) {
  int k = -1;
  for (int i = 0; i < B; i++)
    if (tab[8 * i] > 0) k = i;
  if (k < 0) return;
  const int h = min(tab[8 * k], Hmax), w = min(max(tab[8 * k + 1], 0), Wmax);
  const bool u8 = tab[8 * k + 5] != 0;
  const long plane = (long)Hmax * Wmax;
  const int npx = h * w;
  for (int p = blockIdx.x * MID_THREADS + threadIdx.x; p < npx; p += gridDim.x * MID_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = ((long)y * Wmax + x) * 3;
    if (u8) {
      const unsigned char* s = reinterpret_cast<const unsigned char*>(frames) + k * plane * 3 + q;
      unsigned char* o = reinterpret_cast<unsigned char*>(prev) + q;
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    } else {
      const float* s = reinterpret_cast<const float*>(frames) + k * plane * 3 + q;
      float* o = reinterpret_cast<float*>(prev) + q;
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
  }
}

}  // namespace
