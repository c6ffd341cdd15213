// .flo ground truth on the device (core/png_device.py): Middlebury / FlyingChairs / Sintel flow files, and Sintel's `invalid`
// and `occlusions` masks, become the evaluation batches' flow and mask maps without a host decode.
//
// A .flo body is h * w little-endian float pairs, so there is nothing to decode: the host reads the body straight into pinned
// staging, one copy brings it to the device, and these kernels cut the window (the table's signed origin: crop, central crop
// and zero padding in one rule, as unflow_png_to_window) and derive the masks.  Both entries read the PNG entries' table
// (include/unflow_hip.h); a .flo row has bpp = 8, sample_bytes = 4 and src = the byte offset of its first float in `raw`.
//
// One thread per output pixel: one 8-byte load of the flow pair (two 4-byte loads when the entry's src is only 4-byte aligned;
// uniform per entry), one 8-byte store per flow map, one 4-byte store per mask; the Sintel entry adds two byte loads (a packed
// PNG's rows start at any address).  Plain C++ loads and stores, no atomics.  Bound by bytes: 8 in and 12 (Middlebury rule) or
// 24 (Sintel) out per pixel.
#include "common.h"

namespace {

constexpr int FLO_DESC = 8;                    // int64 per table entry
constexpr long FLO_MAX_SIDE = 1 << 24;

struct FloWindow {
  const unsigned char* base;                   // h * w float pairs
  long h, w, oy, ox;
  bool pair_aligned;                           // base is 8-byte aligned: one load per pixel
};

// False: the entry is skipped (src misaligned, the body does not fit `raw`, or a field is out of range).
__device__ __forceinline__ bool flo_window_of(const long* d, const unsigned char* raw, long raw_bytes, FloWindow& g) {
  const long src = d[0], h = d[2], w = d[3], bpp = d[4], sb = d[5], oy = d[6], ox = d[7];
  if (h <= 0 || w <= 0 || h > FLO_MAX_SIDE || w > FLO_MAX_SIDE || bpp != 8 || sb != 4) return false;
  if (oy < -FLO_MAX_SIDE || oy > FLO_MAX_SIDE || ox < -FLO_MAX_SIDE || ox > FLO_MAX_SIDE) return false;
  if (src < 0 || (src & 3) != 0 || src > raw_bytes || h * w * 8 > raw_bytes - src) return false;
  g = FloWindow{raw + src, h, w, oy, ox, (reinterpret_cast<uintptr_t>(raw + src) & 7) == 0};
  return true;
}

// The file's pair at window pixel (y, x), bit for bit, or +0 outside the file (`inside` false).
__device__ __forceinline__ float2 flo_pair(const FloWindow& g, unsigned y, unsigned x, bool& inside) {
  const long fy = (long)y + g.oy, fx = (long)x + g.ox;
  inside = fy >= 0 && fy < g.h && fx >= 0 && fx < g.w;
  if (!inside) return make_float2(0.f, 0.f);
  const unsigned char* p = g.base + (fy * g.w + fx) * 8;
  if (g.pair_aligned) return *reinterpret_cast<const float2*>(p);
  const float* q = reinterpret_cast<const float*>(p);
  return make_float2(q[0], q[1]);
}

// The decoded-PNG window of png_decode.hip, restated for the mask rows: 1 to 4 channels of 1 or 2 bytes.
struct MaskWindow {
  const unsigned char* base;
  long h, w, oy, ox;
  int bpp;
};

__device__ __forceinline__ bool mask_window_of(const long* d, const unsigned char* dec, long dec_bytes, MaskWindow& g) {
  const long off = d[1], h = d[2], w = d[3], bpp = d[4], sb = d[5], oy = d[6], ox = d[7];
  if (h <= 0 || w <= 0 || h > FLO_MAX_SIDE || w > FLO_MAX_SIDE || bpp < 1 || bpp > 8 || (sb != 1 && sb != 2) || bpp % sb != 0 ||
      bpp / sb > 4)
    return false;
  if (oy < -FLO_MAX_SIDE || oy > FLO_MAX_SIDE || ox < -FLO_MAX_SIDE || ox > FLO_MAX_SIDE) return false;
  if (off < 0 || off > dec_bytes || h * w * bpp > dec_bytes - off) return false;
  g = MaskWindow{dec + off, h, w, oy, ox, (int)bpp};
  return true;
}

// 1 where channel 0 of the PNG pixel is non-zero (the high byte of a 16-bit sample: the first byte), 0 elsewhere and in the padding.
__device__ __forceinline__ float mask_bit(const MaskWindow& g, unsigned y, unsigned x) {
  const long fy = (long)y + g.oy, fx = (long)x + g.ox;
  if (fy < 0 || fy >= g.h || fx < 0 || fx >= g.w) return 0.f;
  return g.base[(fy * g.w + fx) * g.bpp] != 0 ? 1.f : 0.f;
}

__global__ __launch_bounds__(256) void flo_to_flow_gt_kernel(const unsigned char* __restrict__ raw, long raw_bytes,
                                                             const long* __restrict__ table, int Hs, int Ws,
                                                             float2* __restrict__ flow, float* __restrict__ mask) {
  FloWindow g;
  if (!flo_window_of(table + (long)blockIdx.y * FLO_DESC, raw, raw_bytes, g)) return;
  const unsigned n = (unsigned)Hs * (unsigned)Ws;                   // < 2^31 / 3 (the host checks)
  float2* of = flow + (long)blockIdx.y * n;
  float* om = mask + (long)blockIdx.y * n;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned y = i / (unsigned)Ws, x = i - y * (unsigned)Ws;
    bool inside;
    const float2 f = flo_pair(g, y, x, inside);
    of[i] = f;
    om[i] = (inside && f.x < 1e9f && f.y < 1e9f) ? 1.f : 0.f;     // ordered compares: a NaN component gives 0
  }
}

__global__ __launch_bounds__(256) void sintel_gt_kernel(const unsigned char* __restrict__ raw, long raw_bytes,
                                                        const unsigned char* __restrict__ dec, long dec_bytes,
                                                        const long* __restrict__ table, int nb, int Hs, int Ws,
                                                        float2* __restrict__ flow, float* __restrict__ mask) {
  FloWindow g;
  MaskWindow gi, go;
  const long e = blockIdx.y;
  if (!flo_window_of(table + e * FLO_DESC, raw, raw_bytes, g) ||
      !mask_window_of(table + (nb + e) * FLO_DESC, dec, dec_bytes, gi) ||
      !mask_window_of(table + (2L * nb + e) * FLO_DESC, dec, dec_bytes, go))
    return;
  const unsigned n = (unsigned)Hs * (unsigned)Ws;
  const long map = (long)nb * n;                                    // map 0: occluded, map 1: non-occluded
  float2* f_occ = flow + e * n;
  float2* f_noc = f_occ + map;
  float* m_occ = mask + e * n;
  float* m_noc = m_occ + map;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned y = i / (unsigned)Ws, x = i - y * (unsigned)Ws;
    bool inside;
    const float2 f = flo_pair(g, y, x, inside);
    const float visible = 1.f - mask_bit(go, y, x), valid = 1.f - mask_bit(gi, y, x);
    f_occ[i] = f;
    f_noc[i] = make_float2(f.x * visible, f.y * visible);           // fp32 products: -0 under a negative component, NaN under inf
    m_occ[i] = valid;
    m_noc[i] = valid * visible;
  }
}

bool flo_launch_ok(const void* raw, long raw_bytes, int n, int Hs, int Ws) {
  return n > 0 && n <= 65535 && Hs > 0 && Ws > 0 && raw_bytes > 0 && (long)Hs * Ws * 3 <= 0x7fffffffL &&
         (reinterpret_cast<uintptr_t>(raw) & 3) == 0;
}

}  // namespace

UNFLOW_API int unflow_flo_to_flow_gt(const unsigned char* raw, long raw_bytes, const long* table, int n, int Hs, int Ws,
                                     float* flow, float* mask, unflow_stream_t stream) {
  if (!raw || !table || !flow || !mask) return UNFLOW_ERR_NULL;
  if (!flo_launch_ok(raw, raw_bytes, n, Hs, Ws)) return UNFLOW_ERR_SHAPE;
  const dim3 grid(min(stream_grid((long)Hs * Ws), 256), n);
  flo_to_flow_gt_kernel<<<grid, 256, 0, as_stream(stream)>>>(raw, raw_bytes, table, Hs, Ws, reinterpret_cast<float2*>(flow), mask);
  return launch_status();
}

UNFLOW_API int unflow_sintel_gt(const unsigned char* raw, long raw_bytes, const unsigned char* decoded, long decoded_bytes,
                                const long* table, int n, int Hs, int Ws, float* flow, float* mask, unflow_stream_t stream) {
  if (!raw || !decoded || !table || !flow || !mask) return UNFLOW_ERR_NULL;
  if (!flo_launch_ok(raw, raw_bytes, n, Hs, Ws) || decoded_bytes <= 0) return UNFLOW_ERR_SHAPE;
  const dim3 grid(min(stream_grid((long)Hs * Ws), 256), n);
  sintel_gt_kernel<<<grid, 256, 0, as_stream(stream)>>>(raw, raw_bytes, decoded, decoded_bytes, table, n, Hs, Ws,
                                                        reinterpret_cast<float2*>(flow), mask);
  return launch_status();
}
