// Flow visualisation (core/flow_util.py flow_to_color / flow_error_image, core/inference.py FlowEstimator(visual=True)): the
// pictures of the reference's eval_gui.py (:133-142, :160-204) and flow_util.py (:5-95) as memory-bound kernels.
//
// Operator form, dense [B,H,W,*] tensors: unflow_flow_to_color (batch-wide max_flow, as the reference) and
// unflow_flow_error_image.  Estimator form, unflow_inference_visual: geometry from the device desc table (csrc/frame_desc.h), so
// the one captured graph serves mixed frame sizes and a short last batch; two kernels on the grid of the output kernel:
//   visual_frames_kernel   staged frames -> the frames the reference shows: resize_input to (H, W), resize_output back to (h, w),
//                          composed per pixel (each of the four corners of the second resize is formed from the staged frame
//                          with csrc/frame_desc.h's expression: bit-identical to two unflow_resize_bilinear_tf1 launches),
//                          kept as float4 rows [2][B][Hmax][Wmax] for the warp taps; and max |flow|, max |gt * mask| per sample
//   visual_images_kernel   overlay, brightness error (image_warp's taps and tap order, csrc/image_warp.h), flow colours, and with
//                          ground truth the KITTI error image and the ground truth's colours -> uint8 (and optionally fp32)
// Sequence form, unflow_sequence_visual (FlowEstimator(..., sequence=..., visual='sequence')): the same pictures along a clip, driven by
// the frame table, the pair table and the carry source of a sequence replay; a shown frame per engine row, [B + 1][Hmax][Wmax]:
//   unflow_sequence_carry           shown row src (the previous replay's last frame) -> row 0
//   sequence_visual_frames_kernel   staged frame j -> shown row j + 1 (every frame of the clip resampled once), the maxima of pair j
//   sequence_visual_images_kernel   pair i = (row i, row i + 1): visual_images_kernel's three pictures, and with the backward flow
//                                   and the forward occlusion mask its colours and the brightness error of the non-occluded pixels
// max of non-negative floats = unsigned max of their bit patterns: an integer atomicMax, exact and independent of the order.
// The slots clean themselves: every block of the kernel that reads a maximum takes an integer ticket when it is done, and the
// last one zeroes the slot and the ticket for the next launch (graph replays included), as inference_output_kernel's ticket
// does — no memset node in a captured graph.  No float atomics: results are the same from run to run and between graph replay
// and eager launches.
// 8-bit values: floor(min(max(x * 255, 0), 255) + 0.5) evaluated in fp64, where the product of an fp32 value and 255 is exact —
// the byte is the exact round-half-up of the fp32 image value (an fp32 product could land on a half level it did not reach).
#include "common.h"
#include "frame_desc.h"
#include "image_warp.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int N_IMAGES = 5;                            // overlay, brightness error, flow colours, error image, gt colours
constexpr float PI_F = 3.14159265358979323846f;

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

__device__ __forceinline__ unsigned char to_byte(float x) {
  return (unsigned char)floor(fmin(fmax((double)x * 255.0, 0.0), 255.0) + 0.5);
}

// flow_util.py:5-43.  The reference's own atan2 table: u == 0 gives +-pi (not +-pi/2); u == v == 0 (NaN there): hue 0, and its
// saturation is 0, so the pixel is white.  max_flow == 0 (an all-zero field, NaN there): saturation 0.
__device__ __forceinline__ float3 wheel_color(float u, float v, float m, float max_flow) {
  const float mag = sqrtf(u * u + v * v);
  float angle = 0.f;
  if (u > 0.f) angle = atanf(v / u);
  else if (u < 0.f) angle = v >= 0.f ? atanf(v / u) + PI_F : atanf(v / u) - PI_F;
  else if (v > 0.f) angle = PI_F;
  else if (v < 0.f) angle = -PI_F;
  const float t = angle / (2.f * PI_F) + 1.0f;
  const float hue = t - floorf(t);                     // floormod(., 1)
  const float s = max_flow > 0.f ? clip01(mag * 8.f / max_flow) : 0.f;
  // tf.image.hsv_to_rgb with value 1 (clip(8 - s, 0, 1))
  const float d = 6.f * hue;
  const float r = clip01(fabsf(d - 3.f) - 1.f), g = clip01(2.f - fabsf(d - 2.f)), b = clip01(2.f - fabsf(d - 4.f));
  const float w = 1.f - s;
  return make_float3((w + s * r) * m, (w + s * g) * m, (w + s * b) * m);
}

// The KITTI devkit's colour map (flow_util.py:63-73): error in [lo, hi) -> rgb / 255; nothing matches from 1e9 on (black)
__device__ __forceinline__ float3 log_color(float error) {
  const float edge[11] = {0.f, 0.0625f, 0.125f, 0.25f, 0.5f, 1.f, 2.f, 4.f, 8.f, 16.f, 1000000000.0f};
  const float rgb[10][3] = {{49, 54, 149}, {69, 117, 180}, {116, 173, 209}, {171, 217, 233}, {224, 243, 248},
                            {254, 224, 144}, {253, 174, 97}, {244, 109, 67}, {215, 48, 39}, {165, 0, 38}};
  float3 c = make_float3(0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < 10; i++)
    if (error >= edge[i] && error < edge[i + 1]) c = make_float3(rgb[i][0] / 255.0f, rgb[i][1] / 255.0f, rgb[i][2] / 255.0f);
  return c;
}

// flow_util.py:46-95: f = flow_1, g = flow_2 (the ground truth)
__device__ __forceinline__ float3 error_color(float2 f, float2 g, float m_occ, float m_noc, bool log_colors) {
  const float du = f.x - g.x, dv = f.y - g.y;
  const float diff = sqrtf(du * du + dv * dv);
  if (log_colors) {
    const float mag = sqrtf(g.x * g.x + g.y * g.y);
    const float rel = mag > 0.f ? 20.f * diff / mag : INFINITY;        // |gt| = 0: the absolute term decides (diff = 0: bin 0)
    float3 c = log_color(fminf(diff / 3.f, rel));
    if (m_noc == 0.f) c = make_float3(c.x * 0.5f, c.y * 0.5f, c.z * 0.5f);
    return make_float3(c.x * m_occ, c.y * m_occ, c.z * m_occ);
  }
  const float e = (fminf(diff, 5.f) / 5.f) * m_occ;   // errors in occluded areas are red
  return make_float3(e, e * m_noc, e * m_noc);
}

__device__ __forceinline__ void put(float* __restrict__ f32, unsigned char* __restrict__ u8, long px, float3 c) {
  if (f32) { f32[px * 3] = c.x; f32[px * 3 + 1] = c.y; f32[px * 3 + 2] = c.z; }
  if (u8) { u8[px * 3] = to_byte(c.x); u8[px * 3 + 1] = to_byte(c.y); u8[px * 3 + 2] = to_byte(c.z); }
}

// max over the block of a non-negative value -> one atomicMax on its bit pattern
__device__ __forceinline__ void block_max_bits(float v, unsigned* __restrict__ slot, unsigned* red) {
  unsigned bits = __float_as_uint(v);
  for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_down((int)bits, o, 64));
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[wid] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = 0u;
    for (int k = 0; k < (int)(blockDim.x >> 6); k++) m = max(m, red[k]);
    if (m) atomicMax(slot, m);
  }
}

// After every thread of the block has read the maxima: the last block of `nb` to get here zeroes the `n` slots and the ticket.
__device__ __forceinline__ void release_max(unsigned* __restrict__ slots, int n, unsigned* __restrict__ ticket, unsigned nb) {
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == nb - 1u) {
    for (int k = 0; k < n; k++) slots[k] = 0u;
    *ticket = 0u;
  }
}

// |x| with NaN -> 0, so that the bit pattern orders like the value
__device__ __forceinline__ float abs_num(float x) { return fmaxf(fabsf(x), 0.f); }

// ------------------------------------------------------------------------------------------------ operator form (dense)
__global__ __launch_bounds__(VIS_THREADS) void flow_max_kernel(const float* __restrict__ flow, const float* __restrict__ mask, long npx,
                                                               unsigned* __restrict__ max_bits) {
  __shared__ unsigned red[VIS_THREADS / 64];
  float mx = 0.f;
  for (long i = blockIdx.x * (long)VIS_THREADS + threadIdx.x; i < npx; i += (long)gridDim.x * VIS_THREADS) {
    const float2 f = reinterpret_cast<const float2*>(flow)[i];
    const float m = mask ? mask[i] : 1.f;
    mx = fmaxf(mx, fmaxf(abs_num(f.x * m), abs_num(f.y * m)));
  }
  block_max_bits(mx, max_bits, red);
}

__global__ __launch_bounds__(VIS_THREADS) void flow_to_color_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                                    long npx, float max_flow, unsigned* __restrict__ max_bits,
                                                                    float* __restrict__ out_f32, unsigned char* __restrict__ out_u8) {
  const float mf = max_bits ? __uint_as_float(*max_bits) : max_flow;
  for (long i = blockIdx.x * (long)VIS_THREADS + threadIdx.x; i < npx; i += (long)gridDim.x * VIS_THREADS) {
    const float2 f = reinterpret_cast<const float2*>(flow)[i];
    put(out_f32, out_u8, i, wheel_color(f.x, f.y, mask ? mask[i] : 1.f, mf));
  }
  if (max_bits) release_max(max_bits, 1, max_bits + 1, gridDim.x);
}

__global__ __launch_bounds__(VIS_THREADS) void flow_error_image_kernel(const float* __restrict__ flow_1, const float* __restrict__ flow_2,
                                                                       const float* __restrict__ mask_occ,
                                                                       const float* __restrict__ mask_noc, int log_colors, long npx,
                                                                       float* __restrict__ out_f32, unsigned char* __restrict__ out_u8) {
  for (long i = blockIdx.x * (long)VIS_THREADS + threadIdx.x; i < npx; i += (long)gridDim.x * VIS_THREADS) {
    const float2 f = reinterpret_cast<const float2*>(flow_1)[i], g = reinterpret_cast<const float2*>(flow_2)[i];
    put(out_f32, out_u8, i, error_color(f, g, mask_occ[i], mask_noc ? mask_noc[i] : 1.f, log_colors != 0));
  }
}

// ------------------------------------------------------------------------------------------------ estimator form (desc)
// the frame the reference shows at frame pixel (y, x): resize_output(resize_input(frame)) — resize_tf1_point from (H, W) to
// (h, w), each corner resampled from the staged frame on the fly
template <typename T>
__device__ __forceinline__ float4 shown_pixel(const T* __restrict__ base, const FrameDesc& d, int Hmax, int Wmax, int H, int W, int y,
                                              int x, float sy2, float sx2) {
  const float fy = (float)y * sy2, fx = (float)x * sx2;
  const int Y0 = (int)floorf(fy), X0 = (int)floorf(fx);
  const int Y1 = min(Y0 + 1, H - 1), X1 = min(X0 + 1, W - 1);
  const float ly = fy - (float)Y0, lx = fx - (float)X0;
  const float3 tl = frame_resample(base, d, Hmax, Wmax, H, W, Y0, X0), tr = frame_resample(base, d, Hmax, Wmax, H, W, Y0, X1);
  const float3 bl = frame_resample(base, d, Hmax, Wmax, H, W, Y1, X0), br = frame_resample(base, d, Hmax, Wmax, H, W, Y1, X1);
  float v[3];
  const float t0[3] = {tl.x, tl.y, tl.z}, t1[3] = {tr.x, tr.y, tr.z}, b0[3] = {bl.x, bl.y, bl.z}, b1[3] = {br.x, br.y, br.z};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float top = t0[c] + (t1[c] - t0[c]) * lx, bot = b0[c] + (b1[c] - b0[c]) * lx;
    v[c] = top + (bot - top) * ly;
  }
  return make_float4(v[0], v[1], v[2], 0.f);
}

// the ground truth of frame pixel (y, x): at the frame's origin in its staging row, zero outside (as the output kernel reads it)
struct GtPx {
  float2 g;
  float m_occ, m_noc;
};

__device__ __forceinline__ GtPx load_gt(const float* __restrict__ gt_flow, const float* __restrict__ gt_mask, const FrameDesc& d, int nmaps,
                                        int B, int b, int Hmax, int Wmax, int y, int x) {
  GtPx o{make_float2(0.f, 0.f), 0.f, nmaps >= 2 ? 0.f : 1.f};
  const int r = y + d.y0, c = x + d.x0;
  if (r < 0 || r >= Hmax || c < 0 || c >= Wmax) return o;
  const long plane = (long)Hmax * Wmax, s = (long)b * plane + (long)r * Wmax + c;
  o.g = reinterpret_cast<const float2*>(gt_flow)[s];
  o.m_occ = gt_mask[s];
  if (nmaps >= 2) o.m_noc = gt_mask[(long)B * plane + s];
  return o;
}

__global__ __launch_bounds__(VIS_THREADS) void visual_frames_kernel(const void* __restrict__ frames, const int* __restrict__ desc, int B,
                                                                    int Hmax, int Wmax, int H, int W, const float* __restrict__ flow,
                                                                    const float* __restrict__ gt_flow, const float* __restrict__ gt_mask,
                                                                    float4* __restrict__ shown, unsigned* __restrict__ max_bits) {
  __shared__ unsigned red[VIS_THREADS / 64];
  const int b = blockIdx.y;
  const FrameDesc d = load_desc(desc, b);
  const int h = min(max(d.h, 0), Hmax), w = min(max(d.w, 0), Wmax);    // never past the (Hmax, Wmax) rows
  if (h == 0 || w == 0) return;                        // uniform per sample
  const int nmaps = gt_flow ? min(max(d.nmaps, 0), 2) : 0;
  const long plane = (long)Hmax * Wmax;
  const float sy2 = (float)H / (float)d.h, sx2 = (float)W / (float)d.w;
  const float2* fl = reinterpret_cast<const float2*>(flow) + b * plane;
  float mx = 0.f, mx_gt = 0.f;
  const int npx = h * w;                               // < 2^31 (the host checks Hmax * Wmax)
  for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < npx; p += gridDim.x * VIS_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
#pragma unroll
    for (int fr = 0; fr < 2; fr++) {
      const long off = ((long)fr * B + b) * plane * 3;
      shown[((long)fr * B + b) * plane + q] =
          d.u8 ? shown_pixel(reinterpret_cast<const unsigned char*>(frames) + off, d, Hmax, Wmax, H, W, y, x, sy2, sx2)
               : shown_pixel(reinterpret_cast<const float*>(frames) + off, d, Hmax, Wmax, H, W, y, x, sy2, sx2);
    }
    const float2 f = fl[q];
    mx = fmaxf(mx, fmaxf(abs_num(f.x), abs_num(f.y)));
    if (nmaps) {
      const GtPx t = load_gt(gt_flow, gt_mask, d, nmaps, B, b, Hmax, Wmax, y, x);
      mx_gt = fmaxf(mx_gt, fmaxf(abs_num(t.g.x * t.m_occ), abs_num(t.g.y * t.m_occ)));
    }
  }
  block_max_bits(mx, max_bits + 2 * b, red);
  if (nmaps) block_max_bits(mx_gt, max_bits + 2 * b + 1, red);         // uniform per sample
}

__global__ __launch_bounds__(VIS_THREADS) void visual_images_kernel(const int* __restrict__ desc, int B, int Hmax, int Wmax,
                                                                    const float* __restrict__ flow, const float* __restrict__ gt_flow,
                                                                    const float* __restrict__ gt_mask, const float4* __restrict__ shown,
                                                                    unsigned* __restrict__ max_bits, unsigned char* __restrict__ out_u8,
                                                                    float* __restrict__ out_f32) {
  const int b = blockIdx.y;
  const FrameDesc d = load_desc(desc, b);
  const int h = min(max(d.h, 0), Hmax), w = min(max(d.w, 0), Wmax);
  if (h == 0 || w == 0) return;
  const int nmaps = gt_flow ? min(max(d.nmaps, 0), 2) : 0;
  const long plane = (long)Hmax * Wmax;
  const float2* fl = reinterpret_cast<const float2*>(flow) + b * plane;
  const float4* im1 = shown + b * plane;
  const float4* im2 = shown + ((long)B + b) * plane;
  const float mf = __uint_as_float(max_bits[2 * b]), mf_gt = __uint_as_float(max_bits[2 * b + 1]);
  const int npx = h * w;
  for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < npx; p += gridDim.x * VIS_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    const float4 a = im1[q], s = im2[q];
    const float2 f = fl[q];
    // image_warp(im2, flow): image_warp_fwd_kernel's taps and tap order (csrc/ops_warp.hip, flow_scale 1)
    const IwTaps t = iw_sample(x, y, f.x * 1.0f, f.y * 1.0f, h, w, Wmax);
    const float4 ta = im2[t.ia], tb = im2[t.ib], tc = im2[t.ic], td = im2[t.id];
    const float3 wp = make_float3(((t.wa * ta.x + t.wb * tb.x) + t.wc * tc.x) + t.wd * td.x,
                                  ((t.wa * ta.y + t.wb * tb.y) + t.wc * tc.y) + t.wd * td.y,
                                  ((t.wa * ta.z + t.wb * tb.z) + t.wc * tc.z) + t.wd * td.z);
    float3 img[N_IMAGES];
    img[0] = make_float3((a.x * 0.5f + s.x * 0.5f) / 255.0f, (a.y * 0.5f + s.y * 0.5f) / 255.0f, (a.z * 0.5f + s.z * 0.5f) / 255.0f);
    img[1] = make_float3(fabsf(a.x - wp.x) / 255.0f, fabsf(a.y - wp.y) / 255.0f, fabsf(a.z - wp.z) / 255.0f);
    img[2] = wheel_color(f.x, f.y, 1.f, mf);
    if (nmaps) {
      const GtPx g = load_gt(gt_flow, gt_mask, d, nmaps, B, b, Hmax, Wmax, y, x);
      img[3] = error_color(f, g.g, g.m_occ, g.m_noc, true);
      img[4] = wheel_color(g.g.x, g.g.y, g.m_occ, mf_gt);
    }
#pragma unroll
    for (int k = 0; k < N_IMAGES; k++) {
      if (k >= 3 && !nmaps) continue;
      const long px = ((long)k * B + b) * plane + q;
      put(out_f32, out_u8, px, img[k]);
    }
  }
  release_max(max_bits + 2 * b, 2, max_bits + 2 * B + b, gridDim.x);   // every block of a sample with h > 0 gets here
}

// ------------------------------------------------------------------------------------------------ sequence form (tables)
// The tables of one sequence replay (core/inference.py sequence_tables): frame table [B][8] at word 0, pair table [B][8] at word
// 8B, carry source at word 16B, and at word 16B + 1 the bit pattern of a clip-wide max_flow (0: every pair has its own maximum).
__device__ __forceinline__ unsigned clip_max_bits(const int* __restrict__ tab, int B) { return (unsigned)tab[16 * B + 1]; }

// Block row j: staged frame j (frame slot j) -> shown row j + 1, each frame of the clip once; and the maxima of PAIR slot j,
// max |flow_fw| and max |flow_bw|.  The two slots are valid independently; no maxima with a clip-wide max_flow.
__global__ __launch_bounds__(VIS_THREADS) void sequence_visual_frames_kernel(const void* __restrict__ frames, const int* __restrict__ tab,
                                                                             int B, int Hmax, int Wmax, int H, int W,
                                                                             const float* __restrict__ flow_fw,
                                                                             const float* __restrict__ flow_bw, float4* __restrict__ shown,
                                                                             unsigned* __restrict__ max_bits) {
  __shared__ unsigned red[VIS_THREADS / 64];
  const int j = blockIdx.y;
  const long plane = (long)Hmax * Wmax;
  const FrameDesc d = load_desc(tab, j);
  const int fh = min(max(d.h, 0), Hmax), fw = min(max(d.w, 0), Wmax);  // never past the (Hmax, Wmax) rows
  if (fh > 0 && fw > 0) {                              // uniform per block row
    const float sy2 = (float)H / (float)d.h, sx2 = (float)W / (float)d.w;
    const long off = (long)j * plane * 3;
    float4* row = shown + ((long)j + 1) * plane;
    const int npx = fh * fw;                           // < 2^31 (the host checks Hmax * Wmax)
    for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < npx; p += gridDim.x * VIS_THREADS) {
      const int y = p / fw, x = p - y * fw;
      row[(long)y * Wmax + x] =
          d.u8 ? shown_pixel(reinterpret_cast<const unsigned char*>(frames) + off, d, Hmax, Wmax, H, W, y, x, sy2, sx2)
               : shown_pixel(reinterpret_cast<const float*>(frames) + off, d, Hmax, Wmax, H, W, y, x, sy2, sx2);
    }
  }
  const FrameDesc pd = load_desc(tab + 8 * B, j);
  const int h = min(max(pd.h, 0), Hmax), w = min(max(pd.w, 0), Wmax);
  if (h == 0 || w == 0 || clip_max_bits(tab, B) != 0u) return;         // uniform per block row
  const float2* ff = reinterpret_cast<const float2*>(flow_fw) + j * plane;
  const float2* fb = flow_bw ? reinterpret_cast<const float2*>(flow_bw) + j * plane : nullptr;
  float mx = 0.f, mx_bw = 0.f;
  const int npx = h * w;
  for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < npx; p += gridDim.x * VIS_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    const float2 f = ff[q];
    mx = fmaxf(mx, fmaxf(abs_num(f.x), abs_num(f.y)));
    if (fb) {
      const float2 g = fb[q];
      mx_bw = fmaxf(mx_bw, fmaxf(abs_num(g.x), abs_num(g.y)));
    }
  }
  block_max_bits(mx, max_bits + 2 * j, red);
  if (fb) block_max_bits(mx_bw, max_bits + 2 * j + 1, red);            // uniform per launch
}

// Pair i of the pair table: im1 = shown row i, im2 = shown row i + 1, flow_fw[i] -> images 0..2 with visual_images_kernel's
// expressions; with flow_bw / occ_fw: 3 the backward flow's colours, 4 the brightness error where the pixel is not occluded.
__global__ __launch_bounds__(VIS_THREADS) void sequence_visual_images_kernel(const int* __restrict__ tab, int B, int Hmax, int Wmax,
                                                                             const float* __restrict__ flow_fw,
                                                                             const float* __restrict__ flow_bw,
                                                                             const unsigned char* __restrict__ occ_fw,
                                                                             const float4* __restrict__ shown, unsigned* __restrict__ max_bits,
                                                                             unsigned char* __restrict__ out_u8, float* __restrict__ out_f32) {
  const int b = blockIdx.y;
  const FrameDesc d = load_desc(tab + 8 * B, b);
  const int h = min(max(d.h, 0), Hmax), w = min(max(d.w, 0), Wmax);
  if (h == 0 || w == 0) return;
  const long plane = (long)Hmax * Wmax;
  const float2* fl = reinterpret_cast<const float2*>(flow_fw) + b * plane;
  const float2* fb = flow_bw ? reinterpret_cast<const float2*>(flow_bw) + b * plane : nullptr;
  const unsigned char* oc = flow_bw ? occ_fw + b * plane : nullptr;
  const float4* im1 = shown + b * plane;
  const float4* im2 = shown + ((long)b + 1) * plane;
  const unsigned clip = clip_max_bits(tab, B);
  const float mf = __uint_as_float(clip ? clip : max_bits[2 * b]), mf_bw = __uint_as_float(clip ? clip : max_bits[2 * b + 1]);
  const int npx = h * w;
  for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < npx; p += gridDim.x * VIS_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    const float4 a = im1[q], s = im2[q];
    const float2 f = fl[q];
    // image_warp(im2, flow): image_warp_fwd_kernel's taps and tap order (csrc/ops_warp.hip, flow_scale 1)
    const IwTaps t = iw_sample(x, y, f.x * 1.0f, f.y * 1.0f, h, w, Wmax);
    const float4 ta = im2[t.ia], tb = im2[t.ib], tc = im2[t.ic], td = im2[t.id];
    const float3 wp = make_float3(((t.wa * ta.x + t.wb * tb.x) + t.wc * tc.x) + t.wd * td.x,
                                  ((t.wa * ta.y + t.wb * tb.y) + t.wc * tc.y) + t.wd * td.y,
                                  ((t.wa * ta.z + t.wb * tb.z) + t.wc * tc.z) + t.wd * td.z);
    float3 img[N_IMAGES];
    img[0] = make_float3((a.x * 0.5f + s.x * 0.5f) / 255.0f, (a.y * 0.5f + s.y * 0.5f) / 255.0f, (a.z * 0.5f + s.z * 0.5f) / 255.0f);
    img[1] = make_float3(fabsf(a.x - wp.x) / 255.0f, fabsf(a.y - wp.y) / 255.0f, fabsf(a.z - wp.z) / 255.0f);
    img[2] = wheel_color(f.x, f.y, 1.f, mf);
    if (fb) {
      const float2 g = fb[q];
      img[3] = wheel_color(g.x, g.y, 1.f, mf_bw);
      img[4] = oc[q] ? make_float3(0.f, 0.f, 0.f) : img[1];
    }
#pragma unroll
    for (int k = 0; k < N_IMAGES; k++) {
      if (k >= 3 && !fb) continue;
      const long px = ((long)k * B + b) * plane + q;
      put(out_f32, out_u8, px, img[k]);
    }
  }
  release_max(max_bits + 2 * b, 2, max_bits + 2 * B + b, gridDim.x);   // every block of a valid pair gets here
}

// one launch dimension of the dense kernels: about four pixels per thread
int dense_grid(long npx) { return (int)max(1L, min((npx + 4L * VIS_THREADS - 1) / (4L * VIS_THREADS), 4096L)); }

}  // namespace

UNFLOW_API int unflow_flow_to_color(const float* flow, const float* mask, const float* max_flow, int B, int H, int W, float* out_f32,
                                    unsigned char* out_u8, unsigned* max_bits, unflow_stream_t stream) {
  if (!flow || (!out_f32 && !out_u8)) return UNFLOW_ERR_NULL;
  if (!max_flow && !max_bits) return UNFLOW_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0) return UNFLOW_ERR_SHAPE;
  const long npx = (long)B * H * W;
  const hipStream_t st = as_stream(stream);
  float mf = 0.f;
  if (max_flow) {
    mf = fmaxf(max_flow[0], 1.0f);                     // flow_util.py:31-32
    max_bits = nullptr;
  } else {
    flow_max_kernel<<<dense_grid(npx), VIS_THREADS, 0, st>>>(flow, mask, npx, max_bits);
  }
  flow_to_color_kernel<<<dense_grid(npx), VIS_THREADS, 0, st>>>(flow, mask, npx, mf, max_bits, out_f32, out_u8);
  return launch_status();
}

UNFLOW_API int unflow_flow_error_image(const float* flow_1, const float* flow_2, const float* mask_occ, const float* mask_noc,
                                       int log_colors, int B, int H, int W, float* out_f32, unsigned char* out_u8,
                                       unflow_stream_t stream) {
  if (!flow_1 || !flow_2 || !mask_occ || (!out_f32 && !out_u8)) return UNFLOW_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0) return UNFLOW_ERR_SHAPE;
  const long npx = (long)B * H * W;
  flow_error_image_kernel<<<dense_grid(npx), VIS_THREADS, 0, as_stream(stream)>>>(flow_1, flow_2, mask_occ, mask_noc, log_colors, npx,
                                                                                  out_f32, out_u8);
  return launch_status();
}

UNFLOW_API int unflow_inference_visual(const void* frames, const int* desc, int B, int Hmax, int Wmax, int H, int W, const float* flow,
                                       const float* gt_flow, const float* gt_mask, float* shown, unsigned* max_bits,
                                       unsigned char* out_u8, float* out_f32, unflow_stream_t stream) {
  if (!frames || !desc || !flow || !shown || !max_bits || (!out_u8 && !out_f32)) return UNFLOW_ERR_NULL;
  if ((gt_flow != nullptr) != (gt_mask != nullptr)) return UNFLOW_ERR_NULL;
  if (B <= 0 || Hmax <= 0 || Wmax <= 0 || H <= 0 || W <= 0 || (long)Hmax * Wmax > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
  const hipStream_t st = as_stream(stream);
  const dim3 grid(unflow_inference_output_blocks(Hmax, Wmax), B);
  visual_frames_kernel<<<grid, VIS_THREADS, 0, st>>>(frames, desc, B, Hmax, Wmax, H, W, flow, gt_flow, gt_mask,
                                                     reinterpret_cast<float4*>(shown), max_bits);
  visual_images_kernel<<<grid, VIS_THREADS, 0, st>>>(desc, B, Hmax, Wmax, flow, gt_flow, gt_mask, reinterpret_cast<const float4*>(shown),
                                                     max_bits, out_u8, out_f32);
  return launch_status();
}

UNFLOW_API int unflow_sequence_visual(const void* frames, const int* tab, int B, int Hmax, int Wmax, int H, int W, const float* flow_fw,
                                      const float* flow_bw, const unsigned char* occ_fw, float* shown, unsigned* max_bits,
                                      unsigned char* out_u8, float* out_f32, unflow_stream_t stream) {
  if (!frames || !tab || !flow_fw || !shown || !max_bits || (!out_u8 && !out_f32)) return UNFLOW_ERR_NULL;
  if ((flow_bw != nullptr) != (occ_fw != nullptr)) return UNFLOW_ERR_NULL;
  if (B <= 0 || Hmax <= 0 || Wmax <= 0 || H <= 0 || W <= 0 || (long)Hmax * Wmax > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
  // the previous replay's last shown frame (row src) -> row 0, before the frames kernel overwrites rows [1, B]
  const unflow_carry_buf row{shown, (long)Hmax * Wmax, 16, 16};
  const int status = unflow_sequence_carry(&row, 1, tab + 16 * B, B, stream);
  if (status != UNFLOW_OK) return status;
  const hipStream_t st = as_stream(stream);
  const dim3 grid(unflow_inference_output_blocks(Hmax, Wmax), B);
  sequence_visual_frames_kernel<<<grid, VIS_THREADS, 0, st>>>(frames, tab, B, Hmax, Wmax, H, W, flow_fw, flow_bw,
                                                              reinterpret_cast<float4*>(shown), max_bits);
  sequence_visual_images_kernel<<<grid, VIS_THREADS, 0, st>>>(tab, B, Hmax, Wmax, flow_fw, flow_bw, occ_fw,
                                                              reinterpret_cast<const float4*>(shown), max_bits, out_u8, out_f32);
  return launch_status();
}
