// Forward-only flow inference (core/inference.py FlowEstimator): the two kernels around the network.
//
// Both take the geometry of every sample from a small device table (desc, include/unflow_hip.h), not from
// kernel arguments, so that one captured graph serves batches that mix frame sizes (KITTI: 370 x 1226, 375 x 1242,
// 376 x 1241) and a short final batch: the host rewrites the table, the graph stays.
//
// unflow_inference_input: staged frames [2][B][Hmax][Wmax][3] (uint8 or fp32, [0, 255]) -> the network input.  For every
//   network pixel: the TF1 legacy bilinear resample of the sample's (h, w) frame region (origin (y0, x0) in its staging
//   row; outside the buffer reads as zero: resize_input's crop / pad of the KITTIInput layout), /255, minus the channel mean
//   (unflow_prepare_image_pair's arithmetic); rows [0, B) = im1, [B, 2B) = im2, plus the operand planes of a FlowNetC's conv1.
// unflow_inference_input_frames: the same per pixel for sequence mode's layout, staged frames [F][Hmax][Wmax][3] -> F consecutive
//   rows of the network input (and of conv1's planes) from the row pointer the caller passes (csrc/sequence.hip: the carry).
// unflow_inference_output: the last network's flow2 (or flow0 with full_res) -> the frame-size flow of every sample: the
//   composed resize (final_flows()' resize * 20 to (H, W), then resize_output_flow's resize to (h, w) and per-axis rescale)
//   evaluated at the four points each frame pixel needs, with csrc/resize_tf1.h's expression: bit-identical to the chained
//   launches.  Optional: the KITTI 16-bit encoding (eval_gui.py flow_to_int16) and the EPE / outlier sums against up to two
//   ground-truth maps, reduced in a fixed order (per-block fp64 partials; the last block of a sample, found by an integer
//   ticket, sums them with a fixed thread-to-partial assignment and a fixed tree; no float atomics) — bit-identical from run to run and between graph replay and eager runs.
// unflow_inference_occlusion: the frame-size forward and backward flows (two unflow_inference_output launches) -> both
//   forward-backward occlusion masks of losses.occlusion (losses.py:125-134), image_warp's taps from csrc/image_warp.h, and
//   integer TP / FP / FN of the forward mask against KITTI's occluded pixels (per-block integer sums, one integer atomicAdd per
//   block and count: exact, hence the same from run to run).
#include "common.h"
#include "frame_desc.h"
#include "igemm_shared.h"
#include "image_warp.h"
#include "resize_tf1.h"

namespace {

constexpr int OUT_THREADS = 256;
constexpr int OCC_THREADS = 256;
constexpr int MAX_MAPS = 2;

template <typename T>
__device__ __forceinline__ float4 input_pixel(const T* __restrict__ base, const FrameDesc& d, int Hmax, int Wmax, int H, int W,
                                              int oy, int ox, float m0, float m1, float m2) {
  const float3 v = frame_resample(base, d, Hmax, Wmax, H, W, oy, ox);      // csrc/frame_desc.h
  return make_float4(v.x / 255.0f - m0, v.y / 255.0f - m1, v.z / 255.0f - m2, 0.f);
}

__global__ __launch_bounds__(256) void inference_input_kernel(const void* __restrict__ frames, const int* __restrict__ desc, int B,
                                                              int Hmax, int Wmax, int H, int W, float* __restrict__ net4,
                                                              igemm::PlaneOut pl, float m0, float m1, float m2) {
  const long per = (long)H * W, n = 2 * (long)B * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / per;                          // [0, 2B): frame fr = row / B of sample b = row % B
    const int p = (int)(i - row * per);
    const int oy = p / W, ox = p - oy * W;
    const FrameDesc d = load_desc(desc, (int)(row % B));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d.h > 0 && d.w > 0) {
      const long off = row * (long)Hmax * Wmax * 3;
      v = d.u8 ? input_pixel(reinterpret_cast<const unsigned char*>(frames) + off, d, Hmax, Wmax, H, W, oy, ox, m0, m1, m2)
               : input_pixel(reinterpret_cast<const float*>(frames) + off, d, Hmax, Wmax, H, W, oy, ox, m0, m1, m2);
    }
    reinterpret_cast<float4*>(net4)[i] = v;            // one 16-byte store; planes: one 8-byte store per plane
    igemm::store_planes4(pl, (size_t)i, 0, v);
  }
}

// Sequence mode: one frame per row.  Row r of the launch is frame r of the staging buffer with desc slot r; index i of net4 /
// pl counts from the row pointer the caller passed, so nothing outside the F rows is touched.  The value of a pixel is
// inference_input_kernel's expression (input_pixel, store_planes4): a row is bit-identical to the pair kernel's row.
__global__ __launch_bounds__(256) void inference_input_frames_kernel(const void* __restrict__ frames, const int* __restrict__ desc,
                                                                     int F, int Hmax, int Wmax, int H, int W,
                                                                     float* __restrict__ net4, igemm::PlaneOut pl, float m0, float m1,
                                                                     float m2) {
  const long per = (long)H * W, n = (long)F * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / per;                          // [0, F)
    const int p = (int)(i - row * per);
    const int oy = p / W, ox = p - oy * W;
    const FrameDesc d = load_desc(desc, (int)row);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d.h > 0 && d.w > 0) {
      const long off = row * (long)Hmax * Wmax * 3;
      v = d.u8 ? input_pixel(reinterpret_cast<const unsigned char*>(frames) + off, d, Hmax, Wmax, H, W, oy, ox, m0, m1, m2)
               : input_pixel(reinterpret_cast<const float*>(frames) + off, d, Hmax, Wmax, H, W, oy, ox, m0, m1, m2);
    }
    reinterpret_cast<float4*>(net4)[i] = v;
    igemm::store_planes4(pl, (size_t)i, 0, v);
  }
}

// final_flows()' value at network pixel (Y, X), channel c: resize_bilinear_tf1(flow, H, W) * scale, or flow * scale when the
// flow is already at (H, W) (full_res: unflow_scale of flow0)
__device__ __forceinline__ float final_at(const float* __restrict__ fb, int fh, int fw, int H, int W, float sy, float sx, float scale,
                                          int c, int Y, int X) {
  if (fh == H && fw == W) return fb[((long)Y * W + X) * 2 + c] * scale;
  return resize_tf1_point(fb + c, fh, fw, 2, Y, X, sy, sx) * scale;
}

__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < (int)(blockDim.x >> 6); k++) t += red[k];
  return t;                                            // valid in thread 0
}

__global__ __launch_bounds__(OUT_THREADS) void inference_output_kernel(
    const float* __restrict__ flow, int fh, int fw, float flow_scale, int H, int W, const int* __restrict__ desc, int B, int Hmax,
    int Wmax, float* __restrict__ out_flow, unsigned short* __restrict__ out_u16, const float* __restrict__ gt_flow,
    const float* __restrict__ gt_mask, double* __restrict__ partial, unsigned* __restrict__ ticket, double* __restrict__ sums,
    int* __restrict__ counts) {
  __shared__ double red[OUT_THREADS / 64];
  __shared__ int last;
  const int b = blockIdx.y;
  const FrameDesc d = load_desc(desc, b);
  const int nmaps = (gt_flow && gt_mask && d.h > 0) ? min(d.nmaps, MAX_MAPS) : 0;
  const float* fb = flow + (long)b * fh * fw * 2;
  const float sy1 = (float)fh / (float)H, sx1 = (float)fw / (float)W;               // flow -> (H, W)
  const float sy2 = d.h > 0 ? (float)H / (float)d.h : 0.f, sx2 = d.w > 0 ? (float)W / (float)d.w : 0.f;   // (H, W) -> (h, w)
  const float ru = (float)((double)d.w / (double)W), rv = (float)((double)d.h / (double)H);             // resize_output_flow
  const long plane = (long)Hmax * Wmax;
  double e_sum[MAX_MAPS] = {0.0, 0.0}, o_sum[MAX_MAPS] = {0.0, 0.0}, m_sum[MAX_MAPS] = {0.0, 0.0};
  // the output rows hold (Hmax, Wmax): a larger frame (the host refuses one) would be cut, never written past its row
  const int oh = min(max(d.h, 0), Hmax), ow = min(max(d.w, 0), Wmax);
  const int npx = oh * ow;                             // < 2^31: Hmax * Wmax staging pixels (32-bit division below)
  for (int p = blockIdx.x * OUT_THREADS + threadIdx.x; p < npx; p += gridDim.x * OUT_THREADS) {
    const int y = p / ow, x = p - y * ow;
    // resize_tf1_point from (H, W) to (h, w), each of its four corners formed from the flow on the fly
    const float fy = (float)y * sy2, fx = (float)x * sx2;
    const int Y0 = (int)floorf(fy), X0 = (int)floorf(fx);
    const int Y1 = min(Y0 + 1, H - 1), X1 = min(X0 + 1, W - 1);
    const float ly = fy - (float)Y0, lx = fx - (float)X0;
    float uv[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const float tl = final_at(fb, fh, fw, H, W, sy1, sx1, flow_scale, c, Y0, X0);
      const float tr = final_at(fb, fh, fw, H, W, sy1, sx1, flow_scale, c, Y0, X1);
      const float bl = final_at(fb, fh, fw, H, W, sy1, sx1, flow_scale, c, Y1, X0);
      const float br = final_at(fb, fh, fw, H, W, sy1, sx1, flow_scale, c, Y1, X1);
      const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
      uv[c] = (top + (bot - top) * ly) * 1.0f;       // unflow_resize_bilinear_tf1(., h, w, scale = 1)
    }
    const float u = uv[0] * ru, v = uv[1] * rv;
    const long q = (long)b * plane + (long)y * Wmax + x;
    if (out_flow) reinterpret_cast<float2*>(out_flow)[q] = make_float2(u, v);
    if (out_u16) {
      // eval_gui.py:68-74: cast(max(0, min(x * 64 + 32768, 65535))) — truncation; third channel 1
      unsigned short* o = out_u16 + q * 3;
      o[0] = (unsigned short)fmaxf(0.f, fminf(u * 64.0f + 32768.0f, 65535.0f));
      o[1] = (unsigned short)fmaxf(0.f, fminf(v * 64.0f + 32768.0f, 65535.0f));
      o[2] = 1;
    }
    if (nmaps) {
      // the ground truth of frame pixel (y, x) sits at the frame's origin in its staging row (resize_output_crop)
      const int r = y + d.y0, cc = x + d.x0;
      const bool in = r >= 0 && r < Hmax && cc >= 0 && cc < Wmax;
#pragma unroll
      for (int k = 0; k < MAX_MAPS; k++) {
        if (k >= nmaps) continue;
        float2 g = make_float2(0.f, 0.f);
        float m = 0.f;
        if (in) {
          const long s = ((long)k * B + b) * plane + (long)r * Wmax + cc;
          g = reinterpret_cast<const float2*>(gt_flow)[s];
          m = gt_mask[s];
        }
        const float du = g.x - u, dv = g.y - v;
        const float diff = sqrtf(du * du + dv * dv) * m;                    // flow_util.py euclidean(gt - flow) * mask
        const float thr = fmaxf(sqrtf(g.x * g.x + g.y * g.y) * 0.05f, 3.0f);
        e_sum[k] += (double)diff;
        o_sum[k] += diff >= thr ? 1.0 : 0.0;
        m_sum[k] += (double)m;
      }
    }
  }
  if (nmaps == 0) return;                              // uniform per sample: every block of it takes this branch
  // fixed-order reduction: block partials in fp64, summed by the last block of the sample
  const int nb = gridDim.x;
#pragma unroll
  for (int k = 0; k < MAX_MAPS; k++) {
    if (k >= nmaps) continue;                          // uniform: every thread of the block skips together
    const double e = block_sum_f64(e_sum[k], red), o = block_sum_f64(o_sum[k], red), m = block_sum_f64(m_sum[k], red);
    if (threadIdx.x == 0) {
      double* pp = partial + (((long)b * nb + blockIdx.x) * MAX_MAPS + k) * 3;
      pp[0] = e; pp[1] = o; pp[2] = m;
    }
  }
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(ticket + b, 1u) == (unsigned)(nb - 1);
  }
  __syncthreads();
  if (!last) return;
  // the sample's last block: every thread sums a fixed stride of the block partials, then the block tree — a fixed order for
  // a given grid, independent of which block finished last
  __threadfence();
#pragma unroll
  for (int k = 0; k < MAX_MAPS; k++) {
    if (k >= nmaps) continue;
    double e = 0.0, o = 0.0, m = 0.0;
    for (int j = threadIdx.x; j < nb; j += OUT_THREADS) {
      const volatile double* pp = partial + (((long)b * nb + j) * MAX_MAPS + k) * 3;
      e += pp[0]; o += pp[1]; m += pp[2];
    }
    e = block_sum_f64(e, red);
    o = block_sum_f64(o, red);
    m = block_sum_f64(m, red);
    if (threadIdx.x == 0) {
      sums[((long)b * MAX_MAPS + k) * 2] = e;
      sums[((long)b * MAX_MAPS + k) * 2 + 1] = m;
      counts[(long)b * MAX_MAPS + k] = (int)o;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) ticket[b] = 0u;                // ready for the next launch (graph replays included)
}

// image_warp(im, flow) at frame pixel (x, y) of a sample whose frame is h x w, rows Wmax apart: the partner field `im` at
// (x, y) + f, clamped to the frame — image_warp_fwd_kernel's taps and tap order (csrc/ops_warp.hip, flow_scale 1)
__device__ __forceinline__ float2 warp_at(const float2* __restrict__ im, int x, int y, float2 f, int h, int w, int Wmax) {
#pragma clang fp contract(off)
  const IwTaps t = iw_sample(x, y, f.x, f.y, h, w, Wmax);
  const float2 a = im[t.ia], b = im[t.ib], c = im[t.ic], d = im[t.id];
  return make_float2(((t.wa * a.x + t.wb * b.x) + t.wc * c.x) + t.wd * d.x, ((t.wa * a.y + t.wb * b.y) + t.wc * c.y) + t.wd * d.y);
}

__global__ __launch_bounds__(OCC_THREADS) void inference_occlusion_kernel(
    const float* __restrict__ flow_fw, const float* __restrict__ flow_bw, const int* __restrict__ desc, int B, int Hmax, int Wmax,
    const float* __restrict__ gt_mask, unsigned char* __restrict__ occ_fw, unsigned char* __restrict__ occ_bw,
    int* __restrict__ counts) {
  // losses.occlusion is a chain of separate torch kernels: every product and sum below is rounded on its own (no FMA)
#pragma clang fp contract(off)
  __shared__ int red[3][OCC_THREADS / 64];
  const int b = blockIdx.y;
  const FrameDesc d = load_desc(desc, b);
  const int h = min(max(d.h, 0), Hmax), w = min(max(d.w, 0), Wmax);    // never past the (Hmax, Wmax) rows
  const bool score = gt_mask != nullptr && d.nmaps >= 2 && h > 0 && w > 0;
  const long plane = (long)Hmax * Wmax;
  const float2* fw = reinterpret_cast<const float2*>(flow_fw) + b * plane;
  const float2* bw = reinterpret_cast<const float2*>(flow_bw) + b * plane;
  int tp = 0, fp = 0, fn = 0;
  const int npx = h * w;                               // < 2^31 (the host checks Hmax * Wmax)
  for (int p = blockIdx.x * OCC_THREADS + threadIdx.x; p < npx; p += gridDim.x * OCC_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    const float2 f = fw[q], g = bw[q];
    const float2 gw = warp_at(bw, x, y, f, h, w, Wmax);     // image_warp(flow_bw, flow_fw)
    const float2 fwp = warp_at(fw, x, y, g, h, w, Wmax);    // image_warp(flow_fw, flow_bw)
    const float mag = (f.x * f.x + f.y * f.y) + (g.x * g.x + g.y * g.y);     // |fw|^2 + |bw|^2, unwarped
    const float thr = 0.01f * mag + 0.5f;
    const float dfx = f.x + gw.x, dfy = f.y + gw.y, dbx = g.x + fwp.x, dby = g.y + fwp.y;
    const bool o_fw = dfx * dfx + dfy * dfy > thr, o_bw = dbx * dbx + dby * dby > thr;
    occ_fw[b * plane + q] = o_fw ? 1 : 0;
    occ_bw[b * plane + q] = o_bw ? 1 : 0;
    if (score) {
      // KITTI's maps at the frame's origin in its staging row (as the output kernel reads them): map 0 = occ, map 1 = noc
      const int r = y + d.y0, c = x + d.x0;
      if (r >= 0 && r < Hmax && c >= 0 && c < Wmax) {
        const long s = (long)r * Wmax + c;
        const float m_occ = gt_mask[(long)b * plane + s], m_noc = gt_mask[((long)B + b) * plane + s];
        if (m_occ == 1.f) {                            // evaluated pixel; occluded in the ground truth: not in noc
          const bool gt_occ = m_noc == 0.f;
          tp += (o_fw && gt_occ) ? 1 : 0;
          fp += (o_fw && !gt_occ) ? 1 : 0;
          fn += (!o_fw && gt_occ) ? 1 : 0;
        }
      }
    }
  }
  if (!score) return;                                  // uniform per sample: every block of it takes this branch
  const int v[3] = {tp, fp, fn};
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int s = v[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) red[k][wid] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int s = 0;
    for (int i = 0; i < OCC_THREADS / 64; i++) s += red[threadIdx.x][i];
    if (s) atomicAdd(counts + (long)b * 3 + threadIdx.x, s);
  }
}

__global__ void zero_counts_kernel(int* __restrict__ counts, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) counts[i] = 0;
}

}  // namespace

UNFLOW_API int unflow_inference_input(const void* frames, const int* desc, int B, int Hmax, int Wmax, int H, int W, float* net_in4,
                                      const float* mean3, const unflow_planes* net_pl, unflow_stream_t stream) {
  if (!frames || !desc || !net_in4 || !mean3) return UNFLOW_ERR_NULL;
  if (B <= 0 || Hmax <= 0 || Wmax <= 0 || H <= 0 || W <= 0) return UNFLOW_ERR_SHAPE;
  igemm::PlaneOut pl{};
  if (net_pl && net_pl->base) {
    if ((net_pl->n_planes != 1 && net_pl->n_planes != 3) || net_pl->ld < 4 || net_pl->ld % 4 != 0 ||
        (reinterpret_cast<uintptr_t>(net_pl->base) & 7) != 0)
      return UNFLOW_ERR_UNSUPPORTED;
    pl.base = reinterpret_cast<unsigned short*>(net_pl->base);
    pl.plane_stride = net_pl->plane_stride;
    pl.ld = net_pl->ld; pl.lo = 0; pl.hi = 4; pl.n_planes = net_pl->n_planes;
  }
  const float m0 = mean3[0] / 255.0f, m1 = mean3[1] / 255.0f, m2 = mean3[2] / 255.0f;
  inference_input_kernel<<<stream_grid(2L * B * H * W), 256, 0, as_stream(stream)>>>(frames, desc, B, Hmax, Wmax, H, W, net_in4, pl,
                                                                                    m0, m1, m2);
  return launch_status();
}

UNFLOW_API int unflow_inference_input_frames(const void* frames, const int* desc, int F, int Hmax, int Wmax, int H, int W,
                                             float* net_in4, const float* mean3, const unflow_planes* net_pl,
                                             unflow_stream_t stream) {
  if (!frames || !desc || !net_in4 || !mean3) return UNFLOW_ERR_NULL;
  if (F <= 0 || Hmax <= 0 || Wmax <= 0 || H <= 0 || W <= 0) return UNFLOW_ERR_SHAPE;
  igemm::PlaneOut pl{};
  if (net_pl && net_pl->base) {
    if ((net_pl->n_planes != 1 && net_pl->n_planes != 3) || net_pl->ld < 4 || net_pl->ld % 4 != 0 ||
        (reinterpret_cast<uintptr_t>(net_pl->base) & 7) != 0)
      return UNFLOW_ERR_UNSUPPORTED;
    pl.base = reinterpret_cast<unsigned short*>(net_pl->base);
    pl.plane_stride = net_pl->plane_stride;
    pl.ld = net_pl->ld; pl.lo = 0; pl.hi = 4; pl.n_planes = net_pl->n_planes;
  }
  const float m0 = mean3[0] / 255.0f, m1 = mean3[1] / 255.0f, m2 = mean3[2] / 255.0f;
  inference_input_frames_kernel<<<stream_grid((long)F * H * W), 256, 0, as_stream(stream)>>>(frames, desc, F, Hmax, Wmax, H, W,
                                                                                            net_in4, pl, m0, m1, m2);
  return launch_status();
}

UNFLOW_API int unflow_inference_output_blocks(int Hmax, int Wmax) {
  const long px = (long)Hmax * Wmax;
  const long nb = (px + 4L * OUT_THREADS - 1) / (4L * OUT_THREADS);   // about four pixels per thread
  return (int)max(1L, min(nb, 1024L));
}

UNFLOW_API int unflow_inference_output(const float* flow, int fh, int fw, float flow_scale, int H, int W, const int* desc, int B,
                                       int Hmax, int Wmax, float* out_flow, unsigned short* out_u16, const float* gt_flow,
                                       const float* gt_mask, double* partial, unsigned* ticket, double* sums, int* counts,
                                       unflow_stream_t stream) {
  if (!flow || !desc) return UNFLOW_ERR_NULL;
  if (B <= 0 || Hmax <= 0 || Wmax <= 0 || H <= 0 || W <= 0 || fh <= 0 || fw <= 0 || fh > H || fw > W) return UNFLOW_ERR_SHAPE;
  if ((gt_flow != nullptr) != (gt_mask != nullptr)) return UNFLOW_ERR_NULL;
  if (gt_flow && (!partial || !ticket || !sums || !counts)) return UNFLOW_ERR_NULL;
  const dim3 grid(unflow_inference_output_blocks(Hmax, Wmax), B);
  inference_output_kernel<<<grid, OUT_THREADS, 0, as_stream(stream)>>>(flow, fh, fw, flow_scale, H, W, desc, B, Hmax, Wmax,
                                                                       out_flow, out_u16, gt_flow, gt_mask, partial, ticket, sums,
                                                                       counts);
  return launch_status();
}

UNFLOW_API int unflow_inference_occlusion(const float* flow_fw, const float* flow_bw, const int* desc, int B, int Hmax, int Wmax,
                                          const float* gt_mask, unsigned char* occ_fw, unsigned char* occ_bw, int* counts,
                                          unflow_stream_t stream) {
  if (!flow_fw || !flow_bw || !desc || !occ_fw || !occ_bw) return UNFLOW_ERR_NULL;
  if (gt_mask && !counts) return UNFLOW_ERR_NULL;
  if (B <= 0 || Hmax <= 0 || Wmax <= 0 || (long)Hmax * Wmax > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
  const hipStream_t st = as_stream(stream);
  // zeroed by a launch, not by hipMemsetAsync: inside a replayed graph a memset node of a few bytes has left other words than
  // zero in its target (DESIGN 7.4 met it at 24 bytes; 7.17 met it here, at B = 2, once the counts of a sequence graph were read)
  if (counts) zero_counts_kernel<<<1, 64, 0, st>>>(counts, 3 * B);
  const dim3 grid(unflow_inference_output_blocks(Hmax, Wmax), B);
  inference_occlusion_kernel<<<grid, OCC_THREADS, 0, st>>>(flow_fw, flow_bw, desc, B, Hmax, Wmax, gt_mask, occ_fw, occ_bw, counts);
  return launch_status();
}
