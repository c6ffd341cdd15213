// Supervised fine-tuning step (src/e2eflow/core/supervised.py:12-65): the loss of one network's final flow against the
// KITTI ground truth, and the one-direction stage input of a FlowNetS refinement network.
//
// unflow_supervised_flow_loss fuses what an unfused path would run as five launches with four full-resolution round trips
// (resize_bilinear * 20, subtract the GT, masked Charbonnier, its gradient, the adjoint of the resize): one workgroup per
// tile of FT x FT fine pixels (T = FT / r coarse pixels per side).
//   1. the coarse flow of the tile plus a one-pixel apron goes to LDS;
//   2. every fine pixel of the tile and of its r-pixel top / left halo forms the upsampled flow with the fp32 expression
//      order of resize_bilinear_tf1_kernel (csrc/train_misc.hip: the flow the loss sees is bit-identical to
//      FlowNetEngine.final_flows()), reads its GT and mask, and writes d loss / d final to LDS; the loss of a fine pixel
//      is counted by the tile that owns it, never by a halo;
//   3. the adjoint of the upsampling is a gather, separable and in a fixed order: first along x (coarse column j takes the
//      fine columns [r(j-1), r(j+1)-1] with their legacy-bilinear weights, ascending), then along y the same way.
// d_flow therefore has no float atomics and is bit-reproducible; the loss uses the block-partial atomicAdd of every other
// loss kernel (csrc/loss.hip).  About 12 bytes per fine pixel (GT, mask, ~1/r^2 of the coarse flow): a launch-bound kernel.
#include "common.h"

#define SUP_ALPHA 0.45f
#define SUP_EPS 0.001f

template <int R>
struct SupTile {
  static constexpr int FT = (R == 1) ? 32 : 64;   // fine tile side
  static constexpr int T = FT / R;                 // coarse tile side
  static constexpr int FH = FT + R;                // fine rows / columns incl. the top / left halo
  static constexpr int CA = T + 2;                 // coarse rows / columns incl. the apron
};

template <int R>
__global__ __launch_bounds__(256) void supervised_flow_loss_kernel(const float* __restrict__ flow, int h, int w,
                                                                   const float* __restrict__ gt,
                                                                   const float* __restrict__ mask, float flow_scale,
                                                                   float loss_scale, float grad_scale,
                                                                   float* __restrict__ loss_acc, float* __restrict__ d_flow,
                                                                   int accumulate, int H, int W, int tiles_x,
                                                                   int tiles_y) {
  using S = SupTile<R>;
  constexpr int T = S::T, FH = S::FH, CA = S::CA;
  __shared__ float2 cf[CA][CA];      // coarse flow, rows / cols ci0-1 .. ci0+T
  __shared__ float2 g[FH][FH];       // d loss / d final, fine rows / cols fi0-R .. fi0+FT-1
  __shared__ float2 gx[FH][T];       // after the x gather
  __shared__ float red[4];
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
  const int ci0 = ty * T, cj0 = tx * T, fi0 = ci0 * R, fj0 = cj0 * R;
  const float2* fl = reinterpret_cast<const float2*>(flow) + (long)b * h * w;
  const float2* gt2 = reinterpret_cast<const float2*>(gt) + (long)b * H * W;
  const float* mk = mask ? mask + (long)b * H * W : nullptr;
  // 1. coarse tile + apron (indices outside the image are never read below)
  for (int e = threadIdx.x; e < CA * CA; e += blockDim.x) {
    const int ci = ci0 - 1 + e / CA, cj = cj0 - 1 + e % CA;
    float2 v = make_float2(0.f, 0.f);
    if (ci >= 0 && ci < h && cj >= 0 && cj < w) v = fl[(long)ci * w + cj];
    cf[e / CA][e % CA] = v;
  }
  __syncthreads();
  // 2. d loss / d final over the tile and its halo; the loss over the owned pixels
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  float part = 0.f;
  for (int e = threadIdx.x; e < FH * FH; e += blockDim.x) {
    const int ly_ = e / FH, lx_ = e % FH;
    const int oy = fi0 - R + ly_, ox = fj0 - R + lx_;
    float2 gv = make_float2(0.f, 0.f);
    if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
      // resize_bilinear_tf1_kernel's expression, term for term
      const float fy = (float)oy * sy, fx = (float)ox * sx;
      const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
      const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
      const float ly = fy - (float)y0, lx = fx - (float)x0;
      const float2 tl = cf[y0 - ci0 + 1][x0 - cj0 + 1], tr = cf[y0 - ci0 + 1][x1 - cj0 + 1];
      const float2 bl = cf[y1 - ci0 + 1][x0 - cj0 + 1], br = cf[y1 - ci0 + 1][x1 - cj0 + 1];
      const float topu = tl.x + (tr.x - tl.x) * lx, botu = bl.x + (br.x - bl.x) * lx;
      const float topv = tl.y + (tr.y - tl.y) * lx, botv = bl.y + (br.y - bl.y) * lx;
      const float u = (topu + (botu - topu) * ly) * flow_scale, v = (topv + (botv - topv) * ly) * flow_scale;
      const long p = (long)oy * W + ox;
      const float2 t = gt2[p];
      const float m = mk ? mk[p] : 1.f;
      const float du = u - t.x, dv = v - t.y;
      const float qu = du * du + SUP_EPS * SUP_EPS, qv = dv * dv + SUP_EPS * SUP_EPS;
      const float eu = powf(qu, SUP_ALPHA), ev = powf(qv, SUP_ALPHA);
      if (oy >= fi0 && ox >= fj0) part += m * eu + m * ev;
      // d/d d of (d^2 + eps^2)^alpha = 2 alpha d (d^2 + eps^2)^(alpha - 1)
      gv = make_float2(grad_scale * m * du * (eu / qu), grad_scale * m * dv * (ev / qv));
    }
    g[ly_][lx_] = gv;
  }
  const float tot = block_sum(part, red);
  if (threadIdx.x == 0 && loss_acc) atomicAdd(loss_acc, tot * loss_scale);
  if (!d_flow) return;
  // 3a. gather along x: coarse column j <- fine columns [R(j-1), R(j+1)-1], ascending
  for (int e = threadIdx.x; e < FH * T; e += blockDim.x) {
    const int r = e / T, jj = e % T, j = cj0 + jj;
    float su = 0.f, sv = 0.f;
    if (j < w) {
#pragma unroll
      for (int k = 0; k < 2 * R; k++) {
        const int ox = R * (j - 1) + k;
        if (ox < 0 || ox >= W) continue;
        const float fx = (float)ox * sx;
        const int x0 = (int)floorf(fx), x1 = min(x0 + 1, w - 1);
        const float lx = fx - (float)x0;
        const float wt = (x0 == j ? 1.f - lx : 0.f) + (x1 == j ? lx : 0.f);
        const float2 q = g[r][ox - fj0 + R];
        su += wt * q.x;
        sv += wt * q.y;
      }
    }
    gx[r][jj] = make_float2(su, sv);
  }
  __syncthreads();
  // 3b. gather along y, then d flow = flow_scale * (adjoint of the resize)
  for (int e = threadIdx.x; e < T * T; e += blockDim.x) {
    const int ii = e / T, jj = e % T, i = ci0 + ii, j = cj0 + jj;
    if (i >= h || j >= w) continue;
    float su = 0.f, sv = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * R; k++) {
      const int oy = R * (i - 1) + k;
      if (oy < 0 || oy >= H) continue;
      const float fy = (float)oy * sy;
      const int y0 = (int)floorf(fy), y1 = min(y0 + 1, h - 1);
      const float ly = fy - (float)y0;
      const float wt = (y0 == i ? 1.f - ly : 0.f) + (y1 == i ? ly : 0.f);
      const float2 q = gx[oy - fi0 + R][jj];
      su += wt * q.x;
      sv += wt * q.y;
    }
    float2* o = reinterpret_cast<float2*>(d_flow) + ((long)b * h + i) * w + j;
    float2 r2 = make_float2(su * flow_scale, sv * flow_scale);
    if (accumulate) {
      const float2 old = *o;
      r2 = make_float2(old.x + r2.x, old.y + r2.y);
    }
    *o = r2;
  }
}

template <int R>
static void launch_sup(const float* flow, int h, int w, const float* gt, const float* mask, float flow_scale, float loss_scale,
                       float grad_scale, float* loss_acc, float* d_flow, int accumulate, int B, int H, int W,
                       hipStream_t st) {
  using S = SupTile<R>;
  const int tiles_x = cdiv(w, S::T), tiles_y = cdiv(h, S::T);
  supervised_flow_loss_kernel<R><<<B * tiles_x * tiles_y, 256, 0, st>>>(flow, h, w, gt, mask, flow_scale, loss_scale,
                                                                        grad_scale, loss_acc, d_flow, accumulate, H, W,
                                                                        tiles_x, tiles_y);
}

UNFLOW_API int unflow_supervised_flow_loss(const float* flow, int h, int w, const float* flow_gt, const float* mask_gt,
                                           float flow_scale, float weight, float* loss_acc, float* d_flow, int accumulate,
                                           int B, int H, int W, unflow_stream_t stream) {
  if (!flow || !flow_gt || !loss_acc) return UNFLOW_ERR_NULL;
  if (B <= 0 || h <= 0 || w <= 0 || H % h != 0 || W % w != 0 || H / h != W / w) return UNFLOW_ERR_SHAPE;
  const int r = H / h;
  if (r != 1 && r != 2 && r != 4 && r != 8) return UNFLOW_ERR_SHAPE;
  if ((long)B * H * W >= (1L << 31)) return UNFLOW_ERR_SHAPE;
  // normaliser B*H*W*2 (losses.py:311-312: every element of the difference, not the mask sum); the same fp32 quotient the
  // per-level loss entry points form from (weight, normaliser)
  const float loss_scale = weight / ((float)B * (float)H * (float)W * 2.f);
  const float grad_scale = loss_scale * (2.f * SUP_ALPHA);
  hipStream_t st = as_stream(stream);
  switch (r) {
    case 1: launch_sup<1>(flow, h, w, flow_gt, mask_gt, flow_scale, loss_scale, grad_scale, loss_acc, d_flow, accumulate, B, H, W, st); break;
    case 2: launch_sup<2>(flow, h, w, flow_gt, mask_gt, flow_scale, loss_scale, grad_scale, loss_acc, d_flow, accumulate, B, H, W, st); break;
    case 4: launch_sup<4>(flow, h, w, flow_gt, mask_gt, flow_scale, loss_scale, grad_scale, loss_acc, d_flow, accumulate, B, H, W, st); break;
    default: launch_sup<8>(flow, h, w, flow_gt, mask_gt, flow_scale, loss_scale, grad_scale, loss_acc, d_flow, accumulate, B, H, W, st); break;
  }
  return launch_status();
}

// ------------------------------------------------------------------ one-direction stage input (flownet.py:46-59)
// The engine's network input is [im1; im2] (2B rows); a FlowNetS stage of the one-direction engine takes first = rows
// [0, B), second = rows [B, 2B) — second = first + B*H*W pixels.  Same maths as stack_input_kernel / stack_input_bwd_kernel
// of csrc/train_misc.hip (those pair the rows of the directed batch modulo their output count and stay as they are).
__device__ __forceinline__ void upsampled_flow(const float* prev, int n, int x, int y, int h, int w, float sy, float sx,
                                               float fscale, float& u, float& v, int& y0, int& x0, int& y1, int& x1,
                                               float& ly, float& lx) {
  const float fy = (float)y * sy, fx = (float)x * sx;
  y0 = (int)floorf(fy);
  x0 = (int)floorf(fx);
  y1 = min(y0 + 1, h - 1);
  x1 = min(x0 + 1, w - 1);
  ly = fy - (float)y0;
  lx = fx - (float)x0;
  const float2* pf = reinterpret_cast<const float2*>(prev) + (long)n * h * w;
  const float2 tl = pf[(long)y0 * w + x0], tr = pf[(long)y0 * w + x1], bl = pf[(long)y1 * w + x0], br = pf[(long)y1 * w + x1];
  const float tu = tl.x + (tr.x - tl.x) * lx, bu = bl.x + (br.x - bl.x) * lx;
  const float tv = tl.y + (tr.y - tl.y) * lx, bv = bl.y + (br.y - bl.y) * lx;
  u = (tu + (bu - tu) * ly) * fscale;
  v = (tv + (bv - tv) * ly) * fscale;
}

__global__ void stack_input_pair_kernel(const float* __restrict__ first, const float* __restrict__ second,
                                        const float* __restrict__ prev, float* __restrict__ out, int ldo, int N, int H, int W,
                                        int h, int w, float fscale) {
  const long npx = (long)N * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < npx; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int n = (int)(i / ((long)W * H));
    const long sb = (long)n * H * W;
    const float4 a = reinterpret_cast<const float4*>(first)[i];
    const float4 b = reinterpret_cast<const float4*>(second)[i];
    float* o = out + i * ldo;
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
    o[3] = b.x; o[4] = b.y; o[5] = b.z;
    if (!prev) continue;
    float u, v, ly, lx;
    int y0, x0, y1, x1;
    upsampled_flow(prev, n, x, y, h, w, sy, sx, fscale, u, v, y0, x0, y1, x1, ly, lx);
    o[6] = u; o[7] = v;
    const float fu = floorf(u), fv = floorf(v);
    const float xw = u - fu, yw = v - fv;
    const float wa = (1.f - xw) * (1.f - yw), wb = (1.f - xw) * yw, wc = xw * (1.f - yw), wd = xw * yw;
    const int xi = x + (int)fu, yi = y + (int)fv;
    const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1);
    const int ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
    const float4 Ia = reinterpret_cast<const float4*>(second)[sb + (long)ya * W + xa];
    const float4 Ib = reinterpret_cast<const float4*>(second)[sb + (long)yb * W + xa];
    const float4 Ic = reinterpret_cast<const float4*>(second)[sb + (long)ya * W + xb];
    const float4 Id = reinterpret_cast<const float4*>(second)[sb + (long)yb * W + xb];
    const float w0 = ((wa * Ia.x + wb * Ib.x) + wc * Ic.x) + wd * Id.x;
    const float w1 = ((wa * Ia.y + wb * Ib.y) + wc * Ic.y) + wd * Id.y;
    const float w2 = ((wa * Ia.z + wb * Ib.z) + wc * Ic.z) + wd * Id.z;
    o[8] = w0; o[9] = w1; o[10] = w2;
    o[11] = fabsf(w0 - a.x); o[12] = fabsf(w1 - a.y); o[13] = fabsf(w2 - a.z);
  }
}

__global__ void stack_input_pair_bwd_kernel(const float* __restrict__ dout, int ldo, const float* __restrict__ first,
                                            const float* __restrict__ second, const float* __restrict__ prev,
                                            float* __restrict__ d_prev, int N, int H, int W, int h, int w, float fscale) {
  const long npx = (long)N * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < npx; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int n = (int)(i / ((long)W * H));
    const long sb = (long)n * H * W;
    const float4 a = reinterpret_cast<const float4*>(first)[i];
    float u, v, ly, lx;
    int y0, x0, y1, x1;
    upsampled_flow(prev, n, x, y, h, w, sy, sx, fscale, u, v, y0, x0, y1, x1, ly, lx);
    const float fu = floorf(u), fv = floorf(v);
    const float xw = u - fu, yw = v - fv;
    const float wa = (1.f - xw) * (1.f - yw), wb = (1.f - xw) * yw, wc = xw * (1.f - yw), wd = xw * yw;
    const int xi = x + (int)fu, yi = y + (int)fv;
    const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1);
    const int ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
    const float4 Ia = reinterpret_cast<const float4*>(second)[sb + (long)ya * W + xa];
    const float4 Ib = reinterpret_cast<const float4*>(second)[sb + (long)yb * W + xa];
    const float4 Ic = reinterpret_cast<const float4*>(second)[sb + (long)ya * W + xb];
    const float4 Id = reinterpret_cast<const float4*>(second)[sb + (long)yb * W + xb];
    const float* gq = dout + i * ldo;
    const float ia[3] = {Ia.x, Ia.y, Ia.z}, ib[3] = {Ib.x, Ib.y, Ib.z}, ic[3] = {Ic.x, Ic.y, Ic.z}, id[3] = {Id.x, Id.y, Id.z};
    const float fa[3] = {a.x, a.y, a.z};
    float du = gq[6], dv = gq[7];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float wv = ((wa * ia[c] + wb * ib[c]) + wc * ic[c]) + wd * id[c];
      const float df = wv - fa[c];
      const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
      const float gc = gq[8 + c] + sg * gq[11 + c];
      du += gc * ((ic[c] - ia[c]) * (1.f - yw) + (id[c] - ib[c]) * yw);
      dv += gc * ((ib[c] - ia[c]) * (1.f - xw) + (id[c] - ic[c]) * xw);
    }
    du *= fscale;
    dv *= fscale;
    float* dp = d_prev + (long)n * h * w * 2;
    const float wtl = (1.f - lx) * (1.f - ly), wtr = lx * (1.f - ly), wbl = (1.f - lx) * ly, wbr = lx * ly;
    atomicAdd(dp + ((long)y0 * w + x0) * 2, du * wtl); atomicAdd(dp + ((long)y0 * w + x0) * 2 + 1, dv * wtl);
    atomicAdd(dp + ((long)y0 * w + x1) * 2, du * wtr); atomicAdd(dp + ((long)y0 * w + x1) * 2 + 1, dv * wtr);
    atomicAdd(dp + ((long)y1 * w + x0) * 2, du * wbl); atomicAdd(dp + ((long)y1 * w + x0) * 2 + 1, dv * wbl);
    atomicAdd(dp + ((long)y1 * w + x1) * 2, du * wbr); atomicAdd(dp + ((long)y1 * w + x1) * 2 + 1, dv * wbr);
  }
}

UNFLOW_API int unflow_stack_input_pair(const float* first4, const float* second4, const float* prev_flow2, float* out,
                                       int ld_out, int N, int H, int W, int h, int w, float flow_scale,
                                       unflow_stream_t stream) {
  if (!first4 || !second4 || !out) return UNFLOW_ERR_NULL;
  if (N <= 0 || H <= 0 || W <= 0 || ld_out < (prev_flow2 ? 14 : 6)) return UNFLOW_ERR_SHAPE;
  if (prev_flow2 && (h <= 0 || w <= 0)) return UNFLOW_ERR_SHAPE;
  stack_input_pair_kernel<<<stream_grid((long)N * H * W), 256, 0, as_stream(stream)>>>(first4, second4, prev_flow2, out, ld_out,
                                                                                       N, H, W, h, w, flow_scale);
  return launch_status();
}

UNFLOW_API int unflow_stack_input_pair_bwd(const float* d_out, int ld_out, const float* first4, const float* second4,
                                           const float* prev_flow2, float* d_prev_flow2, int N, int H, int W, int h, int w,
                                           float flow_scale, unflow_stream_t stream) {
  if (!d_out || !first4 || !second4 || !prev_flow2 || !d_prev_flow2) return UNFLOW_ERR_NULL;
  if (N <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || ld_out < 14) return UNFLOW_ERR_SHAPE;
  stack_input_pair_bwd_kernel<<<stream_grid((long)N * H * W), 256, 0, as_stream(stream)>>>(
      d_out, ld_out, first4, second4, prev_flow2, d_prev_flow2, N, H, W, h, w, flow_scale);
  return launch_status();
}
