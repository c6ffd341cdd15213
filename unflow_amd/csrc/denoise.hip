// Temporal denoising along a clip (core/inference.py FlowEstimator(..., sequence='bidirectional', denoise=...)): per
// pair of a sequence replay the later frame is averaged with its own history, fetched along the backward flow — a recursive,
// motion-compensated filter.  The history (an 8.8 colour and a count per pixel) lives on the device from replay to replay.
//
// The definition is include/unflow_hip.h's and it is integer everywhere but in the flow's validity test and one rintf per
// component; tests/denoise_ref.py mirrors every step and the test is equality.  A history pixel is ONE 8-byte word {r, g, b, n} of
// uint16, so a tap is one load and a row of pixels is coalesced.  The taps of a slot read the history BEFORE the slot at displaced
// positions, so the update is never in place: two slabs in the workspace take turns (slot i reads slab i & 1 and writes the other
// one), a launch in front fills slab 0 from the state (or from the clip's first frame) and one behind copies slab B & 1 back.
// 2 B + 2 launches, the kernel boundaries being the only hand-off between workgroups:
//   dn_begin_kernel     state -> slab 0; with carry source 0 the (h, w) corner of frame-table slot 0 becomes {q(colour), n = 1}.
//   dn_level_kernel     per slot, at most 512 blocks walking the pixels of (h, w) with a stride: the prediction, its L1 distance from the frame, the 256 bins of
//                       E in LDS (integer LDS atomics), then one global integer add per non-empty bin and block.
//   dn_filter_kernel    per slot, over the whole [Hmax][Wmax] plane: every block derives M and t from the slot's 256 words (a scan
//                       through shuffles and LDS), a pixel of (h, w) is predicted again and blended, its new history goes to the
//                       other slab and its byte to out_den; a pixel outside (h, w) — every pixel of a slot that is no pair — is
//                       copied from slab to slab.  The three counts: registers, a shuffle tree per wave, LDS, one integer atomic
//                       per count and block.
//   dn_end_kernel       slab B & 1 -> state, and the histogram words back to zero: no memset node in a captured graph.
// No float atomics, no float reductions, no inline assembly.  tol and depth travel by value.
#include "common.h"
#include "mid_common.h"

namespace {

constexpr int DN_THREADS = 256, DN_WAVES = DN_THREADS / 64;
constexpr int DN_BINS = 256;
constexpr int DN_BLOCKS = 512;                         // the two per-slot grids: every block ends with atomics on the slot's few lines
constexpr int DN_MAX = 4096;                           // Hmax, Wmax: PX, PY < 2^19 (the ranges: include/unflow_hip.h)
typedef unsigned long long dn_word;                    // {r, g, b, n}: four uint16, r in the low bits

__device__ __forceinline__ dn_word dn_pack(unsigned r, unsigned g, unsigned b, unsigned n) {
  return (dn_word)(r & 0xffffu) | ((dn_word)(g & 0xffffu) << 16) | ((dn_word)(b & 0xffffu) << 32) | ((dn_word)(n & 0xffffu) << 48);
}

// q of staged frame `slot` at element e (3 * pixel + channel): uint8 and fp32 frames take the one path through mid_q
__device__ __forceinline__ unsigned dn_q(const void* __restrict__ frames, bool u8, long e) {
  const float c = u8 ? (float)reinterpret_cast<const unsigned char*>(frames)[e] : reinterpret_cast<const float*>(frames)[e];
  return (unsigned)mid_q(c);
}

// What both passes know of pixel (x, y) of a pair slot: cur, and for a pixel that is not FRESH pred, np and e
struct DnPixel {
  unsigned cur[3], pred[3], np, e;
  bool fresh;
};
__device__ __forceinline__ DnPixel dn_predict(const void* __restrict__ frame, bool u8, const float2* __restrict__ bw,
                                               const unsigned char* __restrict__ occ, const dn_word* __restrict__ hist, int Wmax, int h,
                                               int w, int x, int y) {
  DnPixel px;
  const long q = (long)y * Wmax + x;
#pragma unroll
  for (int k = 0; k < 3; k++) px.cur[k] = dn_q(frame, u8, q * 3 + k);
  px.pred[0] = px.pred[1] = px.pred[2] = px.np = px.e = 0;
  px.fresh = true;
  const float2 f = bw[q];
  if (!(fabsf(f.x) < 4096.f && fabsf(f.y) < 4096.f)) return px;     // not VALID: tested before any conversion
  const int PX = (x << 6) + (int)rintf(f.x * 64.f), PY = (y << 6) + (int)rintf(f.y * 64.f);
  if (PX < 0 || PX > ((w - 1) << 6) || PY < 0 || PY > ((h - 1) << 6)) return px;   // not INSIDE
  if (occ[q]) return px;
  px.fresh = false;
  const int ix = PX >> 6, iy = PY >> 6;
  const unsigned qx = PX & 63, qy = PY & 63;
  const int jx = min(ix + 1, w - 1), jy = min(iy + 1, h - 1);
  const dn_word a = hist[(long)iy * Wmax + ix], b = hist[(long)iy * Wmax + jx], c = hist[(long)jy * Wmax + ix],
                d = hist[(long)jy * Wmax + jx];
  const unsigned waa = (64 - qx) * (64 - qy), wba = qx * (64 - qy), wab = (64 - qx) * qy, wbb = qx * qy;
  unsigned e = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int sh = 16 * k;
    const unsigned s = waa * (unsigned)((a >> sh) & 0xffff) + wba * (unsigned)((b >> sh) & 0xffff) +
                       wab * (unsigned)((c >> sh) & 0xffff) + wbb * (unsigned)((d >> sh) & 0xffff);   // <= 2^12 (2^16 - 1)
    px.pred[k] = (s + 2048u) >> 12;
    e += px.pred[k] > px.cur[k] ? px.pred[k] - px.cur[k] : px.cur[k] - px.pred[k];
  }
  px.e = e;
  px.np = min(min((unsigned)(a >> 48), (unsigned)(b >> 48)), min((unsigned)(c >> 48), (unsigned)(d >> 48)));
  return px;
}

__global__ __launch_bounds__(DN_THREADS) void dn_begin_kernel(const void* __restrict__ frames, const int* __restrict__ tab, int B,
                                                              int Hmax, int Wmax, const dn_word* __restrict__ state,
                                                              dn_word* __restrict__ slab) {
  int h0 = 0, w0 = 0;
  if (tab[16 * (long)B] <= 0 && tab[0] > 0 && tab[1] > 0 && tab[0] <= Hmax && tab[1] <= Wmax) {   // the clip starts here
    h0 = tab[0];
    w0 = tab[1];
  }
  const bool u8 = tab[5] != 0;
  const int plane = Hmax * Wmax;
  for (int p = blockIdx.x * DN_THREADS + threadIdx.x; p < plane; p += gridDim.x * DN_THREADS) {
    const int y = p / Wmax, x = p - y * Wmax;
    dn_word v;
    if (y < h0 && x < w0)
      v = dn_pack(dn_q(frames, u8, (long)p * 3), dn_q(frames, u8, (long)p * 3 + 1), dn_q(frames, u8, (long)p * 3 + 2), 1);
    else
      v = state[p];
    slab[p] = v;
  }
}

__global__ __launch_bounds__(DN_THREADS) void dn_level_kernel(const void* __restrict__ frames, const float2* __restrict__ flow,
                                                              const unsigned char* __restrict__ occ, const int* __restrict__ tab, int B,
                                                              int b, int Hmax, int Wmax, const dn_word* __restrict__ hist,
                                                              int* __restrict__ bins, int* __restrict__ out_stats) {
  __shared__ int lds[DN_BINS];
  const MidPair d = mid_pair(tab, B, b, Hmax, Wmax);
  if (d.h <= 0) return;                                // uniform: nothing read, nothing written
  const int npx = d.h * d.w;                           // <= 2^24
  if ((int)(blockIdx.x * DN_THREADS) >= npx) return;
  if (blockIdx.x == 0 && threadIdx.x >= 3 && threadIdx.x < 8) out_stats[8 * (long)b + threadIdx.x] = 0;   // counted by the filter pass
  lds[threadIdx.x] = 0;
  __syncthreads();
  const long plane = (long)Hmax * Wmax;
  const void* frame = d.u8 ? (const void*)(reinterpret_cast<const unsigned char*>(frames) + b * plane * 3)
                           : (const void*)(reinterpret_cast<const float*>(frames) + b * plane * 3);
  for (int p = blockIdx.x * DN_THREADS + threadIdx.x; p < npx; p += gridDim.x * DN_THREADS) {
    const int y = p / d.w, x = p - y * d.w;
    const DnPixel px = dn_predict(frame, d.u8, flow + b * plane, occ + b * plane, hist, Wmax, d.h, d.w, x, y);
    if (!px.fresh) atomicAdd(lds + min(px.e >> 8, 255u), 1);
  }
  __syncthreads();
  const int v = lds[threadIdx.x];
  if (v) atomicAdd(bins + DN_BINS * (long)b + threadIdx.x, v);   // integer: exact in any order
}

__global__ __launch_bounds__(DN_THREADS) void dn_filter_kernel(const void* __restrict__ frames, const float2* __restrict__ flow,
                                                               const unsigned char* __restrict__ occ, const int* __restrict__ tab,
                                                               int B, int b, int Hmax, int Wmax, int tol, int depth,
                                                               const dn_word* __restrict__ hist, dn_word* __restrict__ next,
                                                               const int* __restrict__ bins, unsigned char* __restrict__ out_den,
                                                               int* __restrict__ out_stats) {
  __shared__ int part[DN_WAVES], below[DN_WAVES], cnt[3];
  const MidPair d = mid_pair(tab, B, b, Hmax, Wmax);
  const int plane = Hmax * Wmax;
  if (d.h <= 0) {                                      // no pair: the history passes through
    for (int p = blockIdx.x * DN_THREADS + threadIdx.x; p < plane; p += gridDim.x * DN_THREADS) next[p] = hist[p];
    return;
  }
  // M and t from the slot's histogram: an inclusive scan of the 256 bins, one per thread
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int cum = bins[DN_BINS * (long)b + threadIdx.x];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int n = __shfl_up(cum, off, 64);
    if (lane >= off) cum += n;
  }
  if (lane == 63) part[wid] = cum;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  int eligible = 0;
#pragma unroll
  for (int j = 0; j < DN_WAVES; j++) {
    if (j < wid) cum += part[j];
    eligible += part[j];
  }
  const int half = (eligible + 1) / 2;
  const int nb = (int)__popcll(__ballot(cum < half));  // the bins in front of M: cum is monotone
  if (lane == 0) below[wid] = nb;
  __syncthreads();
  const int M = ((below[0] + below[1]) + below[2]) + below[3];
  int t = tol;
  if (tol < 0) {
    t = 0;
    while (t < 4 && (8 << t) < 2 * M) t++;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out_stats[8 * (long)b + 0] = t;
    out_stats[8 * (long)b + 1] = M;
    out_stats[8 * (long)b + 2] = eligible;
  }
  const void* frame = d.u8 ? (const void*)(reinterpret_cast<const unsigned char*>(frames) + (long)b * plane * 3)
                           : (const void*)(reinterpret_cast<const float*>(frames) + (long)b * plane * 3);
  int c_fresh = 0, c_rej = 0, c_n = 0;
  for (int p = blockIdx.x * DN_THREADS + threadIdx.x; p < plane; p += gridDim.x * DN_THREADS) {
    const int y = p / Wmax, x = p - y * Wmax;
    if (y >= d.h || x >= d.w) {
      next[p] = hist[p];
      continue;
    }
    const DnPixel px = dn_predict(frame, d.u8, flow + (long)b * plane, occ + (long)b * plane, hist, Wmax, d.h, d.w, x, y);
    unsigned neff = 0;
    if (px.fresh) {
      c_fresh++;
    } else {
      const unsigned dd = min(px.e >> (11 + t), 6u);
      if (dd == 6)
        c_rej++;
      else
        neff = px.np >> dd;
    }
    unsigned A[3];
    unsigned char* o = out_den + ((long)b * plane + p) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      A[k] = (neff * px.pred[k] + px.cur[k] + ((neff + 1) >> 1)) / (neff + 1);
      o[k] = (unsigned char)((A[k] + 128) >> 8);
    }
    const unsigned nn = min(neff + 1, (unsigned)depth);
    c_n += (int)nn;
    next[p] = dn_pack(A[0], A[1], A[2], nn);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c_fresh += __shfl_down(c_fresh, off, 64);
    c_rej += __shfl_down(c_rej, off, 64);
    c_n += __shfl_down(c_n, off, 64);
  }
  if (lane == 0) {
    if (c_fresh) atomicAdd(cnt + 0, c_fresh);
    if (c_rej) atomicAdd(cnt + 1, c_rej);
    if (c_n) atomicAdd(cnt + 2, c_n);
  }
  __syncthreads();
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(out_stats + 8 * (long)b + 3 + threadIdx.x, cnt[threadIdx.x]);   // integer: exact
}

__global__ __launch_bounds__(DN_THREADS) void dn_end_kernel(int B, int Hmax, int Wmax, const dn_word* __restrict__ slab,
                                                            dn_word* __restrict__ state, int* __restrict__ bins) {
  const int plane = Hmax * Wmax, words = B * DN_BINS;  // B <= 65535: below 2^24
  for (int p = blockIdx.x * DN_THREADS + threadIdx.x; p < plane; p += gridDim.x * DN_THREADS) state[p] = slab[p];
  for (int p = blockIdx.x * DN_THREADS + threadIdx.x; p < words; p += gridDim.x * DN_THREADS) bins[p] = 0;
}

inline bool dn_shape_ok(int B, int Hmax, int Wmax) {
  return B >= 1 && B <= 65535 && Hmax >= 1 && Wmax >= 1 && Hmax <= DN_MAX && Wmax <= DN_MAX;
}

}  // namespace

UNFLOW_API size_t unflow_sequence_denoise_workspace_bytes(int B, int Hmax, int Wmax) {
  if (!dn_shape_ok(B, Hmax, Wmax)) return 0;
  return (size_t)B * DN_BINS * sizeof(int) + 2 * (size_t)Hmax * Wmax * sizeof(dn_word);
}

UNFLOW_API int unflow_sequence_denoise(const void* frames, const int* tab, int B, int Hmax, int Wmax, const float* flow_bw,
                                       const unsigned char* occ_bw, int tol, int depth, void* state, void* workspace,
                                       unsigned char* out_den, int* out_stats, unflow_stream_t stream) {
  if (!frames || !tab || !flow_bw || !occ_bw || !state || !workspace || !out_den || !out_stats) return UNFLOW_ERR_NULL;
  if (!dn_shape_ok(B, Hmax, Wmax)) return UNFLOW_ERR_SHAPE;
  if (tol < -1 || tol > 4 || depth < 1 || depth > 64) return UNFLOW_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(flow_bw)) & 7)
    return UNFLOW_ERR_UNSUPPORTED;                     // the history words and float2
  const hipStream_t st = as_stream(stream);
  const long pixels = (long)Hmax * Wmax;
  int* bins = reinterpret_cast<int*>(workspace);
  dn_word* slab[2] = {reinterpret_cast<dn_word*>(bins + (size_t)B * DN_BINS), nullptr};
  slab[1] = slab[0] + pixels;
  const float2* flow = reinterpret_cast<const float2*>(flow_bw);
  const int grid = stream_grid(pixels, DN_THREADS);
  // the per-slot passes: a block per 256 pixels ends 1920 blocks of a 384 x 1280 slot with up to 256 + 3 integer atomics each on
  // the slot's nine lines, and those, not the pixels, set the time; two blocks per CU walk the slot with a stride
  const int slot_grid = grid < DN_BLOCKS ? grid : DN_BLOCKS;
  dn_begin_kernel<<<grid, DN_THREADS, 0, st>>>(frames, tab, B, Hmax, Wmax, reinterpret_cast<const dn_word*>(state), slab[0]);
  for (int b = 0; b < B; b++) {
    dn_level_kernel<<<slot_grid, DN_THREADS, 0, st>>>(frames, flow, occ_bw, tab, B, b, Hmax, Wmax, slab[b & 1], bins, out_stats);
    dn_filter_kernel<<<slot_grid, DN_THREADS, 0, st>>>(frames, flow, occ_bw, tab, B, b, Hmax, Wmax, tol, depth, slab[b & 1],
                                                  slab[(b + 1) & 1], bins, out_den, out_stats);
  }
  dn_end_kernel<<<grid, DN_THREADS, 0, st>>>(B, Hmax, Wmax, slab[B & 1], reinterpret_cast<dn_word*>(state), bins);
  return launch_status();
}
