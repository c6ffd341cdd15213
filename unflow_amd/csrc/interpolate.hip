// In-between frames along a clip (core/inference.py FlowEstimator(..., sequence=..., interpolate=n)): n frames
// between the two frames of every pair of a sequence replay, by a forward splat of the pair's colours along its flow (and, on a
// bidirectional estimator, of the second frame's colours along the backward flow), normalised by the splatted weight.
//
// The definition is include/unflow_hip.h's, and it is integer from the splat on: a source pixel's colour is quantised to 8.8 fixed
// point, its sub-pixel position to 1/64, its four tap weights are products of two 6-bit fractions and the direction weight, and the
// sums are 64-bit integers.  Integer addition is associative, so the order in which the atomics arrive cannot change a bit: two
// launches, and graph replay against eager launches, give identical bytes (forward_warp's idiom).  Three launches:
//   mid_splat_kernel       one thread per source pixel, in-between frame j and direction: 16 no-return 64-bit global atomics (four
//                          targets x {r, g, b, weight}).  The sums are four PLANES per (j, pair slot), so the 64 lanes of one
//                          atomic instruction — neighbouring source pixels, one tap, one sum — land on neighbouring 8-byte words
//                          wherever the flow is smooth, the access shape global atomics want (with the four sums of a target
//                          adjacent instead, one 8-byte word per 32-byte run, the entry measured 1.6x slower: DESIGN 7.16)
//   mid_normalise_kernel   one thread per target pixel and j: reads the four sums, writes the pixel — the quotient, or the
//                          temporal blend where the weight is below the hole threshold, counted — and zeroes what it read, so
//                          the accumulators are zero again for the next launch (no memset node in a graph)
//   mid_prev_kernel        the last new staged frame -> prev, for pair slot 0 of the NEXT replay; behind the splat, which reads prev
// No float atomics, no LDS.  The fp32 steps before the quantisation are rounded one by one (-ffp-contract=off), the two time
// fractions are formed on the host and passed by value: tests/mid_ref.py mirrors every step and the test is equality.
//
// unflow_sequence_interpolate_ordered is the same three launches with the splat and the normalisation instantiated
// "ordered": every source pixel's tap weights carry conf = 64 >> d, d from the summed colour difference between the pixel and the
// other frame at the end of its flow, a pixel at the floor (d == 6) or masked splats its own colour at conf 1, and a hole in
// one-direction mode takes the later frame's byte.  A few VALU operations on values the unordered splat has in registers already;
// nothing more is read.  The unordered instantiation compiles to what it was; tests/mid_order_ref.py mirrors the ordered one.
#include "common.h"
#include "image_warp.h"
#include "mid_common.h"

namespace {

constexpr float MID_LIMIT = 1e6f;                      // a flow component of this magnitude (or not finite) contributes nothing
constexpr unsigned long long MID_HOLE = 1024ull;       // weight sums below this are holes: a quarter of one source pixel's weight
constexpr int MID_ORDER_MAX = 4;                       // the steepness of the ordered splat: conf halves per 64 >> order grey levels
constexpr long MID_ORDER_PIXELS = 1L << 23;            // ordered: Hmax * Wmax up to here keeps every sum inside 63 bits
// The ordered weight word.  A hole is a target that too little of the source lands on, however well it agrees: the test is on the
// conf-less weight sum Sw0, as in the unordered entry, so the holes are that entry's holes.  Sw0 <= Sw <= 64 Sw0, so Sw < 1024 is
// a hole and Sw >= 65536 is none whatever Sw0 is, and in between Sw0 <= Sw < 2^16: 18 bits hold it exactly.  Sw < 2^24 taps *
// 4096 * 7 * 64 < 2^45 stays below bit 46, and what Sw0 carries out of bit 63 where it does not matter is gone without harm.
constexpr int MID_SW_BITS = 46;
constexpr unsigned long long MID_SW_MASK = (1ull << MID_SW_BITS) - 1, MID_SW_SURE = 64ull * MID_HOLE;

struct MidTimes {
  float t[MID_MAX], s[MID_MAX];                        // t = j / (n + 1), s = (n + 1 - j) / (n + 1), fp32 divisions of the host
};

template <typename T>
__device__ __forceinline__ float3 mid_load(const T* __restrict__ im, long px) {
  return make_float3((float)im[px * 3], (float)im[px * 3 + 1], (float)im[px * 3 + 2]);
}

template <bool ORD, typename T>
__device__ __forceinline__ void mid_splat(const T* __restrict__ here, const T* __restrict__ other, const float2* __restrict__ flow,
                                          const unsigned char* __restrict__ occ, int h, int w, int Wmax, float w_here,
                                          float w_other, unsigned long long a, unsigned long long* __restrict__ acc, long plane,
                                          int shift) {
  const int npx = h * w;                               // < 2^31 (the host checks Hmax * Wmax)
  for (int p = blockIdx.x * MID_THREADS + threadIdx.x; p < npx; p += gridDim.x * MID_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    const float2 f = flow[q];
    if (!(fabsf(f.x) < MID_LIMIT && fabsf(f.y) < MID_LIMIT)) continue;     // NaN compares false; before any integer conversion
    const float3 c = mid_load(here, q);
    float cc[3] = {c.x, c.y, c.z};
    unsigned long long aw = a;                         // ordered: the direction weight times conf
    if (!(occ && occ[q])) {
      const IwTaps t = iw_sample(x, y, f.x, f.y, h, w, Wmax);
      const float3 ta = mid_load(other, t.ia), tb = mid_load(other, t.ib), tc = mid_load(other, t.ic), td = mid_load(other, t.id);
      const float wp[3] = {((t.wa * ta.x + t.wb * tb.x) + t.wc * tc.x) + t.wd * td.x,
                           ((t.wa * ta.y + t.wb * tb.y) + t.wc * tc.y) + t.wd * td.y,
                           ((t.wa * ta.z + t.wb * tb.z) + t.wc * tc.z) + t.wd * td.z};
      bool blend = true;
      if constexpr (ORD) {
        // how far the two frames disagree along this pixel's flow, in summed grey levels; a NaN gives 765 (fminf's rule)
        const float e = fminf((fabsf(cc[0] - wp[0]) + fabsf(cc[1] - wp[1])) + fabsf(cc[2] - wp[2]), 765.f);
        const int d = min(((int)e) >> shift, 6);
        aw = a * (unsigned long long)(64 >> d);
        blend = d != 6;                                // at the floor: its own colour, as if it were masked
      }
      if (blend) {
#pragma unroll
        for (int k = 0; k < 3; k++) cc[k] = w_here * cc[k] + w_other * wp[k];
      }
    }
    const unsigned long long cq[3] = {(unsigned long long)mid_q(cc[0]), (unsigned long long)mid_q(cc[1]),
                                      (unsigned long long)mid_q(cc[2])};
    // the position in the in-between frame: this frame's pixel moved by the other frame's share of the way
    const float px = (float)x + w_other * f.x, py = (float)y + w_other * f.y;
    const float fx = floorf(px), fy = floorf(py);
    const int ix = (int)fx, iy = (int)fy;
    const int qx = (int)((px - fx) * 64.f), qy = (int)((py - fy) * 64.f);
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
#pragma unroll
      for (int dx = 0; dx < 2; dx++) {
        const int tx = ix + dx, ty = iy + dy;
        const int wx = dx ? qx : 64 - qx, wy = dy ? qy : 64 - qy;
        if (tx < 0 || tx >= w || ty < 0 || ty >= h || wx == 0 || wy == 0) continue;        // dropped, not clamped
        const unsigned long long W = (unsigned long long)(wx * wy) * aw;
        unsigned long long* s = acc + (long)ty * Wmax + tx;
        atomicAdd(s, W * cq[0]);
        atomicAdd(s + plane, W * cq[1]);
        atomicAdd(s + 2 * plane, W * cq[2]);
        if constexpr (ORD)                             // the weight word: Sw below, the conf-less weight (mod 2^18) on top
          atomicAdd(s + 3 * plane, W + (((unsigned long long)(wx * wy) * a) << MID_SW_BITS));
        else
          atomicAdd(s + 3 * plane, W);
      }
    }
  }
}

// grid (blocks, B, n * directions): block row b = pair slot, z = direction * n + (j - 1); shift = 6 - order (ordered only)
template <bool ORD>
__global__ __launch_bounds__(MID_THREADS) void mid_splat_kernel(const void* __restrict__ frames, const void* __restrict__ prev,
                                                                const int* __restrict__ tab, int B, int Hmax, int Wmax, int n,
                                                                MidTimes tm, const float* __restrict__ flow_fw,
                                                                const float* __restrict__ flow_bw,
                                                                const unsigned char* __restrict__ occ_fw,
                                                                const unsigned char* __restrict__ occ_bw,
                                                                unsigned long long* __restrict__ acc, int* __restrict__ out_holes,
                                                                int shift) {
  const int b = blockIdx.y, dir = blockIdx.z / n, j = blockIdx.z - dir * n + 1;
  const MidPair d = mid_pair(tab, B, b, Hmax, Wmax);
  if (d.h == 0) return;                                // uniform per block row: nothing read, nothing written
  if (dir == 0 && blockIdx.x == 0 && threadIdx.x == 0) out_holes[(long)(j - 1) * B + b] = 0;   // counted by the normalise pass
  const long plane = (long)Hmax * Wmax;
  const float t = tm.t[j - 1], s = tm.s[j - 1];
  const float2* flow = reinterpret_cast<const float2*>(dir ? flow_bw : flow_fw) + b * plane;
  const unsigned char* occ = occ_fw ? (dir ? occ_bw : occ_fw) + b * plane : nullptr;
  unsigned long long* a = acc + ((long)(j - 1) * B + b) * plane * 4;
  // forward: s im0 + t warp(im1), moved by t, weight n + 1 - j; backward: t im1 + s warp(im0), moved by s, weight j
  const float w_here = dir ? t : s, w_other = dir ? s : t;
  const unsigned long long wt = dir ? j : n + 1 - j;
  if (d.u8)
    mid_splat<ORD>(mid_frame<unsigned char>(frames, prev, plane, b, dir), mid_frame<unsigned char>(frames, prev, plane, b, 1 - dir),
                   flow, occ, d.h, d.w, Wmax, w_here, w_other, wt, a, plane, shift);
  else
    mid_splat<ORD>(mid_frame<float>(frames, prev, plane, b, dir), mid_frame<float>(frames, prev, plane, b, 1 - dir), flow, occ, d.h,
                   d.w, Wmax, w_here, w_other, wt, a, plane, shift);
}

// MODE 0: unordered.  1, 2: ordered, the weight word unpacked and the hole test on the conf-less weight; 2 is one direction, where
// a hole takes the later frame's byte — the frame in which a disoccluded pixel is visible.
template <int MODE, typename T>
__device__ __forceinline__ int mid_normalise(const T* __restrict__ im0, const T* __restrict__ im1, int h, int w, int Wmax, int n, int j,
                                             unsigned long long* __restrict__ acc, long plane, unsigned char* __restrict__ out) {
  int holes = 0;
  const int npx = h * w;
  const long long a0 = n + 1 - j, a1 = j, den = (long long)(n + 1) * 256, half = (long long)(n + 1) * 128;
  for (int p = blockIdx.x * MID_THREADS + threadIdx.x; p < npx; p += gridDim.x * MID_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    const unsigned long long word = acc[3 * plane + q];
    unsigned long long Sw = word;
    bool full = Sw >= MID_HOLE;
    if constexpr (MODE != 0) {
      Sw = word & MID_SW_MASK;
      full = Sw >= MID_HOLE && (Sw >= MID_SW_SURE || (word >> MID_SW_BITS) >= MID_HOLE);
    }
    unsigned char* o = out + q * 3;
    if (full) {
      const unsigned long long d = Sw * 256ull, r = Sw * 128ull;
      o[0] = (unsigned char)((acc[q] + r) / d);
      o[1] = (unsigned char)((acc[plane + q] + r) / d);
      o[2] = (unsigned char)((acc[2 * plane + q] + r) / d);
    } else if constexpr (MODE == 2) {                  // a hole: the later frame
      const float3 c1 = mid_load(im1, q);
      o[0] = (unsigned char)((mid_q(c1.x) + 128) / 256);
      o[1] = (unsigned char)((mid_q(c1.y) + 128) / 256);
      o[2] = (unsigned char)((mid_q(c1.z) + 128) / 256);
      holes++;
    } else {                                           // a hole: the temporal blend of the two frames
      const float3 c0 = mid_load(im0, q), c1 = mid_load(im1, q);
      o[0] = (unsigned char)((a0 * mid_q(c0.x) + a1 * mid_q(c1.x) + half) / den);
      o[1] = (unsigned char)((a0 * mid_q(c0.y) + a1 * mid_q(c1.y) + half) / den);
      o[2] = (unsigned char)((a0 * mid_q(c0.z) + a1 * mid_q(c1.z) + half) / den);
      holes++;
    }
    if (word) {                                        // every kept tap has a weight above 0: no weight, nothing to clean
#pragma unroll
      for (int k = 0; k < 4; k++) acc[k * plane + q] = 0ull;
    }
  }
  return holes;
}

// grid (blocks, B, n)
template <int MODE>
__global__ __launch_bounds__(MID_THREADS) void mid_normalise_kernel(const void* __restrict__ frames, const void* __restrict__ prev,
                                                                    const int* __restrict__ tab, int B, int Hmax, int Wmax, int n,
                                                                    unsigned long long* __restrict__ acc,
                                                                    unsigned char* __restrict__ out_mid, int* __restrict__ out_holes) {
  __shared__ int red[MID_THREADS / 64];
  const int b = blockIdx.y, j = blockIdx.z + 1;
  const MidPair d = mid_pair(tab, B, b, Hmax, Wmax);
  if (d.h == 0) return;
  const long plane = (long)Hmax * Wmax, img = ((long)(j - 1) * B + b) * plane;
  unsigned long long* a = acc + img * 4;
  int holes = d.u8 ? mid_normalise<MODE>(mid_frame<unsigned char>(frames, prev, plane, b, 0),
                                          mid_frame<unsigned char>(frames, prev, plane, b, 1), d.h, d.w, Wmax, n, j, a, plane,
                                          out_mid + img * 3)
                   : mid_normalise<MODE>(mid_frame<float>(frames, prev, plane, b, 0), mid_frame<float>(frames, prev, plane, b, 1), d.h,
                                          d.w, Wmax, n, j, a, plane, out_mid + img * 3);
  for (int o = 32; o > 0; o >>= 1) holes += __shfl_down(holes, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = holes;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int k = 0; k < MID_THREADS / 64; k++) total += red[k];
    if (total) atomicAdd(out_holes + (long)(j - 1) * B + b, total);    // an integer sum: exact, whatever the order
  }
}

}  // namespace

UNFLOW_API size_t unflow_sequence_interpolate_workspace_bytes(int n, int B, int Hmax, int Wmax) {
  if (!mid_shape_ok(n, B, Hmax, Wmax)) return 0;
  return (size_t)n * B * Hmax * Wmax * 4 * sizeof(unsigned long long);
}

namespace {

// order 0: unflow_sequence_interpolate; 1..4: unflow_sequence_interpolate_ordered's definition at that steepness
int mid_launch(int order, const void* frames, const int* tab, int B, int Hmax, int Wmax, int n, const float* flow_fw,
               const float* flow_bw, const unsigned char* occ_fw, const unsigned char* occ_bw, void* prev, void* workspace,
               unsigned char* out_mid, int* out_holes, unflow_stream_t stream) {
  if (!frames || !tab || !flow_fw || !prev || !workspace || !out_mid || !out_holes) return UNFLOW_ERR_NULL;
  if (!mid_shape_ok(n, B, Hmax, Wmax)) return UNFLOW_ERR_SHAPE;
  const int given = (flow_bw != nullptr) + (occ_fw != nullptr) + (occ_bw != nullptr);
  if (given != 0 && given != 3) return UNFLOW_ERR_SHAPE;
  MidTimes tm{};
  for (int j = 1; j <= n; j++) {
    tm.t[j - 1] = (float)j / (float)(n + 1);
    tm.s[j - 1] = (float)(n + 1 - j) / (float)(n + 1);
  }
  const hipStream_t st = as_stream(stream);
  const int blocks = stream_grid((long)Hmax * Wmax, MID_THREADS);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(workspace);
  const dim3 splat(blocks, B, n * (given ? 2 : 1)), norm(blocks, B, n);
  if (order)
    mid_splat_kernel<true><<<splat, MID_THREADS, 0, st>>>(frames, prev, tab, B, Hmax, Wmax, n, tm, flow_fw, flow_bw, occ_fw, occ_bw, acc,
                                                          out_holes, 6 - order);
  else
    mid_splat_kernel<false><<<splat, MID_THREADS, 0, st>>>(frames, prev, tab, B, Hmax, Wmax, n, tm, flow_fw, flow_bw, occ_fw, occ_bw, acc,
                                                           out_holes, 0);
  if (order && given)
    mid_normalise_kernel<1><<<norm, MID_THREADS, 0, st>>>(frames, prev, tab, B, Hmax, Wmax, n, acc, out_mid, out_holes);
  else if (order)
    mid_normalise_kernel<2><<<norm, MID_THREADS, 0, st>>>(frames, prev, tab, B, Hmax, Wmax, n, acc, out_mid, out_holes);
  else
    mid_normalise_kernel<0><<<norm, MID_THREADS, 0, st>>>(frames, prev, tab, B, Hmax, Wmax, n, acc, out_mid, out_holes);
  mid_prev_kernel<<<blocks, MID_THREADS, 0, st>>>(frames, tab, B, Hmax, Wmax, prev);
  return launch_status();
}

}  // namespace

UNFLOW_API int unflow_sequence_interpolate(const void* frames, const int* tab, int B, int Hmax, int Wmax, int n, const float* flow_fw,
                                           const float* flow_bw, const unsigned char* occ_fw, const unsigned char* occ_bw, void* prev,
                                           void* workspace, unsigned char* out_mid, int* out_holes, unflow_stream_t stream) {
  return mid_launch(0, frames, tab, B, Hmax, Wmax, n, flow_fw, flow_bw, occ_fw, occ_bw, prev, workspace, out_mid, out_holes, stream);
}

UNFLOW_API int unflow_sequence_interpolate_ordered(const void* frames, const int* tab, int B, int Hmax, int Wmax, int n,
                                                   const float* flow_fw, const float* flow_bw, const unsigned char* occ_fw,
                                                   const unsigned char* occ_bw, void* prev, void* workspace, unsigned char* out_mid,
                                                   int* out_holes, int order, unflow_stream_t stream) {
  if (order < 0 || order > MID_ORDER_MAX) return UNFLOW_ERR_SHAPE;
  // one tap adds less than 2^37 (4096 * 7 * 64 * 65280) and a target gets at most one tap per source pixel and direction: with
  // Hmax * Wmax <= 2^23 a colour sum stays below 2^62; refused before anything else is looked at
  if (order && (long)Hmax * Wmax > MID_ORDER_PIXELS) return UNFLOW_ERR_SHAPE;
  return mid_launch(order, frames, tab, B, Hmax, Wmax, n, flow_fw, flow_bw, occ_fw, occ_bw, prev, workspace, out_mid, out_holes, stream);
}
