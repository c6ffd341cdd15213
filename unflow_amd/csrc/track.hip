// Tracks along a clip (core/inference.py FlowEstimator(..., sequence=..., track=...)): where the pixels of a clip's
// first frame are in frame t — the forward flows of the replay's pairs chained through image_warp's bilinear taps — and whether
// each one is still visible.
//
// One thread per track, walking the replay's up to B pair slots in order: the steps of a track depend on each other (the taps of
// slot i + 1 are chosen by the displacement slot i left), the tracks do not.  Per step a track issues four float2 gathers (and
// four mask bytes) whose addresses are known together, so they are in flight together; what hides the chain of B such round trips
// is the other waves: at 256 threads per block and no LDS a CU holds its 8 waves per SIMD, and a grid of 2048 blocks is exactly
// what the chip keeps resident (256 CUs x 8 blocks).  A second track per thread would halve the waves to double the loads per
// wave: the same bytes in flight, more registers.  Consecutive tracks are consecutive anchors of a row, so with a smooth flow a
// wave's gathers fall on a few rows of the flow map; the state and the outputs are read and written coalesced along n.
// No atomics, no LDS, nothing that depends on the order of the blocks.
#include "common.h"
#include "image_warp.h"

namespace {

constexpr float TRACK_LIMIT = 1e6f;      // a displacement component of this magnitude (or not finite) ends a track

__global__ __launch_bounds__(256) void sequence_track_kernel(const float2* __restrict__ flow, const unsigned char* __restrict__ occ,
                                                             const int* __restrict__ tab, int B, int Hmax, int Wmax,
                                                             const int2* __restrict__ anchors, int Ncap, float2* __restrict__ disp,
                                                             unsigned char* __restrict__ alive, float2* __restrict__ out_disp,
                                                             unsigned char* __restrict__ out_alive) {
  const int* pairs = tab + 8 * (long)B;
  const int carry = tab[16 * (long)B], S = tab[16 * (long)B + 2];
  const long N = min(tab[16 * (long)B + 3], Ncap);
  if (!anchors && S < 1) return;                       // no grid: nothing to track
  const long plane = (long)Hmax * Wmax;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
    float2 d = make_float2(0.f, 0.f);
    bool live = true;
    if (carry > 0) {                                   // a later replay of the clip: continue from the state
      d = disp[n];
      live = alive[n] != 0;
    }
    int2 an = make_int2(0, 0);
    if (anchors) an = anchors[n];
    for (int i = 0; i < B; i++) {
      const int h = pairs[8 * i], w = pairs[8 * i + 1];
      if (h <= 0 || w <= 0 || h > Hmax || w > Wmax) continue;   // not a pair of the clip: nothing read, nothing written
      if (live) {
        long ax = an.x, ay = an.y;
        if (!anchors) {                                // the dense grid of stride S over (h, w), row-major
          const long gw = ((long)w + S - 1) / S;
          const long gy = n / gw;
          ax = (n - gy * gw) * S;
          ay = gy * S;
        }
        live = ax >= 0 && ax < w && ay >= 0 && ay < h;
        if (live) {
          const int x = (int)ax, y = (int)ay;
          const IwTaps t = iw_sample(x, y, d.x, d.y, h, w, Wmax);
          const float2* f = flow + i * plane;
          const float2 a = f[t.ia], b = f[t.ib], c = f[t.ic], e = f[t.id];
          if (occ) {                                   // any tap of non-zero weight occluded: the track ends where it is
            const unsigned char* o = occ + i * plane;
            const unsigned char oa = o[t.ia], ob = o[t.ib], oc = o[t.ic], od = o[t.id];
            live = !(oa || (t.yw > 0.f && ob) || (t.xw > 0.f && oc) || (t.xw > 0.f && t.yw > 0.f && od));
          }
          if (live) {
            d.x += ((t.wa * a.x + t.wb * b.x) + t.wc * c.x) + t.wd * e.x;
            d.y += ((t.wa * a.y + t.wb * b.y) + t.wc * c.y) + t.wd * e.y;
            // in the frame: 0 <= position <= size - 1, decided in integers; the magnitude test comes before any cast
            live = fabsf(d.x) < TRACK_LIMIT && fabsf(d.y) < TRACK_LIMIT;
            if (live) {
              const float fu = floorf(d.x), fv = floorf(d.y);
              const int xi = x + (int)fu, yi = y + (int)fv;
              live = xi >= 0 && (xi < w - 1 || (xi == w - 1 && d.x - fu == 0.f)) &&
                     yi >= 0 && (yi < h - 1 || (yi == h - 1 && d.y - fv == 0.f));
            }
          }
        }
      }
      out_disp[(long)i * Ncap + n] = d;
      out_alive[(long)i * Ncap + n] = live ? 1 : 0;
    }
    disp[n] = d;
    alive[n] = live ? 1 : 0;
  }
}

}  // namespace

UNFLOW_API int unflow_sequence_track(const float* flow_fw, const unsigned char* occ_fw, const int* tab, int B, int Hmax, int Wmax,
                                     const int* anchors, int Ncap, float* disp, unsigned char* alive, float* out_disp,
                                     unsigned char* out_alive, unflow_stream_t stream) {
  if (!flow_fw || !tab || !disp || !alive || !out_disp || !out_alive) return UNFLOW_ERR_NULL;
  if (B < 1 || Ncap < 1 || Hmax < 1 || Wmax < 1) return UNFLOW_ERR_SHAPE;
  if ((long)Hmax * Wmax > 0x7fffffffL || B > 0x7fffffff / 16) return UNFLOW_ERR_SHAPE;
  sequence_track_kernel<<<stream_grid(Ncap), 256, 0, as_stream(stream)>>>(
      reinterpret_cast<const float2*>(flow_fw), occ_fw, tab, B, Hmax, Wmax, reinterpret_cast<const int2*>(anchors), Ncap,
      reinterpret_cast<float2*>(disp), alive, reinterpret_cast<float2*>(out_disp), out_alive);
  return launch_status();
}
