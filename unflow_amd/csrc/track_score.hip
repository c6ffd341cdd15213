// Ground truth along a clip (core/inference.py FlowEstimator(..., sequence=..., track=..., ground_truth=True)): the
// ground-truth flows of the replay's pairs chained exactly as csrc/track.hip chains the estimated ones, ended at the ground truth's
// invalid / occluded pixels, and the replay's tracks (unflow_sequence_track's out_disp, out_alive) scored against them per slot.
//
// One thread per track, walking the valid pair slots in order, as sequence_track_kernel does and for its reason: four dependent
// rounds of four gathers (float2 flow + fp32 mask), hidden by the other waves of a 2048 x 256 grid.  What is new is the reduction.
// The trip count of the track loop is uniform per wave (lanes past N idle inside it), so per slot a wave counts each predicate
// with one ballot and sums its fp64 errors with a fixed shuffle tree; lane 0 adds the counts to the block's LDS words (integer
// atomics: exact) and the error to the wave's OWN LDS cell, one grid-stride pass after the other — a fixed order.  A block then
// adds its counts to the slot's accumulators in the caller's scratch (integer atomics again), writes its error sum there as a
// partial and takes a ticket; the last block takes the counts and sums the partials of every block, lane j taking blocks j, j + 64,
// ... and a fixed tree behind — the output kernel's idiom (csrc/inference.hip): the same bytes from every launch of a given grid,
// whichever block comes last.  It zeroes what it read and the ticket, so the scratch is zero again when the launch ends and a
// captured graph needs no memset node.
#include "common.h"
#include "image_warp.h"

namespace {

constexpr float TRACK_LIMIT = 1e6f;      // csrc/track.hip's: a displacement component of this magnitude (or not finite) ends a track
constexpr int TS_THREADS = 256, TS_WAVES = TS_THREADS / 64;
constexpr int TS_GRID = 2048;            // stream_grid's cap: the scratch holds a partial per block of the largest grid
constexpr int TS_COUNTS = 14;            // words 0..13 of a slot's scores are sums over the tracks
constexpr int TS_WORDS = 16;
constexpr int TS_MAX_B = 512;            // LDS: 88 bytes per slot

__device__ __forceinline__ bool ts_pair(const int* __restrict__ pairs, int i, int Hmax, int Wmax) {
  const int h = pairs[8 * i], w = pairs[8 * i + 1];
  return h > 0 && w > 0 && h <= Hmax && w <= Wmax;
}

__device__ __forceinline__ int ts_count(bool p) { return (int)__popcll(__ballot(p)); }

// The sum of the fp64 partials lane, lane + 64, ... below nb of one slot, in that order, and their zeroing.  Eight relaxed
// device-scope loads are in flight together (ordered, volatile loads cost one round trip each: about 0.3 ms of tail at 1820 blocks in
// the first build); eight, not all 32, so that the kernel keeps the registers of its gather loop.
__device__ __forceinline__ double ts_lane_sum(double* __restrict__ pp, int lane, int nb) {
  double s = 0.0;
  for (int j0 = lane; j0 < nb; j0 += 64 * 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int j = j0 + 64 * u;
      v[u] = j < nb ? __hip_atomic_load(pp + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) s += v[u];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int j = j0 + 64 * u;
      if (j < nb) pp[j] = 0.0;
    }
  }
  return s;
}

__global__ __launch_bounds__(TS_THREADS) void track_score_kernel(
    const float2* __restrict__ gt_flow, const float* __restrict__ gt_mask, const int* __restrict__ tab, int B, int Hmax, int Wmax,
    const int2* __restrict__ anchors, int Ncap, const float2* __restrict__ out_disp, const unsigned char* __restrict__ out_alive,
    float2* __restrict__ gt_disp, unsigned char* __restrict__ gt_alive, float2* __restrict__ out_gt_disp,
    unsigned char* __restrict__ out_gt_alive, int* __restrict__ scores, double* __restrict__ err, double* __restrict__ part_err,
    int* __restrict__ acc_cnt, unsigned* __restrict__ ticket) {
  extern __shared__ double lds[];
  double* lerr = lds;                                              // [B][TS_WAVES]
  int* lcnt = reinterpret_cast<int*>(lds + (long)B * TS_WAVES);    // [B][TS_COUNTS]
  __shared__ int last;
  const int* pairs = tab + 8 * (long)B;
  const int carry = tab[16 * (long)B], S = tab[16 * (long)B + 2];
  const long N = min(tab[16 * (long)B + 3], Ncap);
  if ((!anchors && S < 1) || N < 1) return;            // nothing tracked: nothing read, nothing written (uniform over the grid)
  for (int j = threadIdx.x; j < B * TS_WAVES; j += TS_THREADS) lerr[j] = 0.0;
  for (int j = threadIdx.x; j < B * TS_COUNTS; j += TS_THREADS) lcnt[j] = 0;
  __syncthreads();
  const long plane = (long)Hmax * Wmax;
  const long stride = (long)gridDim.x * TS_THREADS;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (long base = (long)blockIdx.x * TS_THREADS + wid * 64; base < N; base += stride) {   // uniform per wave
    const long n = base + lane;
    const bool in = n < N;
    float2 d = make_float2(0.f, 0.f);
    bool live = true;
    if (in && carry > 0) {                             // a later replay of the clip: continue from the state
      d = gt_disp[n];
      live = gt_alive[n] != 0;
    }
    int2 an = make_int2(0, 0);
    if (in && anchors) an = anchors[n];
    for (int i = 0; i < B; i++) {
      const int h = pairs[8 * i], w = pairs[8 * i + 1];
      if (h <= 0 || w <= 0 || h > Hmax || w > Wmax) continue;   // not a pair of the clip: nothing read, nothing written
      const int m = min(pairs[8 * i + 4], 2);          // the maps of this pair's ground truth; none: every track ends here
      if (in && live) {
        long ax = an.x, ay = an.y;
        if (!anchors) {                                // the dense grid of stride S over (h, w), row-major
          const long gw = ((long)w + S - 1) / S;
          const long gy = n / gw;
          ax = (n - gy * gw) * S;
          ay = gy * S;
        }
        live = m > 0 && ax >= 0 && ax < w && ay >= 0 && ay < h;
        if (live) {                                    // csrc/track.hip's step on map 0's flow and the last map's mask
          const int x = (int)ax, y = (int)ay;
          const IwTaps t = iw_sample(x, y, d.x, d.y, h, w, Wmax);
          const float2* f = gt_flow + i * plane;
          const float* o = gt_mask + ((long)(m - 1) * B + i) * plane;
          const float2 a = f[t.ia], b = f[t.ib], c = f[t.ic], e = f[t.id];
          const float oa = o[t.ia], ob = o[t.ib], oc = o[t.ic], od = o[t.id];
          // any tap of non-zero weight invalid (two maps: or occluded): the track ends where it is
          live = !(oa == 0.f || (t.yw > 0.f && ob == 0.f) || (t.xw > 0.f && oc == 0.f) ||
                   (t.xw > 0.f && t.yw > 0.f && od == 0.f));
          if (live) {
            d.x += ((t.wa * a.x + t.wb * b.x) + t.wc * c.x) + t.wd * e.x;
            d.y += ((t.wa * a.y + t.wb * b.y) + t.wc * c.y) + t.wd * e.y;
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
      float d2 = 0.f;
      bool pa = false;
      if (in) {
        const long q = (long)i * Ncap + n;
        out_gt_disp[q] = d;
        out_gt_alive[q] = live ? 1 : 0;
        const float2 p = out_disp[q];                  // used as it is: frozen where the predicted track is dead
        pa = out_alive[q] != 0;
        const float du = p.x - d.x, dv = p.y - d.y;
        d2 = du * du + dv * dv;
      }
      const bool ga = in && live, both = ga && pa;
      int c[TS_COUNTS];
      c[0] = ts_count(ga);
      c[1] = ts_count(in && pa);
      c[2] = ts_count(both);
      const float T[5] = {1.f, 4.f, 16.f, 64.f, 256.f};
#pragma unroll
      for (int k = 0; k < 5; k++) {
        const bool within = d2 < T[k];                  // a NaN compares false
        c[3 + k] = ts_count(ga && within);
        c[8 + k] = ts_count(both && within);
      }
      c[13] = ts_count(in && pa == live);
      double e = both ? (double)sqrtf(d2) : 0.0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o, 64);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < TS_COUNTS; k++)
          if (c[k]) atomicAdd(lcnt + i * TS_COUNTS + k, c[k]);
        lerr[i * TS_WAVES + wid] += e;                 // this wave's cell: its passes in order
      }
    }
    if (in) {
      gt_disp[n] = d;
      gt_alive[n] = live ? 1 : 0;
    }
  }
  // the block's counts into the slot's accumulators (integer atomics: exact in any order), its error sum as a partial; the ticket
  __syncthreads();
  const int nb = gridDim.x;
  for (int q = threadIdx.x; q < B * (TS_COUNTS + 1); q += TS_THREADS) {
    const int i = q / (TS_COUNTS + 1), k = q - i * (TS_COUNTS + 1);
    if (!ts_pair(pairs, i, Hmax, Wmax)) continue;
    if (k < TS_COUNTS) {
      const int c = lcnt[i * TS_COUNTS + k];
      if (c) atomicAdd(acc_cnt + i * TS_COUNTS + k, c);
    } else {
      const double* l = lerr + i * TS_WAVES;
      part_err[(long)i * TS_GRID + blockIdx.x] = ((l[0] + l[1]) + l[2]) + l[3];
    }
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == (unsigned)(nb - 1);
  __syncthreads();
  if (!last) return;
  // the last block: the accumulators are the counts (taken and zeroed in one exchange); a wave per slot sums the error partials,
  // lane j over blocks j, j + 64, ..., then the tree — a fixed order for a given grid — and zeroes them
  __threadfence();
  for (int q = threadIdx.x; q < B * TS_COUNTS; q += TS_THREADS) {
    const int i = q / TS_COUNTS, k = q - i * TS_COUNTS;
    if (ts_pair(pairs, i, Hmax, Wmax)) scores[(long)i * TS_WORDS + k] = atomicExch(acc_cnt + q, 0);
  }
  for (int i = wid; i < B; i += TS_WAVES) {
    if (!ts_pair(pairs, i, Hmax, Wmax)) continue;
    double s = ts_lane_sum(part_err + (long)i * TS_GRID, lane, nb);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) {
      err[i] = s;
      scores[(long)i * TS_WORDS + 14] = (int)N;
      scores[(long)i * TS_WORDS + 15] = 0;
    }
  }
  if (threadIdx.x == 0) *ticket = 0u;                  // ready for the next launch (graph replays included)
}

inline bool ts_shape_ok(int B, int Ncap) { return B >= 1 && B <= TS_MAX_B && Ncap >= 1; }

}  // namespace

UNFLOW_API size_t unflow_sequence_track_score_workspace_bytes(int B, int Ncap) {
  if (!ts_shape_ok(B, Ncap)) return 0;
  // per slot TS_GRID fp64 partials, then the B x TS_COUNTS int32 accumulators at the head of a region kept at TS_COUNTS x
  // TS_GRID int32 per slot, the ticket in the last 16 bytes
  return (size_t)B * TS_GRID * (sizeof(double) + TS_COUNTS * sizeof(int)) + 16;
}

UNFLOW_API int unflow_sequence_track_score(const float* gt_flow, const float* gt_mask, const int* tab, int B, int Hmax, int Wmax,
                                           const int* anchors, int Ncap, const float* out_disp, const unsigned char* out_alive,
                                           float* gt_disp, unsigned char* gt_alive, float* out_gt_disp,
                                           unsigned char* out_gt_alive, int* scores, double* err, void* workspace,
                                           unflow_stream_t stream) {
  if (!gt_flow || !gt_mask || !tab || !out_disp || !out_alive || !gt_disp || !gt_alive || !out_gt_disp || !out_gt_alive ||
      !scores || !err || !workspace)
    return UNFLOW_ERR_NULL;
  if (B < 1 || Ncap < 1 || Hmax < 1 || Wmax < 1) return UNFLOW_ERR_SHAPE;
  if ((long)Hmax * Wmax > 0x7fffffffL || B > TS_MAX_B) return UNFLOW_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return UNFLOW_ERR_UNSUPPORTED;
  double* part_err = reinterpret_cast<double*>(workspace);
  int* acc_cnt = reinterpret_cast<int*>(part_err + (size_t)B * TS_GRID);
  unsigned* ticket = reinterpret_cast<unsigned*>(acc_cnt + (size_t)B * TS_COUNTS * TS_GRID);
  const size_t lds = (size_t)B * (TS_WAVES * sizeof(double) + TS_COUNTS * sizeof(int));
  track_score_kernel<<<stream_grid(Ncap), TS_THREADS, lds, as_stream(stream)>>>(
      reinterpret_cast<const float2*>(gt_flow), gt_mask, tab, B, Hmax, Wmax, reinterpret_cast<const int2*>(anchors), Ncap,
      reinterpret_cast<const float2*>(out_disp), out_alive, reinterpret_cast<float2*>(gt_disp), gt_alive,
      reinterpret_cast<float2*>(out_gt_disp), out_gt_alive, scores, err, part_err, acc_cnt, ticket);
  return launch_status();
}
