// Held-out scores of the in-between frames (core/inference.py FlowEstimator(..., sequence=..., interpolate=n, held_out=True);
// DESIGN 7.18): per pair slot and in-between frame j, the squared error and the 8x8-window SSIM of three candidates — the
// interpolated frame (out_mid), the temporal blend and the nearest frame — against the staged truth frame.  The definition is
// include/unflow_hip.h's; tests/mid_score_ref.py mirrors it.
//
// One launch scores, a second copies the last new frame into this entry's own prev (unflow_sequence_interpolate's has been
// overwritten by the time this entry runs).  The scoring launch is a stencil on 32 x 16 tiles of window origins with a 7-pixel
// halo to the right and below, a block per tile of a slot, grid-stride over the tiles under a block cap:
//   per tile    the 8.8 quantised colours of the two frames -> LDS (16 bit), once for all j
//   per j       truth and out_mid bytes -> LDS (loaded one frame ahead, while the frame before is scored); blend and nearest bytes
//               formed from the quantised colours, once per pixel
//   per channel 8-wide row sums of y, y^2 and per kind x, x^2, x y (11 integers) for every row of the halo region -> LDS;
//               then per origin the 8-high column sums of those, the three SSIMs in fp64, and the squared errors of the tile's
//               own pixels (not the halo's: every pixel counts once)
// Reductions.  The squared errors are integers: wave shuffles, LDS and global integer atomics, exact in any order.  The SSIM sums
// are fp64 and take a fixed route: a thread's terms in order (channel, then origin), a shuffle tree per wave, the four waves in
// order, the block's tiles in order into LDS, the block's sums as partials in the caller's scratch, a ticket, and the last block
// sums the partials, lane l taking blocks l, l + 64, ... and a tree behind (csrc/track_score.hip's idiom).  The last block zeroes
// what it read and the ticket: the scratch is zero again when the launch ends, a captured graph needs no memset node.
#include "common.h"
#include "mid_common.h"

namespace {

constexpr int MS_TX = 32, MS_TY = 16;                  // window origins (and own pixels) per tile
constexpr int MS_HX = MS_TX + 7, MS_HY = MS_TY + 7;    // with the halo
constexpr int MS_PITCH = 40;                           // LDS row pitch of the byte and 16-bit tiles, in elements
constexpr int MS_CAP = 512;                            // blocks per slot at the most, a multiple of 64: more tiles, grid-stride loop
constexpr int MS_KINDS = 3;                            // 0 interpolated, 1 blend, 2 nearest
constexpr int MS_ROWSUMS = 2 + 3 * MS_KINDS;           // Sy, Syy, then per kind Sx, Sxx, Sxy
constexpr int MS_WAVES = MID_THREADS / 64;
constexpr double MS_C1 = 26634.24, MS_C2 = 239708.16;  // 4096 (0.01 * 255)^2, 4096 (0.03 * 255)^2

constexpr int MS_REGION = MS_HY * MS_HX;                                      // pixels of a tile with its halo
constexpr int MS_PASSES = (MS_REGION + MID_THREADS - 1) / MID_THREADS;        // region pixels per thread
// rows of the LDS tiles: the region's, and below them the rows that the threads past the region's end fill, never read — every
// thread loads and stores MS_PASSES pixels without a branch
constexpr int MS_LY = (MS_PASSES * MID_THREADS + MS_HX - 1) / MS_HX;

// The three values of a pixel as they wait in registers between their load and their use, and their 8.8 fixed point: mid_q, which
// for a byte is the byte times 256.  Nothing is unpacked where the load is issued (the channels of a byte pixel are taken apart
// where they are used), so the wait for a load stands where its values are needed and not where it was issued.
template <typename T>
struct MsRaw;
template <>
struct MsRaw<float> {
  float v[3];
  __device__ __forceinline__ void load(const float* __restrict__ p) {
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
  }
  __device__ __forceinline__ unsigned q(int k) const { return (unsigned)mid_q(v[k]); }
};
template <>
struct MsRaw<unsigned char> {
  unsigned lo, hi;                                      // bytes 0 and 1 as they lie in memory (little endian), byte 2: a register each
  __device__ __forceinline__ void load(const unsigned char* __restrict__ p) {
    unsigned short two;
    __builtin_memcpy(&two, p, 2);
    lo = two;
    hi = p[2];
  }
  __device__ __forceinline__ unsigned byte(int k) const { return k == 0 ? lo & 0xffu : k == 1 ? lo >> 8 : hi; }
  __device__ __forceinline__ unsigned q(int k) const { return byte(k) << 8; }
};

// Where region pixel p of the tile at (x0, y0) lies in its image, clamped into the (h, w) frame so that the load needs no branch
// (the value of a pixel outside the frame is dropped afterwards; p past the region's end lands in the LDS rows that are never
// read): the loads of a thread's MS_PASSES pixels are all in flight together instead of one round trip after the other.
struct MsPixel {
  int ry, rx;
  long px;
  bool in;
};
__device__ __forceinline__ MsPixel ms_pixel(int p, int x0, int y0, int h, int w, int Wmax) {
  MsPixel m;
  m.ry = p / MS_HX;
  m.rx = p - m.ry * MS_HX;
  m.in = x0 + m.rx < w && y0 + m.ry < h;
  m.px = (long)min(y0 + m.ry, h - 1) * Wmax + min(x0 + m.rx, w - 1);
  return m;
}

// The LDS of a block
struct MsShared {
  unsigned short q0[3][MS_LY][MS_PITCH], q1[3][MS_LY][MS_PITCH];        // the two frames' 8.8 colours
  unsigned char by[1 + MS_KINDS][3][MS_LY][MS_PITCH];                   // 0 truth, 1 + kind the candidates
  int rs[MS_ROWSUMS][MS_HY][MS_TX];
  double wsum[MS_WAVES][MS_KINDS], bsum[MID_MAX * MS_KINDS];
  unsigned long long bsse[MID_MAX * MS_KINDS];
  int last;
};

// The tiles of this block, every j: the block's sums into S.bsum (fp64, the tiles in order) and S.bsse (integers)
template <typename T>
__device__ __forceinline__ void ms_tiles(MsShared& S, const T* __restrict__ im0, const T* __restrict__ im1,
                                         const T* __restrict__ truth, const unsigned char* __restrict__ out_mid, int h, int w,
                                         int Wmax, int n, long plane_b, long plane_j) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_x = (w + MS_TX - 1) / MS_TX, tiles = tiles_x * ((h + MS_TY - 1) / MS_TY);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {          // uniform per block
    const int ty = tile / tiles_x, x0 = (tile - ty * tiles_x) * MS_TX, y0 = ty * MS_TY;
    MsPixel m[MS_PASSES];
#pragma unroll
    for (int it = 0; it < MS_PASSES; it++) m[it] = ms_pixel(tid + it * MID_THREADS, x0, y0, h, w, Wmax);
    // truth and out_mid of frame j are loaded one frame ahead: frame 1's with the two frames, frame j + 1's before frame j is
    // scored, so that only the first round trip of a tile is waited for
    MsRaw<T> t[MS_PASSES];
    MsRaw<unsigned char> o[MS_PASSES];
    {
      MsRaw<T> a[MS_PASSES], c[MS_PASSES];
#pragma unroll
      for (int it = 0; it < MS_PASSES; it++) {
        a[it].load(im0 + m[it].px * 3);
        c[it].load(im1 + m[it].px * 3);
        t[it].load(truth + (plane_b + m[it].px) * 3);
        o[it].load(out_mid + (plane_b + m[it].px) * 3);
      }
      __syncthreads();                                                    // the last tile's readers are done
#pragma unroll
      for (int it = 0; it < MS_PASSES; it++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          S.q0[k][m[it].ry][m[it].rx] = (unsigned short)(m[it].in ? a[it].q(k) : 0u);
          S.q1[k][m[it].ry][m[it].rx] = (unsigned short)(m[it].in ? c[it].q(k) : 0u);
        }
      }
    }
    for (int j = 1; j <= n; j++) {
      // every term of the blend is below 2^20: 32-bit arithmetic gives the definition's 64-bit values
      const unsigned a0 = n + 1 - j, a1 = j, den = (unsigned)(n + 1) * 256u, half = (unsigned)(n + 1) * 128u;
      const bool near0 = 2 * j <= n + 1;
      __syncthreads();                                                    // q0 / q1 written; the last j's readers are done
#pragma unroll
      for (int it = 0; it < MS_PASSES; it++) {
        const int ry = m[it].ry, rx = m[it].rx;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const unsigned u = S.q0[k][ry][rx], v = S.q1[k][ry][rx];
          S.by[0][k][ry][rx] = (unsigned char)(m[it].in ? (t[it].q(k) + 128u) >> 8 : 0u);
          S.by[1][k][ry][rx] = (unsigned char)(m[it].in ? o[it].byte(k) : 0u);
          S.by[2][k][ry][rx] = (unsigned char)((a0 * u + a1 * v + half) / den);
          S.by[3][k][ry][rx] = (unsigned char)(((near0 ? u : v) + 128u) >> 8);
        }
      }
      if (j < n) {                                                        // frame j + 1, in flight while frame j is scored
        const long img = plane_b + (long)j * plane_j;
#pragma unroll
        for (int it = 0; it < MS_PASSES; it++) {
          t[it].load(truth + (img + m[it].px) * 3);
          o[it].load(out_mid + (img + m[it].px) * 3);
        }
      }
      double ssim[MS_KINDS] = {0.0, 0.0, 0.0};
      unsigned long long sse[MS_KINDS] = {0ull, 0ull, 0ull};
      for (int c = 0; c < 3; c++) {
        __syncthreads();                                                  // the bytes written; the last channel's row sums read
        for (int p = tid; p < MS_HY * MS_TX; p += MID_THREADS) {
          const int r = p / MS_TX, x = p - r * MS_TX;
          int s[MS_ROWSUMS];
#pragma unroll
          for (int k = 0; k < MS_ROWSUMS; k++) s[k] = 0;
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const int y = S.by[0][c][r][x + e];
            s[0] += y;
            s[1] += y * y;
#pragma unroll
            for (int k = 0; k < MS_KINDS; k++) {
              const int v = S.by[1 + k][c][r][x + e];
              s[2 + 3 * k] += v;
              s[3 + 3 * k] += v * v;
              s[4 + 3 * k] += v * y;
            }
          }
#pragma unroll
          for (int k = 0; k < MS_ROWSUMS; k++) S.rs[k][r][x] = s[k];
        }
        __syncthreads();
        for (int p = tid; p < MS_TY * MS_TX; p += MID_THREADS) {
          const int y = p / MS_TX, x = p - y * MS_TX;
          if (x0 + x < w && y0 + y < h) {                                 // an own pixel of the tile
            const int t0 = S.by[0][c][y][x];
#pragma unroll
            for (int k = 0; k < MS_KINDS; k++) {
              const int e = (int)S.by[1 + k][c][y][x] - t0;
              sse[k] += (unsigned long long)(e * e);
            }
          }
          if (x0 + x + 8 > w || y0 + y + 8 > h) continue;                 // the window would cross (h, w)
          int s[MS_ROWSUMS];
#pragma unroll
          for (int k = 0; k < MS_ROWSUMS; k++) {
            int v = 0;
#pragma unroll
            for (int e = 0; e < 8; e++) v += S.rs[k][y + e][x];
            s[k] = v;
          }
          // window sums of 64 bytes: S <= 16320, S.. <= 4161600, so 64 S.., S^2, S S and every term below are under 2^30 in
          // magnitude — 32-bit arithmetic gives the definition's 64-bit values, and the conversions to fp64 are exact
          const int Sy = s[0], vy = 64 * s[1] - Sy * Sy;
#pragma unroll
          for (int k = 0; k < MS_KINDS; k++) {
            const int Sx = s[2 + 3 * k], vx = 64 * s[3 + 3 * k] - Sx * Sx, cxy = 64 * s[4 + 3 * k] - Sx * Sy;
            const double t1 = (double)(2 * Sx * Sy) + MS_C1, t2 = (double)(2 * cxy) + MS_C2;
            const double u1 = (double)(Sx * Sx + Sy * Sy) + MS_C1, u2 = (double)(vx + vy) + MS_C2;
            ssim[k] += (t1 * t2) / (u1 * u2);
          }
        }
      }
      // the tile's sums of frame j: a tree per wave, the waves in order, onto the block's sums
#pragma unroll
      for (int k = 0; k < MS_KINDS; k++) {
        for (int o2 = 32; o2 > 0; o2 >>= 1) {
          ssim[k] += __shfl_down(ssim[k], o2, 64);
          sse[k] += __shfl_down(sse[k], o2, 64);
        }
        if (lane == 0) {
          S.wsum[wid][k] = ssim[k];
          if (sse[k]) atomicAdd(&S.bsse[(j - 1) * MS_KINDS + k], sse[k]);
        }
      }
      __syncthreads();
      if (tid < MS_KINDS)
        S.bsum[(j - 1) * MS_KINDS + tid] += ((S.wsum[0][tid] + S.wsum[1][tid]) + S.wsum[2][tid]) + S.wsum[3][tid];
    }
  }
}

// grid (blocks, B): block row b = pair slot
__global__ __launch_bounds__(MID_THREADS) void mid_score_kernel(const void* __restrict__ frames, const void* __restrict__ prev,
                                                                const int* __restrict__ tab, int B, int Hmax, int Wmax, int n,
                                                                const unsigned char* __restrict__ out_mid,
                                                                const void* __restrict__ truth, long long* __restrict__ out_sse,
                                                                double* __restrict__ out_ssim, double* __restrict__ part,
                                                                unsigned long long* __restrict__ acc_sse,
                                                                unsigned* __restrict__ ticket) {
  __shared__ MsShared S;
  const int b = blockIdx.y;
  const MidPair d = mid_pair(tab, B, b, Hmax, Wmax);
  if (d.h == 0 || tab[8 * (long)B + 8 * b + 6] == 0) return;              // not a pair, or not held out: uniform per block row
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long plane = (long)Hmax * Wmax;
  if (tid < MID_MAX * MS_KINDS) {
    S.bsum[tid] = 0.0;
    S.bsse[tid] = 0ull;
  }
  if (d.u8)
    ms_tiles(S, mid_frame<unsigned char>(frames, prev, plane, b, 0), mid_frame<unsigned char>(frames, prev, plane, b, 1),
             reinterpret_cast<const unsigned char*>(truth), out_mid, d.h, d.w, Wmax, n, b * plane, B * plane);
  else
    ms_tiles(S, mid_frame<float>(frames, prev, plane, b, 0), mid_frame<float>(frames, prev, plane, b, 1),
             reinterpret_cast<const float*>(truth), out_mid, d.h, d.w, Wmax, n, b * plane, B * plane);
  // the block's sums: the squared errors onto the slot's accumulators, the SSIM sums as partials; the ticket
  __syncthreads();
  const int nb = gridDim.x, words = n * MS_KINDS;
  double* pp = part + (long)b * MID_MAX * MS_KINDS * MS_CAP;
  unsigned long long* acc = acc_sse + (long)b * MID_MAX * MS_KINDS;
  if (tid < words) {
    pp[(long)tid * MS_CAP + blockIdx.x] = S.bsum[tid];
    if (S.bsse[tid]) atomicAdd(acc + tid, S.bsse[tid]);
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) S.last = atomicAdd(ticket + b, 1u) == (unsigned)(nb - 1);
  __syncthreads();
  if (!S.last) return;
  __threadfence();
  if (tid < words) {
    const int j = tid / MS_KINDS, k = tid - j * MS_KINDS;
    out_sse[((long)j * B + b) * MS_KINDS + k] = (long long)atomicExch(acc + tid, 0ull);
  }
  // a wave per sum: lane l takes the partials of blocks l, l + 64, ... in that order, then the tree.  The MS_CAP / 64 relaxed
  // device-scope loads of a lane are in flight together (one after the other they cost a round trip each: DESIGN 7.17)
  for (int q = wid; q < words; q += MS_WAVES) {
    double* p = pp + (long)q * MS_CAP;
    double v[MS_CAP / 64];
#pragma unroll
    for (int u = 0; u < MS_CAP / 64; u++) {
      const int i = lane + 64 * u;
      v[u] = i < nb ? __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < MS_CAP / 64; u++) s += v[u];
#pragma unroll
    for (int u = 0; u < MS_CAP / 64; u++) {
      const int i = lane + 64 * u;
      if (i < nb) p[i] = 0.0;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) {
      const int j = q / MS_KINDS, k = q - j * MS_KINDS;
      out_ssim[((long)j * B + b) * MS_KINDS + k] = s;
    }
  }
  if (tid == 0) ticket[b] = 0u;                        // ready for the next launch (graph replays included)
}

inline int ms_blocks(int Hmax, int Wmax) {
  const long tiles = (long)cdiv(Wmax, MS_TX) * cdiv(Hmax, MS_TY);
  return (int)(tiles < MS_CAP ? tiles : MS_CAP);
}

inline bool ms_shape_ok(int n, int B, int Hmax, int Wmax) { return mid_shape_ok(n, B, Hmax, Wmax) && B <= 65535; }

}  // namespace

UNFLOW_API size_t unflow_sequence_interpolate_score_workspace_bytes(int n, int B, int Hmax, int Wmax) {
  if (!ms_shape_ok(n, B, Hmax, Wmax)) return 0;
  // per slot: a partial per block of the largest grid for each of the 7 x 3 sums, the 7 x 3 squared-error accumulators, a ticket
  return (size_t)B * (MID_MAX * MS_KINDS * (MS_CAP + 1) * 8 + 8);
}

UNFLOW_API int unflow_sequence_interpolate_score(const void* frames, const int* tab, int B, int Hmax, int Wmax, int n,
                                                 const unsigned char* out_mid, const void* truth, void* prev, void* workspace,
                                                 long long* out_sse, double* out_ssim, unflow_stream_t stream) {
  if (!frames || !tab || !out_mid || !truth || !prev || !workspace || !out_sse || !out_ssim) return UNFLOW_ERR_NULL;
  if (!ms_shape_ok(n, B, Hmax, Wmax)) return UNFLOW_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return UNFLOW_ERR_UNSUPPORTED;
  double* part = reinterpret_cast<double*>(workspace);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(part + (size_t)B * MID_MAX * MS_KINDS * MS_CAP);
  unsigned* ticket = reinterpret_cast<unsigned*>(acc + (size_t)B * MID_MAX * MS_KINDS);
  const hipStream_t st = as_stream(stream);
  mid_score_kernel<<<dim3(ms_blocks(Hmax, Wmax), B), MID_THREADS, 0, st>>>(frames, prev, tab, B, Hmax, Wmax, n, out_mid, truth, out_sse,
                                                                           out_ssim, part, acc, ticket);
  mid_prev_kernel<<<stream_grid((long)Hmax * Wmax, MID_THREADS), MID_THREADS, 0, st>>>(frames, tab, B, Hmax, Wmax, prev);
  return launch_status();
}
