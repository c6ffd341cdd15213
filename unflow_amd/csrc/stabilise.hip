// Camera motion along a clip (core/inference.py FlowEstimator(..., sequence=..., stabilise=...)): per pair of a sequence
// replay a robust affine fit to the forward flow (the dominant motion), the pixels that do not follow it (the residual map), the
// camera path composed along the clip and the pair's later frame resampled along that path (the stabilised frame).
//
// The definition is include/unflow_hip.h's and it is integer everywhere but in the 3 x 3 solve: the flow is quantised to 1/64 px,
// the coordinates are half pixels about the frame centre, the weights are powers of two from the integer L1 residual, and the
// thirteen sums of the normal equations are 64-bit integers.  Integer addition is associative, so the order in which blocks and
// atomics arrive cannot change a bit; the solve is a fixed sequence of fp64 operations, each rounded on its own
// (-ffp-contract=off), on integers that are the same whatever the order.  tests/stabilise_ref.py mirrors every step and the test
// is equality.  2 R + 3 launches (R = iters), the kernel boundaries being the only hand-off between workgroups:
//   st_accumulate_kernel   R + 1 times, grid (blocks, B): a thread walks pixels of its pair slot with a stride and keeps the thirteen
//                          sums in registers; a shuffle tree per wave, the four waves through LDS, then one 64-bit integer atomic
//                          per sum and block into the slot's words of the workspace.  Iteration r >= 1 weights a pixel by its
//                          residual under the model the solve kernel left in the workspace.
//   st_solve_kernel        R + 1 times, one wave: lane b takes the sums of slot b (and zeroes them), solves and keeps the model
//                          in the workspace; a degenerate iteration ends the slot's loop (the later accumulate passes return at
//                          once).  The last one also walks the slots in order for the path, writes out_motion, out_path and the
//                          path state, zeroes out_counts and leaves the workspace zero: no memset node in a captured graph.
//   st_apply_kernel        grid (blocks, B), one thread per pixel: the residual map under the final model, the stabilised pixel
//                          (four taps of the later frame, 8.8 colours, 8-bit fractions) and the four counts — ballots per wave,
//                          LDS per block, one integer atomic per count and block.
// No float atomics, no float reductions, no inline assembly.  tol, iters and follow travel by value.
#include "common.h"
#include "mid_common.h"

namespace {

constexpr int ST_THREADS = 256, ST_WAVES = ST_THREADS / 64;
constexpr int ST_SUMS = 13;                            // g, gX, gY, gXX, gXY, gYY, gU, gXU, gYU, gV, gXV, gYV, #{g > 0}
// a slot's words of the workspace: the sums, then the model P[6], ended (a degenerate iteration), successful iterations, n of the last
constexpr int ST_P = 13, ST_ENDED = 19, ST_OK = 20, ST_N = 21, ST_WORDS = 24;
constexpr int ST_MAX = 4096;                           // Hmax, Wmax: |X|, |Y| < 2^13 (the ranges: include/unflow_hip.h)
constexpr int ST_ACC_PIXELS = 8;                       // pixels per thread the accumulate grid is sized for
constexpr long long ST_ONE = 1LL << 24;                // 1 in the linear part of a path

// mid_common.h's rule of what a pair slot is (slot 0 without a carried frame is none): one definition for the whole clip
__device__ __forceinline__ bool st_pair(const int* __restrict__ tab, int B, int b, int Hmax, int Wmax, int& h, int& w) {
  const MidPair d = mid_pair(tab, B, b, Hmax, Wmax);
  h = d.h;
  w = d.w;
  return d.h > 0;
}

// One pixel's flow in 1/64 px; false: not VALID (a component not finite or of magnitude >= 4096; tested before any conversion)
__device__ __forceinline__ bool st_quantise(float2 f, int& U, int& V) {
  if (!(fabsf(f.x) < 4096.f && fabsf(f.y) < 4096.f)) return false;
  U = (int)rintf(f.x * 64.f);
  V = (int)rintf(f.y * 64.f);
  return true;
}

// the L1 residual of (U, V) at (X, Y) under model P, in 2^-16 px
__device__ __forceinline__ long long st_residual(const long long (&P)[6], int X, int Y, int U, int V) {
  const long long pu = P[0] + ((P[1] * X + P[2] * Y + 256) >> 9);
  const long long pv = P[3] + ((P[4] * X + P[5] * Y + 256) >> 9);
  const long long ru = ((long long)U << 10) - pu, rv = ((long long)V << 10) - pv;
  return (ru < 0 ? -ru : ru) + (rv < 0 ? -rv : rv);
}

// grid (blocks, B); shift = 17 - k_r of iteration r >= 1 (r == 0: every eligible pixel weighs 1)
__global__ __launch_bounds__(ST_THREADS) void st_accumulate_kernel(const float2* __restrict__ flow, const unsigned char* __restrict__ occ,
                                                                   const int* __restrict__ tab, int B, int Hmax, int Wmax, int r,
                                                                   int shift, long long* ws) {
  __shared__ long long red[ST_WAVES][ST_SUMS];
  const int b = blockIdx.y;
  int h, w;
  if (!st_pair(tab, B, b, Hmax, Wmax, h, w)) return;   // uniform per block row: nothing read, nothing written
  const int npx = h * w;                               // <= 2^24
  if ((int)(blockIdx.x * ST_THREADS) >= npx) return;
  long long* st = ws + (long)b * ST_WORDS;
  if (st[ST_ENDED]) return;                            // a degenerate iteration ended this slot's loop
  long long P[6];
#pragma unroll
  for (int j = 0; j < 6; j++) P[j] = r ? st[ST_P + j] : 0;
  const long plane = (long)Hmax * Wmax;
  const float2* f = flow + b * plane;
  const unsigned char* o = occ ? occ + b * plane : nullptr;
  long long S[ST_SUMS];
#pragma unroll
  for (int j = 0; j < ST_SUMS; j++) S[j] = 0;
  for (int p = blockIdx.x * ST_THREADS + threadIdx.x; p < npx; p += gridDim.x * ST_THREADS) {
    const int y = p / w, x = p - y * w;
    const long q = (long)y * Wmax + x;
    int U, V;
    if (!st_quantise(f[q], U, V)) continue;
    if (o && o[q]) continue;                           // not ELIGIBLE
    const int X = 2 * x - (w - 1), Y = 2 * y - (h - 1);
    int g = 1;
    if (r) {
      const long long d = st_residual(P, X, Y, U, V) >> shift;
      if (d >= 6) continue;                            // weight zero from six halvings on
      g = 64 >> (int)d;
    }
    const int gX = g * X, gY = g * Y;                  // < 2^19
    const long long gU = (long long)g * U, gV = (long long)g * V;   // < 2^24
    S[0] += g;
    S[1] += gX;
    S[2] += gY;
    S[3] += (long long)gX * X;
    S[4] += (long long)gX * Y;
    S[5] += (long long)gY * Y;
    S[6] += gU;
    S[7] += gU * X;
    S[8] += gU * Y;
    S[9] += gV;
    S[10] += gV * X;
    S[11] += gV * Y;
    S[12] += 1;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < ST_SUMS; j++) {
    long long v = S[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wid][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < ST_SUMS) {
    const long long v = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(st + threadIdx.x), (unsigned long long)v);   // two's complement: exact
  }
}

__device__ __forceinline__ long long st_round_clamp(double v, double lim) {
  double x = rint(v);
  if (!(x < lim)) x = lim;                             // a NaN goes to the upper limit (none is reachable behind positive pivots)
  if (x < -lim) x = -lim;
  return (long long)x;
}

// The solve of include/unflow_hip.h on the sums S: false = degenerate, P untouched
__device__ __forceinline__ bool st_solve(const long long (&S)[ST_SUMS], long long (&P)[6]) {
  if (S[12] < 16) return false;
  const double A00 = (double)S[0], A01 = (double)S[1], A02 = (double)S[2], A11 = (double)S[3], A12 = (double)S[4], A22 = (double)S[5];
  const double a00 = A00;
  if (!(a00 > 0.0)) return false;
  const double m1 = A01 / a00, m2 = A02 / a00;
  const double a11 = A11 - m1 * A01, a12 = A12 - m1 * A02;
  double a22 = A22 - m2 * A02;
  if (!(a11 > 0.0)) return false;
  const double m3 = a12 / a11;
  a22 = a22 - m3 * a12;
  if (!(a22 > 0.0)) return false;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const double b0 = (double)S[6 + 3 * c], b1 = (double)S[7 + 3 * c], b2 = (double)S[8 + 3 * c];
    const double b1p = b1 - m1 * b0;
    const double b2p = (b2 - m2 * b0) - m3 * b1p;
    const double p2 = b2p / a22;
    const double p1 = (b1p - a12 * p2) / a11;
    const double p0 = ((b0 - A01 * p1) - A02 * p2) / a00;
    P[3 * c] = st_round_clamp(p0 * 1024.0, 268435456.0);           // 2^-6 px -> 2^-16 px, +-2^28
    P[3 * c + 1] = st_round_clamp(p1 * 524288.0, 8388608.0);        // 2^-5 per pixel -> 2^-24, +-2^23
    P[3 * c + 2] = st_round_clamp(p2 * 524288.0, 8388608.0);
  }
  return true;
}

__device__ __forceinline__ long long st_clamp(long long v, long long lim) { return v < -lim ? -lim : (v > lim ? lim : v); }

// one wave; last: iteration R, which also walks the path and cleans up
__global__ __launch_bounds__(64) void st_solve_kernel(const int* __restrict__ tab, int B, int Hmax, int Wmax, int last, int follow,
                                                      long long* ws, long long* path, long long* __restrict__ out_motion,
                                                      long long* __restrict__ out_path, int* __restrict__ out_counts) {
  for (int b = threadIdx.x; b < B; b += 64) {
    int h, w;
    if (!st_pair(tab, B, b, Hmax, Wmax, h, w)) continue;
    long long* st = ws + (long)b * ST_WORDS;
    if (st[ST_ENDED]) continue;                        // its sums were not formed and are zero
    long long S[ST_SUMS], P[6];
#pragma unroll
    for (int j = 0; j < ST_SUMS; j++) {
      S[j] = st[j];
      st[j] = 0;
    }
    if (st_solve(S, P)) {
#pragma unroll
      for (int j = 0; j < 6; j++) st[ST_P + j] = P[j];
      st[ST_OK] += 1;
      st[ST_N] = S[12];
    } else {
      st[ST_ENDED] = 1;
    }
  }
  if (!last) return;
  __syncthreads();                                     // one workgroup: its own global writes are visible behind the barrier
  if (threadIdx.x != 0) return;
  long long D[6] = {0, ST_ONE, 0, 0, 0, ST_ONE};
  if (tab[16 * (long)B] > 0) {                         // a later replay of the clip: continue from the state
#pragma unroll
    for (int j = 0; j < 6; j++) D[j] = path[j];
  }
  bool any = false;
  for (int b = 0; b < B; b++) {
    int h, w;
    if (!st_pair(tab, B, b, Hmax, Wmax, h, w)) continue;
    long long* st = ws + (long)b * ST_WORDS;
    long long P[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
      P[j] = st[ST_P + j];
      out_motion[8 * (long)b + j] = P[j];
    }
    const long long ok = st[ST_OK];
    out_motion[8 * (long)b + 6] = (ok ? 0 : 1) | (ok << 8);
    out_motion[8 * (long)b + 7] = st[ST_N];
#pragma unroll
    for (int j = ST_P; j < ST_WORDS; j++) st[j] = 0;
    // D' = M o D
    const long long Mxx = ST_ONE + P[1], Mxy = P[2], Myx = P[4], Myy = ST_ONE + P[5], half = 1LL << 23;
    long long N[6];
    N[0] = P[0] + ((Mxx * D[0] + Mxy * D[3] + half) >> 24);
    N[3] = P[3] + ((Myx * D[0] + Myy * D[3] + half) >> 24);
    N[1] = (Mxx * D[1] + Mxy * D[4] + half) >> 24;
    N[2] = (Mxx * D[2] + Mxy * D[5] + half) >> 24;
    N[4] = (Myx * D[1] + Myy * D[4] + half) >> 24;
    N[5] = (Myx * D[2] + Myy * D[5] + half) >> 24;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const long long id = (j == 1 || j == 5) ? ST_ONE : 0;
      long long v = N[j];
      if (follow) {
        const long long E = v - id;
        v = id + E - (E >> follow);
      }
      D[j] = st_clamp(v, (j == 0 || j == 3) ? (1LL << 30) : (1LL << 26));
      out_path[8 * (long)b + j] = D[j];
    }
    out_path[8 * (long)b + 6] = 0;
    out_path[8 * (long)b + 7] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) out_counts[4 * (long)b + j] = 0;   // counted by the apply pass
    any = true;
  }
  if (any) {
#pragma unroll
    for (int j = 0; j < 6; j++) path[j] = D[j];
    path[6] = 0;
    path[7] = 0;
  }
}

template <typename T>
__device__ __forceinline__ void st_sample(const T* __restrict__ im, int Wmax, int ix, int iy, int jx, int jy, int qx, int qy,
                                          unsigned char* __restrict__ o) {
  const long a = ((long)iy * Wmax + ix) * 3, b = ((long)iy * Wmax + jx) * 3, c = ((long)jy * Wmax + ix) * 3,
             d = ((long)jy * Wmax + jx) * 3;
  const long long waa = (256 - qx) * (256 - qy), wba = qx * (256 - qy), wab = (256 - qx) * qy, wbb = qx * qy;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const long long s = waa * mid_q((float)im[a + k]) + wba * mid_q((float)im[b + k]) + wab * mid_q((float)im[c + k]) +
                        wbb * mid_q((float)im[d + k]);
    o[k] = (unsigned char)((s + (1LL << 23)) >> 24);
  }
}

// grid (blocks, B); shift = 17 - k
__global__ __launch_bounds__(ST_THREADS) void st_apply_kernel(const void* __restrict__ frames, const float2* __restrict__ flow,
                                                              const unsigned char* __restrict__ occ, const int* __restrict__ tab, int B,
                                                              int Hmax, int Wmax, int shift, const long long* __restrict__ out_motion,
                                                              const long long* __restrict__ out_path,
                                                              unsigned char* __restrict__ out_resid, unsigned char* __restrict__ out_stab,
                                                              int* __restrict__ out_counts) {
  __shared__ int cnt[4];
  const int b = blockIdx.y;
  int h, w;
  if (!st_pair(tab, B, b, Hmax, Wmax, h, w)) return;
  const int npx = h * w;
  if ((int)(blockIdx.x * ST_THREADS) >= npx) return;
  const bool u8 = tab[8 * (long)B + 8 * b + 5] != 0;
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  long long P[6], D[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    P[j] = out_motion[8 * (long)b + j];
    D[j] = out_path[8 * (long)b + j];
  }
  const long plane = (long)Hmax * Wmax;
  const float2* f = flow + b * plane;
  const unsigned char* o = occ ? occ + b * plane : nullptr;
  const long long xmax = (long long)(w - 1) << 17, ymax = (long long)(h - 1) << 17;
  // uniform trip count per wave: the ballots below need every lane; the counts stay in (wave-uniform) registers over the passes
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int p0 = blockIdx.x * ST_THREADS; p0 < npx; p0 += gridDim.x * ST_THREADS) {
    const int p = p0 + threadIdx.x;
    const bool in = p < npx;
    bool valid = false, masked = false, moving = false, bare = false;
    if (in) {
      const int y = p / w, x = p - y * w;
      const long q = (long)y * Wmax + x;
      const int X = 2 * x - (w - 1), Y = 2 * y - (h - 1);
      int U, V;
      valid = st_quantise(f[q], U, V);
      unsigned char res = 255;
      if (valid) {
        const long long e = st_residual(P, X, Y, U, V);
        const long long rq = e >> 14;
        res = (unsigned char)(rq > 255 ? 255 : rq);
        masked = o && o[q];
        moving = !masked && (e >> shift) >= 6;
      }
      out_resid[b * plane + q] = res;
      const long long Px = 2 * (D[0] + ((D[1] * X + D[2] * Y + 256) >> 9)) + ((long long)(w - 1) << 16);
      const long long Py = 2 * (D[3] + ((D[4] * X + D[5] * Y + 256) >> 9)) + ((long long)(h - 1) << 16);
      unsigned char* so = out_stab + (b * plane + q) * 3;
      if (Px >= 0 && Px <= xmax && Py >= 0 && Py <= ymax) {
        const int ix = (int)(Px >> 17), iy = (int)(Py >> 17), qx = (int)(Px >> 9) & 255, qy = (int)(Py >> 9) & 255;
        const int jx = min(ix + 1, w - 1), jy = min(iy + 1, h - 1);
        if (u8)
          st_sample(reinterpret_cast<const unsigned char*>(frames) + b * plane * 3, Wmax, ix, iy, jx, jy, qx, qy, so);
        else
          st_sample(reinterpret_cast<const float*>(frames) + b * plane * 3, Wmax, ix, iy, jx, jy, qx, qy, so);
      } else {
        so[0] = 0; so[1] = 0; so[2] = 0;
        bare = true;
      }
    }
    c0 += (int)__popcll(__ballot(valid));
    c1 += (int)__popcll(__ballot(masked));
    c2 += (int)__popcll(__ballot(moving));
    c3 += (int)__popcll(__ballot(bare));
  }
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(cnt + 0, c0);
    if (c1) atomicAdd(cnt + 1, c1);
    if (c2) atomicAdd(cnt + 2, c2);
    if (c3) atomicAdd(cnt + 3, c3);
  }
  __syncthreads();
  if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(out_counts + 4 * (long)b + threadIdx.x, cnt[threadIdx.x]);   // integer: exact
}

inline bool st_shape_ok(int B, int Hmax, int Wmax) {
  return B >= 1 && B <= 65535 && Hmax >= 1 && Wmax >= 1 && Hmax <= ST_MAX && Wmax <= ST_MAX;
}

}  // namespace

UNFLOW_API size_t unflow_sequence_stabilise_workspace_bytes(int B) {
  if (B < 1 || B > 65535) return 0;
  return (size_t)B * ST_WORDS * sizeof(long long);
}

UNFLOW_API int unflow_sequence_stabilise(const void* frames, const int* tab, int B, int Hmax, int Wmax, const float* flow_fw,
                                         const unsigned char* occ_fw, int tol, int iters, int follow, long long* path,
                                         void* workspace, long long* out_motion, long long* out_path, unsigned char* out_resid,
                                         unsigned char* out_stab, int* out_counts, unflow_stream_t stream) {
  if (!frames || !tab || !flow_fw || !path || !workspace || !out_motion || !out_path || !out_resid || !out_stab || !out_counts)
    return UNFLOW_ERR_NULL;
  if (!st_shape_ok(B, Hmax, Wmax)) return UNFLOW_ERR_SHAPE;
  if (tol < 0 || tol > 4 || iters < 0 || iters > 4 || follow < 0 || follow > 8) return UNFLOW_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(path) | reinterpret_cast<uintptr_t>(out_motion) |
       reinterpret_cast<uintptr_t>(out_path) | reinterpret_cast<uintptr_t>(flow_fw)) & 7)   // flow_fw is read as float2
    return UNFLOW_ERR_UNSUPPORTED;
  const hipStream_t st = as_stream(stream);
  long long* ws = reinterpret_cast<long long*>(workspace);
  const float2* flow = reinterpret_cast<const float2*>(flow_fw);
  const long pixels = (long)Hmax * Wmax;
  int acc_blocks = cdiv(pixels, (long)ST_THREADS * ST_ACC_PIXELS);
  if (acc_blocks > 512) acc_blocks = 512;
  // the apply grid: what the chip keeps resident over all slots — every block ends with four atomics on its slot's one line of
  // counts, and with a block per 256 pixels those, not the pixels, set the kernel's time
  int app_blocks = stream_grid(pixels, ST_THREADS);
  if (app_blocks > cdiv(2048, B)) app_blocks = cdiv(2048, B);
  const dim3 acc(acc_blocks, B), app(app_blocks, B);
  for (int r = 0; r <= iters; r++) {
    const int kr = tol - (iters - r) > 0 ? tol - (iters - r) : 0;
    st_accumulate_kernel<<<acc, ST_THREADS, 0, st>>>(flow, occ_fw, tab, B, Hmax, Wmax, r, 17 - kr, ws);
    st_solve_kernel<<<1, 64, 0, st>>>(tab, B, Hmax, Wmax, r == iters, follow, ws, path, out_motion, out_path, out_counts);
  }
  st_apply_kernel<<<app, ST_THREADS, 0, st>>>(frames, flow, occ_fw, tab, B, Hmax, Wmax, 17 - tol, out_motion, out_path, out_resid,
                                              out_stab, out_counts);
  return launch_status();
}
