// PNG decode on the device (core/png_device.py): the two steps behind zlib's inflate that the host cannot vectorise.
//
// unflow_png_unfilter reconstructs the scanlines of a batch of images in one launch, one workgroup per image, geometry from a
// device table (include/unflow_hip.h).  A byte at (x, y) depends on (x - bpp, y), (x, y - 1) and (x - bpp, y - 1), mod 256, so the
// independent work of one image is its bpp byte lanes and a skewed wavefront over rows:
//
//   * R = 64 rows are in flight, one per LANE of the workgroup's first wave; a lane decodes a whole pixel (its bpp byte lanes,
//     unrolled) per step.  At step t lane r works on pixel t - r.  `a` (left) is the lane's own previous result; `b` (up) is lane
//     r - 1's result of the previous step, fetched with one DPP wave shift per byte lane (no LDS round trip on the chain); `c`
//     (upper left) is the lane's own previous `b`.  Lane 0 takes `b` from the row above the band.  The filter type is a per-lane
//     constant of the band and is applied with selects, so the wave never diverges and every lane is a valid DPP source.
//   * The band is walked in chunks of CW = 64 steps.  A chunk's raw bytes (row r: pixels [j CW - r, j CW - r + CW), the skewed
//     slab) sit in an LDS tile and are decoded in place.  Waves 1-3 are the memory side: while wave 0 decodes chunk j they store
//     chunk j - 1 and load chunk j + 1 (three tiles, one barrier per chunk), so the chain never waits on HBM inside a band.
//   * Bands of 64 rows run one after another.  The pipeline drains between bands; after the barrier the previous band's last
//     decoded row is read back from the output as the "up" row of the next band (row 64 of the tile).
//
// The kernel is bound by the dependency chain of wave 0 (w + 63 steps per band, about 35 instructions per byte lane and step,
// issued by one wave), not by bytes: 2B workgroups on a side stream under the training step (DESIGN 7.6 has the measured time).
// Scanline starts are odd (1 + w bpp bytes per row), so global accesses are byte-wide, 64 consecutive bytes per wave
// instruction; the memory side issues a row's loads branch-free and back to back, or it — not the chain — sets the pace (a
// guarded load per byte waits for each before the next: 3.2 instead of 2.2 ms for eight 384 x 1242 RGB frames).  Outputs are
// plain C++ stores.
//
// unflow_png_to_batch is read_png_image + crop + normalisation of core/input.py: decoded frames -> fp32 [n][H][W][3].
#include "common.h"

namespace {

constexpr int PNG_R = 64;                      // rows in flight = lanes of the decoding wave
constexpr int PNG_CW = 64;                     // steps per chunk
constexpr int PNG_PITCH = PNG_CW * 8 + 4;      // bytes per tile row: 129 dwords, odd, so the 64 lanes' bytes spread over the banks
constexpr int PNG_TILE = (PNG_R + 1) * PNG_PITCH;      // 64 skewed rows + the up row of lane 0
constexpr int PNG_TILES = 3;                   // decoding, being loaded, being stored
constexpr int PNG_DESC = 8;                    // int64 per image

struct PngImage {
  const unsigned char* src;                    // h rows of 1 + w bpp bytes
  unsigned char* dst;                          // h rows of w bpp bytes
  int h, w;
};

// b of lane r = v of lane r - 1 (DPP wave_shr:1; lane 0 gets 0).  Must run with all 64 lanes enabled.
__device__ __forceinline__ unsigned from_lane_above(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

// One tile row of chunk j: 64 * BPP consecutive bytes of a global row starting at byte g0 (may start before the row or run past
// its end: the address is clamped, and what lands in those tile bytes is never used).  Branch-free on purpose — every lane's
// BPP loads are issued before the first is waited for.
template <int BPP>
__device__ __forceinline__ void load_row(const unsigned char* from, long g0, long rowb, unsigned char* to, int lane) {
  unsigned char v[BPP];
#pragma unroll
  for (int k = 0; k < BPP; k++) v[k] = from[min(max(g0 + k * 64 + lane, 0L), rowb - 1)];
#pragma unroll
  for (int k = 0; k < BPP; k++) to[k * 64 + lane] = v[k];
}

// Rows first, first + nw, ... of chunk j of the band at y0: global -> tile; the wave with first == 0 also brings the decoded row
// y0 - 1 into row 64.  A row whose slab lies outside the image is skipped (uniform per wave).
template <int BPP>
__device__ __forceinline__ void load_chunk(const PngImage& im, int y0, int nrows, int j, unsigned char* tile, int first, int nw,
                                           int lane) {
  const long rowb = (long)im.w * BPP;
#pragma unroll 2
  for (int rr = first; rr < nrows; rr += nw) {
    const long g0 = (long)(j * PNG_CW - rr) * BPP;
    if (g0 + 64 * BPP <= 0 || g0 >= rowb) continue;
    load_row<BPP>(im.src + (long)(y0 + rr) * (rowb + 1) + 1, g0, rowb, tile + rr * PNG_PITCH, lane);
  }
  const long u0 = (long)j * PNG_CW * BPP;
  if (first == 0 && y0 > 0 && u0 < rowb) load_row<BPP>(im.dst + (long)(y0 - 1) * rowb, u0, rowb, tile + PNG_R * PNG_PITCH, lane);
}

template <int BPP>
__device__ __forceinline__ void store_chunk(const PngImage& im, int y0, int nrows, int j, const unsigned char* tile, int first,
                                            int nw, int lane) {
  const long rowb = (long)im.w * BPP;
#pragma unroll 2
  for (int rr = first; rr < nrows; rr += nw) {
    const long g0 = (long)(j * PNG_CW - rr) * BPP;
    if (g0 + 64 * BPP <= 0 || g0 >= rowb) continue;
    unsigned char* to = im.dst + (long)(y0 + rr) * rowb;
    const unsigned char* from = tile + rr * PNG_PITCH;
    unsigned char v[BPP];
#pragma unroll
    for (int k = 0; k < BPP; k++) v[k] = from[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < BPP; k++) {
      const long g = g0 + k * 64 + lane;
      if (g >= 0 && g < rowb) to[g] = v[k];
    }
  }
}

template <int BPP>
__device__ void unfilter_image(const PngImage& im, unsigned char* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int y0 = 0; y0 < im.h; y0 += PNG_R) {
    const int nrows = min(PNG_R, im.h - y0);
    const int nch = (im.w + nrows - 1 + PNG_CW - 1) / PNG_CW;
    load_chunk<BPP>(im, y0, nrows, 0, lds, wave, 4, lane);
    // per-lane state of the decoding wave: the row's filter, the left pixel, the previous step's up pixel and result
    unsigned ft = 0, a[BPP], c[BPP], res[BPP];
#pragma unroll
    for (int k = 0; k < BPP; k++) a[k] = c[k] = res[k] = 0;
    if (wave == 0 && lane < nrows) ft = im.src[(long)(y0 + lane) * ((long)im.w * BPP + 1)];
    const bool row_ok = lane < nrows, top = y0 == 0;
    __syncthreads();
    for (int j = 0; j < nch; j++) {
      unsigned char* tile = lds + (j % PNG_TILES) * PNG_TILE;
      if (wave == 0) {
        unsigned char* row = tile + lane * PNG_PITCH;
        const unsigned char* uprow = tile + PNG_R * PNG_PITCH;
        unsigned raw[BPP], nxt[BPP], up[BPP], upn[BPP];
#pragma unroll
        for (int k = 0; k < BPP; k++) raw[k] = row[k], up[k] = uprow[k];
        for (int s = 0; s < PNG_CW; s++) {
          const int x = j * PNG_CW + s - lane;
          const bool on = row_ok && (unsigned)x < (unsigned)im.w;
          const int sn = min(s + 1, PNG_CW - 1);              // the next step's raw pixel, in flight during this step
#pragma unroll
          for (int k = 0; k < BPP; k++) nxt[k] = row[sn * BPP + k], upn[k] = uprow[sn * BPP + k];      // uprow: one broadcast read
#pragma unroll
          for (int k = 0; k < BPP; k++) {
            unsigned b = from_lane_above(res[k]);
            if (lane == 0) b = top ? 0u : up[k];
            const int ia = (int)a[k], ib = (int)b, ic = (int)c[k];
            const int pa = abs(ib - ic), pb = abs(ia - ic), pc = abs(ia + ib - 2 * ic);
            const unsigned paeth = (pa <= pb && pa <= pc) ? a[k] : (pb <= pc ? b : c[k]);
            const unsigned avg = (a[k] + b) >> 1;             // on the 9-bit sum
            unsigned pred = 0;
            pred = ft == 1 ? a[k] : pred;
            pred = ft == 2 ? b : pred;
            pred = ft == 3 ? avg : pred;
            pred = ft == 4 ? paeth : pred;
            const unsigned v = (raw[k] + pred) & 255u;
            res[k] = on ? v : 0u;
            a[k] = res[k];
            c[k] = on ? b : 0u;
            if (on) row[s * BPP + k] = (unsigned char)v;
            raw[k] = nxt[k];
            up[k] = upn[k];
          }
        }
      } else {
        if (j > 0) store_chunk<BPP>(im, y0, nrows, j - 1, lds + ((j - 1) % PNG_TILES) * PNG_TILE, wave - 1, 3, lane);
        if (j + 1 < nch) load_chunk<BPP>(im, y0, nrows, j + 1, lds + ((j + 1) % PNG_TILES) * PNG_TILE, wave - 1, 3, lane);
      }
      __syncthreads();
    }
    store_chunk<BPP>(im, y0, nrows, nch - 1, lds + ((nch - 1) % PNG_TILES) * PNG_TILE, wave, 4, lane);
    __syncthreads();        // the band's rows are in memory (workgroup scope) before the next band reads its up row; tiles are free
  }
}

__global__ __launch_bounds__(256) void png_unfilter_kernel(const unsigned char* __restrict__ raw, long raw_bytes,
                                                           unsigned char* out, long out_bytes,
                                                           const long* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[PNG_TILES * PNG_TILE];
  const long* d = table + (long)blockIdx.x * PNG_DESC;
  const long src = d[0], dst = d[1], h = d[2], w = d[3], bpp = d[4];
  // a table entry that does not fit its buffers is skipped (the host validates; this is the memory-safety net)
  if (h <= 0 || w <= 0 || h > (1 << 24) || w > (1 << 24) || bpp < 1 || bpp > 8) return;
  if (src < 0 || dst < 0 || src + h * (1 + w * bpp) > raw_bytes || dst + h * w * bpp > out_bytes) return;
  PngImage im{raw + src, out + dst, (int)h, (int)w};
  switch ((int)bpp) {
    case 1: unfilter_image<1>(im, lds); break;
    case 2: unfilter_image<2>(im, lds); break;
    case 3: unfilter_image<3>(im, lds); break;
    case 4: unfilter_image<4>(im, lds); break;
    case 6: unfilter_image<6>(im, lds); break;
    case 8: unfilter_image<8>(im, lds); break;
    default: break;
  }
}

struct Norm {
  float mean[3], stddev;
  int on;
};

__global__ __launch_bounds__(256) void png_to_batch_kernel(const unsigned char* __restrict__ dec, long dec_bytes,
                                                           const long* __restrict__ table, int H, int W, Norm nm,
                                                           float* __restrict__ out) {
  const long* d = table + (long)blockIdx.y * PNG_DESC;
  const long off = d[1], h = d[2], w = d[3], bpp = d[4], sb = d[5], oy = d[6], ox = d[7];
  if (h <= 0 || w <= 0 || bpp < 1 || bpp > 8 || (sb != 1 && sb != 2) || bpp % sb != 0) return;
  if (oy < 0 || ox < 0 || oy + H > h || ox + W > w || off < 0 || off + h * w * bpp > dec_bytes) return;
  const int ch = (int)(bpp / sb);
  const unsigned n3 = (unsigned)H * (unsigned)W * 3u;            // < 2^31 (the host checks)
  float* o = out + (long)blockIdx.y * n3;
  const unsigned char* base = dec + off;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += gridDim.x * blockDim.x) {
    const unsigned pix = i / 3u, c = i - pix * 3u;
    const unsigned y = pix / (unsigned)W, x = pix - y * (unsigned)W;
    // grey (+ alpha) is replicated, alpha dropped, a 16-bit sample (big-endian) gives its high byte
    const unsigned sc = ch >= 3 ? c : 0u;
    float v = (float)base[((oy + y) * w + ox + x) * bpp + sc * sb];
    if (nm.on) v = __fdiv_rn(v - nm.mean[c], nm.stddev);
    o[i] = v;
  }
}

// The window entries share one geometry rule: output pixel (y, x) is frame pixel (y + oy, x + ox) when that lies inside (h, w),
// else 0 — oy, ox signed, so one rule is the random crop, the central crop and resize_image_with_crop_or_pad's zero padding.
constexpr long PNG_MAX_SIDE = 1 << 24;

struct PngWindow {
  const unsigned char* base;
  long h, w, oy, ox;
  int bpp, sb;
};

// False: the entry is skipped (it does not fit `dec`, or its fields are out of range).
__device__ __forceinline__ bool png_window_of(const long* d, const unsigned char* dec, long dec_bytes, PngWindow& g) {
  const long off = d[1], h = d[2], w = d[3], bpp = d[4], sb = d[5], oy = d[6], ox = d[7];
  if (h <= 0 || w <= 0 || h > PNG_MAX_SIDE || w > PNG_MAX_SIDE || bpp < 1 || bpp > 8 || (sb != 1 && sb != 2) || bpp % sb != 0 ||
      bpp / sb > 4)                        // 1 to 4 channels of 1 or 2 bytes: 1, 2, 3, 4, 6 or 8 bytes per pixel
    return false;
  if (oy < -PNG_MAX_SIDE || oy > PNG_MAX_SIDE || ox < -PNG_MAX_SIDE || ox > PNG_MAX_SIDE) return false;
  if (off < 0 || off > dec_bytes || h * w * bpp > dec_bytes - off) return false;
  g = PngWindow{dec + off, h, w, oy, ox, (int)bpp, (int)sb};
  return true;
}

__global__ __launch_bounds__(256) void png_to_window_kernel(const unsigned char* __restrict__ dec, long dec_bytes,
                                                            const long* __restrict__ table, int Hs, int Ws, Norm nm,
                                                            float* __restrict__ out) {
  PngWindow g;
  if (!png_window_of(table + (long)blockIdx.y * PNG_DESC, dec, dec_bytes, g)) return;
  const int ch = g.bpp / g.sb;
  const unsigned n3 = (unsigned)Hs * (unsigned)Ws * 3u;            // < 2^31 (the host checks)
  float* o = out + (long)blockIdx.y * n3;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += gridDim.x * blockDim.x) {
    const unsigned pix = i / 3u, c = i - pix * 3u;
    const unsigned y = pix / (unsigned)Ws, x = pix - y * (unsigned)Ws;
    const long fy = (long)y + g.oy, fx = (long)x + g.ox;
    const unsigned sc = ch >= 3 ? c : 0u;
    float v = 0.f;                                                  // the padding is zero BEFORE the normalisation
    if (fy >= 0 && fy < g.h && fx >= 0 && fx < g.w) v = (float)g.base[(fy * g.w + fx) * g.bpp + sc * g.sb];
    if (nm.on) v = __fdiv_rn(v - nm.mean[c], nm.stddev);
    o[i] = v;
  }
}

// KITTI's 16-bit RGB flow map: one thread per output pixel reads the pixel's six bytes once (byte loads: a packed frame's rows
// start at any address) and writes the flow pair with one 8-byte store.  (u16 - 32768) / 64 and float(u16) are exact in fp32.
__global__ __launch_bounds__(256) void png_to_flow_gt_kernel(const unsigned char* __restrict__ dec, long dec_bytes,
                                                             const long* __restrict__ table, int Hs, int Ws,
                                                             float2* __restrict__ flow, float* __restrict__ mask) {
  PngWindow g;
  if (!png_window_of(table + (long)blockIdx.y * PNG_DESC, dec, dec_bytes, g)) return;
  if (g.bpp != 6 || g.sb != 2) return;
  const unsigned n = (unsigned)Hs * (unsigned)Ws;                   // < 2^31 / 3 (the host checks)
  float2* of = flow + (long)blockIdx.y * n;
  float* om = mask + (long)blockIdx.y * n;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned y = i / (unsigned)Ws, x = i - y * (unsigned)Ws;
    const long fy = (long)y + g.oy, fx = (long)x + g.ox;
    float2 f = make_float2(0.f, 0.f);
    float m = 0.f;
    if (fy >= 0 && fy < g.h && fx >= 0 && fx < g.w) {
      const unsigned char* p = g.base + (fy * g.w + fx) * 6;
      unsigned char b[6];
#pragma unroll
      for (int k = 0; k < 6; k++) b[k] = p[k];
      f.x = ((float)(int)((b[0] << 8) | b[1]) - 32768.f) * 0.015625f;
      f.y = ((float)(int)((b[2] << 8) | b[3]) - 32768.f) * 0.015625f;
      m = (float)(int)((b[4] << 8) | b[5]);
    }
    of[i] = f;
    om[i] = m;
  }
}

}  // namespace

UNFLOW_API int unflow_png_unfilter_rows(void) { return PNG_R; }

UNFLOW_API int unflow_png_unfilter(const unsigned char* raw, long raw_bytes, unsigned char* decoded, long decoded_bytes,
                                   const long* table, int n, unflow_stream_t stream) {
  if (!raw || !decoded || !table) return UNFLOW_ERR_NULL;
  if (n <= 0 || n > 65535 || raw_bytes <= 0 || decoded_bytes <= 0) return UNFLOW_ERR_SHAPE;
  png_unfilter_kernel<<<n, 256, 0, as_stream(stream)>>>(raw, raw_bytes, decoded, decoded_bytes, table);
  return launch_status();
}

UNFLOW_API int unflow_png_to_batch(const unsigned char* decoded, long decoded_bytes, const long* table, int n, int H, int W,
                                   const float* mean3, float stddev, float* out, unflow_stream_t stream) {
  if (!decoded || !table || !out) return UNFLOW_ERR_NULL;
  if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || decoded_bytes <= 0 || (long)H * W * 3 > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
  if (mean3 && !(stddev != 0.f)) return UNFLOW_ERR_SHAPE;
  Norm nm{};
  if (mean3) {
    nm.mean[0] = mean3[0]; nm.mean[1] = mean3[1]; nm.mean[2] = mean3[2];
    nm.stddev = stddev;
    nm.on = 1;
  }
  const dim3 grid(min(stream_grid((long)H * W * 3), 256), n);
  png_to_batch_kernel<<<grid, 256, 0, as_stream(stream)>>>(decoded, decoded_bytes, table, H, W, nm, out);
  return launch_status();
}

UNFLOW_API int unflow_png_to_window(const unsigned char* decoded, long decoded_bytes, const long* table, int n, int Hs, int Ws,
                                    const float* mean3, float stddev, float* out, unflow_stream_t stream) {
  if (!decoded || !table || !out) return UNFLOW_ERR_NULL;
  if (n <= 0 || n > 65535 || Hs <= 0 || Ws <= 0 || decoded_bytes <= 0 || (long)Hs * Ws * 3 > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
  if (mean3 && !(stddev != 0.f)) return UNFLOW_ERR_SHAPE;
  Norm nm{};
  if (mean3) {
    nm.mean[0] = mean3[0]; nm.mean[1] = mean3[1]; nm.mean[2] = mean3[2];
    nm.stddev = stddev;
    nm.on = 1;
  }
  const dim3 grid(min(stream_grid((long)Hs * Ws * 3), 256), n);
  png_to_window_kernel<<<grid, 256, 0, as_stream(stream)>>>(decoded, decoded_bytes, table, Hs, Ws, nm, out);
  return launch_status();
}

UNFLOW_API int unflow_png_to_flow_gt(const unsigned char* decoded, long decoded_bytes, const long* table, int n, int Hs, int Ws,
                                     float* flow, float* mask, unflow_stream_t stream) {
  if (!decoded || !table || !flow || !mask) return UNFLOW_ERR_NULL;
  if (n <= 0 || n > 65535 || Hs <= 0 || Ws <= 0 || decoded_bytes <= 0 || (long)Hs * Ws * 3 > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
  const dim3 grid(min(stream_grid((long)Hs * Ws), 256), n);
  png_to_flow_gt_kernel<<<grid, 256, 0, as_stream(stream)>>>(decoded, decoded_bytes, table, Hs, Ws,
                                                             reinterpret_cast<float2*>(flow), mask);
  return launch_status();
}

// A stream of the loader's own (core/png_device.py::loader_stream).  torch.cuda.Stream() hands out the streams of a pool of 32
// round-robin, so a loader's "side" stream can BE the stream on which another thread captures a hipGraph (torch.cuda.graph's
// default capture stream, the engine's): the producer thread's uploads then land inside the capture.  A stream created here is
// in no pool.  Non-blocking: no implicit ordering with the null stream.  Never destroyed by the caller (pinned buffers that were
// read on it may be freed, and recorded on it, later).
UNFLOW_API int unflow_stream_create(unflow_stream_t* stream) {
  if (!stream) return UNFLOW_ERR_NULL;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return UNFLOW_ERR_LAUNCH;
  *stream = reinterpret_cast<unflow_stream_t>(s);
  return UNFLOW_OK;
}
