// Deflate on the device (core/png_device.py): the entropy coder of the PNG writer, the last stage of an export that was bound to
// host CPUs.  unflow_deflate turns byte streams that already sit in a device buffer (the scanlines unflow_png_filter wrote) into
// finished zlib streams; the host copies compressed bytes back, forms the chunk CRCs and writes.  The format is the exact integer
// rule of include/unflow_hip.h (tests/deflate_ref.py is the same rule in Python, and the output equals it byte for byte): chunks
// of chunk_bytes coded independently as stored / Huffman over literals / Huffman over literals and distance-1 runs, whichever
// is smallest — the data-parallel part of deflate.  No general LZ77 matching.
//
// deflate_chunk_kernel, one workgroup of 512 threads per (stream, chunk); a thread owns a contiguous span of the chunk:
//   * the chunk is staged into LDS at the source's own 16-byte phase (scanline streams start at every alignment), with 16-byte
//     loads between the first and the last boundary and byte loads at the ragged ends;
//   * a pass over the span: the literal histogram (LDS atomic adds, one per run of equal bytes), the Adler-32 partials, and the
//     span's last / first byte that differs from its predecessor; two block scans (wave shuffles, one LDS step across the waves)
//     turn those into "where did the run I start in begin" and "where does the run I end in stop", so a thread knows the whole
//     run — and its pieces of at most 258 — around every byte of its span without looking outside it;
//   * the token walk fills the second histogram; 2 x 256 threads rank-sort the two histograms by (count, symbol); ONE thread
//     per coding then builds the code (in-place minimum-redundancy construction, the length limit's repair rule, canonical
//     codes, the code-length header) — small and serial, 286 symbols — and leaves the header's bits and the body's size in LDS;
//   * the three sizes are compared; for a Huffman coding the bit lengths of the spans are prefix-summed and every thread
//     writes its tokens at its bit offset into a zeroed LDS buffer: whole words of its own with plain stores, the first and the
//     last word, which it shares with its neighbours, with LDS atomic OR;
//   * the segment goes to the chunk's slot of a scratch buffer with 16-byte stores (the slot is 16-byte aligned), its size, the
//     Adler partials and the coding to the chunk's meta entry.
// deflate_pack_kernel, one workgroup per (stream, chunk) again: the segment's offset is the sum of the sizes before it; the
// segment moves from its slot to its place in the zlib stream — 16-byte stores between the destination's boundaries, each
// formed from aligned words of the slot by funnel shifts, byte stores at the ragged ends; the first chunk's workgroup writes
// 78 01, the last one's combines the Adler partials, writes the checksum and the stream's size.
//
// Plain C++ and LDS atomics only (integer OR and ADD: order-independent, so the output is bit-reproducible), no float arithmetic.
#include "common.h"

namespace {

constexpr int DF_THREADS = 512;
constexpr int DF_WAVES = DF_THREADS / 64;
constexpr int DF_FIELDS = UNFLOW_DEFLATE_FIELDS;
constexpr int DF_META = UNFLOW_DEFLATE_META;
constexpr int DF_SYMS = 286;
constexpr int DF_EOB = 256;
constexpr int DF_MAX_MATCH = 258;
constexpr int DF_HDR_WORDS = 72;                    // 17 + 57 + 287 * 7 bits at the most (see the header), rounded up
constexpr int DF_PACK_THREADS = 256;
constexpr unsigned ADLER_MOD = 65521u;

__host__ __device__ inline long df_round16(long v) { return (v + 15) & ~15L; }
__host__ __device__ inline long df_slot(int chunk_bytes) { return df_round16(chunk_bytes + 5) + 16; }

struct Entry {
  long src, bytes, dst, cap, chunks;
  long scratch, meta;
  bool ok;
};

// The memory-safety net both kernels share (the host validates the same conditions and refuses before any launch).
__host__ __device__ inline Entry df_entry(const long* d, int chunk_bytes, long in_bytes, long scratch_bytes, long meta_chunks,
                                         long out_bytes) {
  Entry e;
  e.src = d[0], e.bytes = d[1], e.dst = d[2];
  const long cap = e.cap = d[3];
  e.scratch = d[4], e.meta = d[5];
  e.chunks = 0;
  e.ok = false;
  if (e.bytes < 1 || e.bytes > in_bytes || e.src < 0 || e.src > in_bytes - e.bytes) return e;
  e.chunks = (e.bytes + chunk_bytes - 1) / chunk_bytes;
  const long need = 2 + e.bytes + 5 * e.chunks + 4;
  if (e.dst < 0 || cap < need || cap > out_bytes || e.dst > out_bytes - cap) return e;
  const long slots = e.chunks * df_slot(chunk_bytes);
  if (e.scratch < 0 || (e.scratch & 15) != 0 || slots > scratch_bytes || e.scratch > scratch_bytes - slots) return e;
  if (e.meta < 0 || e.chunks > meta_chunks || e.meta > meta_chunks - e.chunks) return e;
  e.ok = true;
  return e;
}

// One code under construction (LDS).
struct Tree {
  int count[288];             // the histogram
  int key[288];               // counts of the used symbols in sorted order; then the construction's work array
  unsigned short sym[288];    // the used symbols sorted by (count, symbol)
  unsigned short code[288];   // bit-reversed canonical code: sent from bit 0
  unsigned char len[288];
  unsigned hdr[DF_HDR_WORDS]; // the block header's bits behind BFINAL .. (BFINAL itself is OR-ed in by the composer)
  int level[16], next[16];
  int cl_count[20], cl_key[20], cl_sym[20], cl_len[20], cl_code[20];
  int used, hdr_bits, body_bits;
};

__device__ __forceinline__ int length_symbol(int len) {      // RFC 1951 3.2.5, by formula (the reference uses the table)
  if (len <= 10) return 254 + len;
  if (len == DF_MAX_MATCH) return 285;
  const int l = len - 3, eb = (31 - __clz(l)) - 2;
  return 261 + 4 * eb + ((l >> eb) & 3);
}
__device__ __forceinline__ int length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// Inclusive block scan of one int per thread; `tot` holds DF_WAVES ints.  Both barriers are inside: call from uniform code.
template <class Op>
__device__ __forceinline__ int block_scan(int v, int ident, Op op, int* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v = op(u, v);
  }
  if (lane == 63) tot[wave] = v;
  __syncthreads();
  int pre = ident;
  for (int w = 0; w < wave; w++) pre = op(pre, tot[w]);
  __syncthreads();
  return op(pre, v);
}

// The tokens of positions [lo, hi) of a chunk of n bytes in coding 2.  before: the last position below lo whose byte differs from
// its predecessor (position 0 counts as one); after: the first such position at or behind hi, n if there is none.  A run is the
// maximal stretch [s, q) of bytes that equal their predecessor; L = q - s >= 3: matches of 258 from s, then for r = L % 258 one
// match of r if r >= 3, else r literals.
template <class F>
__device__ __forceinline__ void walk_tokens(const unsigned char* in, int lo, int hi, int before, int after, F&& f) {
  int p = before, q = -1;
  for (int i = lo; i < hi; i++) {
    const unsigned b = in[i];
    if (i == 0 || b != in[i - 1]) {
      f(0, (int)b);
      p = i, q = -1;
      continue;
    }
    if (q < 0) {
      q = i + 1;
      while (q < hi && in[q] == in[q - 1]) q++;
      if (q == hi) q = after;
    }
    const int s = p + 1, L = q - s, o = i - s;
    if (L < 3) {
      f(0, (int)b);
      continue;
    }
    const int r = L % DF_MAX_MATCH, full = L - r;
    if (o >= full) {
      if (r < 3)
        f(0, (int)b);
      else if (o == full)
        f(1, r);
    } else if (o % DF_MAX_MATCH == 0) {
      f(1, DF_MAX_MATCH);
    }
  }
}

// m >= 2 sorted counts in a[] -> leaves per code length in level[1 .. limit] (ONE thread).  Moffat and Katajainen's in-place
// construction (a[] holds weights, then parent indices, then depths of the internal nodes; a leaf is taken before an internal
// node of equal weight); depths above the limit count at the limit; the repair rule: while the Kraft sum exceeds 1, one leaf
// leaves the limit and the deepest non-empty level below it hands one leaf to the next level as two.
__device__ void huff_levels(int* a, int m, int limit, int* level) {
  for (int d = 0; d < 16; d++) level[d] = 0;
  a[0] += a[1];
  int root = 0, leaf = 2;
  for (int nxt = 1; nxt < m - 1; nxt++) {
    if (leaf >= m || a[root] < a[leaf]) {
      a[nxt] = a[root];
      a[root++] = nxt;
    } else {
      a[nxt] = a[leaf++];
    }
    if (leaf >= m || (root < nxt && a[root] < a[leaf])) {
      a[nxt] += a[root];
      a[root++] = nxt;
    } else {
      a[nxt] += a[leaf++];
    }
  }
  a[m - 2] = 0;
  for (int nxt = m - 3; nxt >= 0; nxt--) a[nxt] = a[a[nxt]] + 1;
  int avail = 1, depth = 0;
  root = m - 2;
  while (avail > 0) {
    int used = 0;
    while (root >= 0 && a[root] == depth) used++, root--;
    if (avail > used) level[depth < limit ? depth : limit] += avail - used;
    avail = 2 * used;
    depth++;
  }
  int total = 0;
  for (int d = 1; d <= limit; d++) total += level[d] << (limit - d);
  while (total > (1 << limit)) {
    level[limit]--;
    for (int d = limit - 1; d >= 1; d--)
      if (level[d]) {
        level[d]--;
        level[d + 1] += 2;
        break;
      }
    total--;
  }
}

struct SerialBits {            // an LSB-first writer of one thread into words of its own
  unsigned* w;
  unsigned long long acc;
  int n, word;
  __device__ void put(unsigned v, int nb) {
    acc |= (unsigned long long)v << n;
    n += nb;
    if (n >= 32) {
      if (word < DF_HDR_WORDS - 1) w[word++] = (unsigned)acc;      // never reached: the header's bound is below it
      acc >>= 32;
      n -= 32;
    }
  }
};

// The code-length sequence of a block: lens[0 .. nlit) and the one distance code's length 1, zeros in runs (17 / 18), every
// other length as it is.  f(symbol, extra bits, extra value).
template <class F>
__device__ __forceinline__ void walk_lengths(const unsigned char* lens, int nlit, F&& f) {
  int i = 0;
  while (i <= nlit) {
    const int v = i < nlit ? lens[i] : 1;
    if (v) {
      f(v, 0, 0);
      i++;
      continue;
    }
    int z = 0;
    while (i + z < nlit && lens[i + z] == 0) z++;
    i += z;
    while (z >= 3) {
      const int t = z < 138 ? z : 138;
      if (t >= 11)
        f(18, 7, t - 11);
      else
        f(17, 3, t - 3);
      z -= t;
    }
    for (; z > 0; z--) f(0, 0, 0);
  }
}

// ONE thread: the sorted histogram of T (sym, key, used) -> lengths, codes, the header's bits and the body's size.
__device__ void build_code(Tree& T) {
  const int m = T.used;                                        // >= 2: a literal and end-of-block
  int body = 0;
  for (int k = 0; k < m; k++) {                                // the extra bits and the distance bit of the matches
    const int s = T.sym[k];
    if (s > DF_EOB) body += T.key[k] * (length_extra_bits(s) + 1);
  }
  // key[] is consumed by the construction: the code bits of the body are summed from count[] below
  huff_levels(T.key, m, 15, T.level);
  for (int s = 0; s < 288; s++) T.len[s] = 0;
  int i = 0;
  for (int d = 15; d >= 1; d--)
    for (int k = T.level[d]; k > 0 && i < m; k--) T.len[T.sym[i++]] = (unsigned char)d;
  int code = 0;
  T.level[0] = 0;
  for (int d = 1; d <= 15; d++) {
    code = (code + T.level[d - 1]) << 1;
    T.next[d] = code;
  }
  int nlit = DF_EOB + 1;
  for (int s = 0; s < DF_SYMS; s++) {
    const int l = T.len[s];
    if (!l) continue;
    T.code[s] = (unsigned short)(__brev((unsigned)T.next[l]++) >> (32 - l));
    body += T.count[s] * l;
    if (s >= nlit) nlit = s + 1;
  }
  T.body_bits = body;

  // the code-length code: 19 symbols, sorted by insertion
  for (int s = 0; s < 19; s++) T.cl_count[s] = 0, T.cl_len[s] = 0;
  walk_lengths(T.len, nlit, [&](int s, int, int) { T.cl_count[s]++; });
  int cm = 0;
  for (int s = 0; s < 19; s++) {
    const int c = T.cl_count[s];
    if (!c) continue;
    int k = cm++;
    while (k > 0 && T.cl_key[k - 1] > c) {                    // equal counts keep symbol order: s rises
      T.cl_key[k] = T.cl_key[k - 1];
      T.cl_sym[k] = T.cl_sym[k - 1];
      k--;
    }
    T.cl_key[k] = c;
    T.cl_sym[k] = s;
  }
  if (cm == 1) {
    T.cl_len[T.cl_sym[0]] = 1;
    for (int d = 0; d < 16; d++) T.level[d] = 0;
    T.level[1] = 1;
  } else {
    huff_levels(T.cl_key, cm, 7, T.level);
    i = 0;
    for (int d = 7; d >= 1; d--)
      for (int k = T.level[d]; k > 0 && i < cm; k--) T.cl_len[T.cl_sym[i++]] = d;
  }
  code = 0;
  T.level[0] = 0;
  for (int d = 1; d <= 7; d++) {
    code = (code + T.level[d - 1]) << 1;
    T.next[d] = code;
  }
  for (int s = 0; s < 19; s++) {
    const int l = T.cl_len[s];
    T.cl_code[s] = l ? (int)(__brev((unsigned)T.next[l]++) >> (32 - l)) : 0;
  }
  const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 4;
  for (int k = 4; k < 19; k++)
    if (T.cl_len[order[k]]) hclen = k + 1;

  for (int k = 0; k < DF_HDR_WORDS; k++) T.hdr[k] = 0;
  SerialBits w{T.hdr, 0ull, 0, 0};
  w.put(0, 1);                                                 // BFINAL: the composer sets it
  w.put(2, 2);
  w.put((unsigned)(nlit - 257), 5);
  w.put(0, 5);
  w.put((unsigned)(hclen - 4), 4);
  for (int k = 0; k < hclen; k++) w.put((unsigned)T.cl_len[order[k]], 3);
  walk_lengths(T.len, nlit, [&](int s, int eb, int ev) {
    w.put((unsigned)T.cl_code[s], T.cl_len[s]);
    w.put((unsigned)ev, eb);
  });
  T.hdr[w.word] = (unsigned)w.acc;
  T.hdr_bits = w.word * 32 + w.n;
}

// A thread's LSB-first writer into the shared LDS bit buffer: the first and the last word it touches are shared with the
// neighbouring spans (atomic OR into zeros), the words between are its own.
struct SharedBits {
  unsigned* w;
  unsigned long long acc;
  int n, word;
  bool first;
  __device__ __forceinline__ SharedBits(unsigned* out, int bit) : w(out), acc(0ull), n(bit & 31), word(bit >> 5), first(true) {}
  __device__ __forceinline__ void put(unsigned v, int nb) {
    acc |= (unsigned long long)v << n;
    n += nb;
    if (n >= 32) {
      if (first)
        atomicOr(&w[word], (unsigned)acc);
      else
        w[word] = (unsigned)acc;
      first = false;
      word++;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0 && (unsigned)acc != 0u) atomicOr(&w[word], (unsigned)acc);
  }
};

__global__ __launch_bounds__(DF_THREADS) void deflate_chunk_kernel(const unsigned char* __restrict__ in, long in_bytes,
                                                                   const long* __restrict__ table, int chunk_bytes,
                                                                   unsigned char* __restrict__ scratch, long scratch_bytes,
                                                                   int* __restrict__ meta, long meta_chunks, long out_bytes,
                                                                   int lds_in_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];     // the chunk at its source phase; the segment
  __shared__ Tree trees[2];
  __shared__ int scan_a[DF_THREADS + 1], scan_b[DF_THREADS + 1];
  __shared__ int tot[DF_WAVES];
  __shared__ unsigned adler[2];
  __shared__ int chosen[3];                                               // coding, segment bytes, token bits

  const Entry e = df_entry(table + (long)blockIdx.y * DF_FIELDS, chunk_bytes, in_bytes, scratch_bytes, meta_chunks, out_bytes);
  if (!e.ok || (long)blockIdx.x >= e.chunks) return;
  const int c = blockIdx.x, t = threadIdx.x;
  const bool final = c == e.chunks - 1;
  const int n = (int)(final ? e.bytes - (long)c * chunk_bytes : chunk_bytes);
  const unsigned char* g = in + e.src + (long)c * chunk_bytes;
  const int phase = (int)(reinterpret_cast<uintptr_t>(g) & 15u);
  unsigned char* inb = lds + phase;
  unsigned char* out8 = lds + lds_in_bytes;
  unsigned* out32 = reinterpret_cast<unsigned*>(out8);

  // ---- stage the chunk
  {
    const int head = min((16 - phase) & 15, n), body = (n - head) >> 4;
    for (int v = t; v < body; v += DF_THREADS)
      *reinterpret_cast<uint4*>(inb + head + (v << 4)) = *reinterpret_cast<const uint4*>(g + head + (v << 4));
    const int tail0 = head + (body << 4), edge = head + (n - tail0);
    if (t < edge) {
      const int s = t < head ? t : tail0 + (t - head);
      inb[s] = g[s];
    }
  }
  for (int s = t; s < 288; s += DF_THREADS) {
    trees[0].count[s] = trees[1].count[s] = s == DF_EOB ? 1 : 0;
  }
  if (t < 2) adler[t] = 0u, trees[t].used = 0;
  __syncthreads();

  // ---- the span's pass: literal histogram, Adler partials, the run boundaries
  const int span = (n + DF_THREADS - 1) / DF_THREADS;
  const int lo = min(t * span, n), hi = min(lo + span, n);
  int last_ne = -1, first_ne = n;
  {
    unsigned sa = 0u;
    unsigned long long sb = 0ull;
    int cur = -1, cnt = 0;
    for (int i = lo; i < hi; i++) {
      const int b = inb[i];
      sa += (unsigned)b;
      sb += (unsigned long long)((unsigned)(n - i) * (unsigned)b);
      if (b != cur) {
        if (cnt) atomicAdd(&trees[0].count[cur], cnt);
        cur = b, cnt = 0;
      }
      cnt++;
      if (i == 0 || b != inb[i - 1]) {
        last_ne = i;
        if (first_ne == n) first_ne = i;
      }
    }
    if (cnt) atomicAdd(&trees[0].count[cur], cnt);
    if (lo < hi) {
      atomicAdd(&adler[0], sa);                       // <= 255 * 65535 in all
      atomicAdd(&adler[1], (unsigned)(sb % ADLER_MOD));
    }
  }
  const int incl_max = block_scan(last_ne, -1, [](int a, int b) { return a > b ? a : b; }, tot);
  scan_a[t + 1] = incl_max;
  scan_b[DF_THREADS - 1 - t] = first_ne;               // reversed: a prefix scan of it is a suffix scan
  if (t == 0) scan_a[0] = -1;
  __syncthreads();
  const int rev_min = block_scan(scan_b[t], n, [](int a, int b) { return a < b ? a : b; }, tot);
  const int before = scan_a[t];                        // over the threads below t
  __syncthreads();
  scan_b[DF_THREADS - 1 - t] = rev_min;                // now scan_b[u] = min of first_ne over the threads >= u
  if (t == 0) scan_b[DF_THREADS] = n;
  __syncthreads();
  const int after = scan_b[t + 1];

  // ---- the tokens of coding 2 -> the second histogram
  walk_tokens(inb, lo, hi, before, after, [&](int match, int v) { atomicAdd(&trees[1].count[match ? length_symbol(v) : v], 1); });
  __syncthreads();

  // ---- sort both histograms by (count, symbol): thread k of a half ranks symbols k and k + 256
  {
    Tree& T = trees[t >> 8];
    for (int s = t & 255; s < DF_SYMS; s += 256) {
      const int cs = T.count[s];
      if (cs == 0) continue;
      int rank = 0;
      for (int j = 0; j < DF_SYMS; j++) {
        const int cj = T.count[j];
        rank += (cj != 0 && (cj < cs || (cj == cs && j < s))) ? 1 : 0;
      }
      T.sym[rank] = (unsigned short)s;
      T.key[rank] = cs;
      atomicAdd(&T.used, 1);
    }
  }
  __syncthreads();
  if ((t & 255) == 0) build_code(trees[t >> 8]);
  __syncthreads();

  // ---- the three sizes; the lowest number on a tie
  if (t == 0) {
    int best = 0, bytes = n + 5;
    for (int k = 1; k <= 2; k++) {
      const int bits = trees[k - 1].hdr_bits + trees[k - 1].body_bits + (final ? 0 : 3);
      const int sz = ((bits + 7) >> 3) + (final ? 0 : 4);
      if (sz < bytes) best = k, bytes = sz;
    }
    chosen[0] = best, chosen[1] = bytes;
  }
  __syncthreads();
  const int coding = chosen[0], seg_bytes = chosen[1];

  if (coding == 0) {
    if (t == 0) {
      out8[0] = final ? 1 : 0;
      out8[1] = (unsigned char)(n & 255), out8[2] = (unsigned char)(n >> 8);
      out8[3] = (unsigned char)(~n & 255), out8[4] = (unsigned char)((~n >> 8) & 255);
    }
    for (int i = t; i < n; i += DF_THREADS) out8[5 + i] = inb[i];
  } else {
    const Tree& T = trees[coding - 1];
    for (int k = t; k < (seg_bytes + 3) >> 2; k += DF_THREADS) out32[k] = 0u;
    int bits = 0;
    if (coding == 1) {
      for (int i = lo; i < hi; i++) bits += T.len[inb[i]];
    } else {
      walk_tokens(inb, lo, hi, before, after, [&](int match, int v) {
        const int s = match ? length_symbol(v) : v;
        bits += T.len[s] + (match ? length_extra_bits(s) + 1 : 0);
      });
    }
    const int incl = block_scan(bits, 0, [](int a, int b) { return a + b; }, tot);       // its barriers order the zeroing too
    if (t == DF_THREADS - 1) chosen[2] = incl;
    SharedBits w(out32, T.hdr_bits + incl - bits);
    if (coding == 1) {
      for (int i = lo; i < hi; i++) {
        const int s = inb[i];
        w.put(T.code[s], T.len[s]);
      }
    } else {
      walk_tokens(inb, lo, hi, before, after, [&](int match, int v) {
        if (!match) {
          w.put(T.code[v], T.len[v]);
        } else {
          const int s = length_symbol(v), eb = length_extra_bits(s);
          const unsigned extra = (unsigned)(v - 3) & ((1u << eb) - 1u);          // then the distance code: one 0 bit
          w.put((unsigned)T.code[s] | (extra << T.len[s]), T.len[s] + eb + 1);
        }
      });
    }
    w.finish();
    for (int k = t; k < (T.hdr_bits + 31) >> 5; k += DF_THREADS)
      if (T.hdr[k]) atomicOr(&out32[k], T.hdr[k]);
    __syncthreads();
    if (t == 0) {
      if (final) atomicOr(&out32[0], 1u);
      SharedBits eob(out32, T.hdr_bits + chosen[2]);
      eob.put(T.code[DF_EOB], T.len[DF_EOB]);
      eob.finish();
      if (!final) {                                    // the marker's zeros are there already; FF FF closes it
        const int p0 = seg_bytes - 2, p1 = seg_bytes - 1;
        atomicOr(&out32[p0 >> 2], 255u << (8 * (p0 & 3)));
        atomicOr(&out32[p1 >> 2], 255u << (8 * (p1 & 3)));
      }
    }
  }
  __syncthreads();

  // ---- the segment -> its slot (16-byte aligned, df_slot bytes: the rounding of the last store stays inside)
  unsigned char* slot = scratch + e.scratch + (long)c * df_slot(chunk_bytes);
  for (int v = t; v < (seg_bytes + 15) >> 4; v += DF_THREADS)
    *reinterpret_cast<uint4*>(slot + (v << 4)) = *reinterpret_cast<const uint4*>(out8 + (v << 4));
  if (t == 0) {
    int* mrow = meta + (e.meta + c) * DF_META;
    mrow[0] = seg_bytes;
    mrow[1] = (int)(adler[0] % ADLER_MOD);
    mrow[2] = (int)(adler[1] % ADLER_MOD);
    mrow[3] = coding;
  }
}

__global__ __launch_bounds__(DF_PACK_THREADS) void deflate_pack_kernel(const long* __restrict__ table, long in_bytes,
                                                                       int chunk_bytes,
                                                                       const unsigned char* __restrict__ scratch,
                                                                       long scratch_bytes, const int* __restrict__ meta,
                                                                       long meta_chunks, unsigned char* __restrict__ out,
                                                                       long out_bytes, long* __restrict__ sizes) {
  __shared__ int red[DF_PACK_THREADS / 64];
  const Entry e = df_entry(table + (long)blockIdx.y * DF_FIELDS, chunk_bytes, in_bytes, scratch_bytes, meta_chunks, out_bytes);
  if (!e.ok || (long)blockIdx.x >= e.chunks) return;
  const int c = blockIdx.x, t = threadIdx.x;
  const int* m = meta + e.meta * DF_META;
  int part = 0;
  for (int j = t; j < c; j += DF_PACK_THREADS) part += m[j * DF_META];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if ((t & 63) == 0) red[t >> 6] = part;
  __syncthreads();
  long off = 2;
  for (int w = 0; w < DF_PACK_THREADS / 64; w++) off += red[w];
  const int seg = m[c * DF_META];
  if (seg < 1 || seg > chunk_bytes + 5 || off + seg + 4 > e.cap) return;      // written by deflate_chunk_kernel in this launch: never

  unsigned char* d = out + e.dst + off;
  const unsigned char* s = scratch + e.scratch + (long)c * df_slot(chunk_bytes);
  const unsigned* s32 = reinterpret_cast<const unsigned*>(s);
  const int head = min((int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u), seg);
  const int body = (seg - head) >> 4;
  const int w0 = head >> 2, sh = 8 * (head & 3);                 // every 16-byte group starts at the same byte of a slot word
  for (int v = t; v < body; v += DF_PACK_THREADS) {
    const unsigned* p = s32 + w0 + (v << 2);
    unsigned q[4];
    if (sh == 0) {
      q[0] = p[0], q[1] = p[1], q[2] = p[2], q[3] = p[3];
    } else {
      unsigned a = p[0];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const unsigned b = p[j + 1];                              // inside the slot: it has 16 bytes behind the segment bound
        q[j] = (a >> sh) | (b << (32 - sh));
        a = b;
      }
    }
    *reinterpret_cast<uint4*>(d + head + (v << 4)) = make_uint4(q[0], q[1], q[2], q[3]);
  }
  const int tail0 = head + (body << 4), edge = head + (seg - tail0);
  if (t < edge) {
    const int i = t < head ? t : tail0 + (t - head);
    d[i] = s[i];
  }
  if (t == 0 && c == 0) {
    out[e.dst] = 0x78;
    out[e.dst + 1] = 0x01;
  }
  if (t == 0 && c == e.chunks - 1) {
    unsigned long long A = 1ull, B = 0ull;
    for (long j = 0; j < e.chunks; j++) {
      const unsigned long long nj = (unsigned long long)(j == e.chunks - 1 ? e.bytes - j * chunk_bytes : chunk_bytes);
      B = (B + nj * A + (unsigned long long)m[j * DF_META + 2]) % ADLER_MOD;
      A = (A + (unsigned long long)m[j * DF_META + 1]) % ADLER_MOD;
    }
    d[seg] = (unsigned char)(B >> 8), d[seg + 1] = (unsigned char)(B & 255);
    d[seg + 2] = (unsigned char)(A >> 8), d[seg + 3] = (unsigned char)(A & 255);
    sizes[blockIdx.y] = off + seg + 4;
  }
}

}  // namespace

UNFLOW_API long unflow_deflate_segment_bound(int chunk_bytes) {
  return chunk_bytes >= 1 && chunk_bytes <= UNFLOW_DEFLATE_CHUNK_MAX ? (long)chunk_bytes + 5 : -1;
}

UNFLOW_API long unflow_deflate_stream_bound(long bytes, int chunk_bytes) {
  if (bytes < 1 || chunk_bytes < 1 || chunk_bytes > UNFLOW_DEFLATE_CHUNK_MAX) return -1;
  return 2 + bytes + 5 * ((bytes + chunk_bytes - 1) / chunk_bytes) + 4;
}

UNFLOW_API long unflow_deflate_slot_bytes(int chunk_bytes) {
  return chunk_bytes >= 1 && chunk_bytes <= UNFLOW_DEFLATE_CHUNK_MAX ? df_slot(chunk_bytes) : -1;
}

UNFLOW_API int unflow_deflate(const unsigned char* in, long in_bytes, const long* desc, int n, int max_chunks, int chunk_bytes,
                              unsigned char* scratch, long scratch_bytes, int* meta, long meta_chunks, unsigned char* out,
                              long out_bytes, long* sizes, unflow_stream_t stream) {
  if (!in || !desc || !scratch || !meta || !out || !sizes) return UNFLOW_ERR_NULL;
  if (chunk_bytes < 1 || chunk_bytes > UNFLOW_DEFLATE_CHUNK_MAX) return UNFLOW_ERR_UNSUPPORTED;
  if (n <= 0 || n > 65535 || max_chunks <= 0 || in_bytes <= 0 || scratch_bytes <= 0 || meta_chunks <= 0 || out_bytes <= 0)
    return UNFLOW_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(scratch) & 15) != 0 || (reinterpret_cast<uintptr_t>(meta) & 3) != 0) return UNFLOW_ERR_UNSUPPORTED;
  const int lds_in = 16 + (int)df_round16(chunk_bytes) + 16;                // any phase, and the rounding of the last 16-byte copy
  const int lds_out = (int)df_round16(chunk_bytes + 5) + 16;
  static DynLdsBook book{};
  (void)ensure_dyn_lds(reinterpret_cast<const void*>(&deflate_chunk_kernel), lds_in + lds_out, book);
  const dim3 grid(max_chunks, n);
  deflate_chunk_kernel<<<grid, DF_THREADS, lds_in + lds_out, as_stream(stream)>>>(in, in_bytes, desc, chunk_bytes, scratch,
                                                                                 scratch_bytes, meta, meta_chunks, out_bytes, lds_in);
  if (launch_status() != UNFLOW_OK) return UNFLOW_ERR_LAUNCH;
  deflate_pack_kernel<<<grid, DF_PACK_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(desc, in_bytes, chunk_bytes, scratch,
                                                                                          scratch_bytes, meta, meta_chunks, out,
                                                                                          out_bytes, sizes);
  return launch_status();
}
