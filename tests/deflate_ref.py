"""The deflate rule of unflow_deflate (include/unflow_hip.h, csrc/deflate.hip) written out independently in Python / numpy, and
the inputs of the deflate tests.  Host only; imports nothing from the package.

Rule.  A stream of n bytes is cut into chunks of chunk_bytes (<= CHUNK_MAX); chunk c becomes one segment, coded on its own (no
match reaches before the chunk's first byte), and the zlib stream is 78 01, the segments back to back, Adler-32 big-endian.

A segment is one deflate block (RFC 1951), BFINAL set in the last chunk's, in the coding of least segment BYTES among
  0 stored:    byte BFINAL, LEN, NLEN (little-endian), the chunk's bytes: 5 + n bytes, byte-aligned by itself (no marker);
  1 dynamic Huffman over the literals and end-of-block only;
  2 dynamic Huffman over literals and distance-1 matches: a maximal run of L >= 3 bytes that equal their predecessor becomes
    L // 258 matches of 258 and then, for r = L % 258, one match of r if r >= 3, else r literals;
the lowest number on a tie.  A Huffman segment that is not the last ends with the sync marker: the three header bits of an empty
stored block, zero bits to the byte boundary, 00 00 FF FF.  The last ends with zero bits to the byte boundary.

Code lengths (huff_lengths), for the literal / length alphabet (limit 15) and the code-length alphabet (limit 7): the used symbols
sorted by (count, symbol); one used symbol gets length 1; otherwise the in-place minimum-redundancy construction of Moffat and
Katajainen on the sorted counts gives the number of leaves per depth, depths above the limit are counted at the limit, and while
the Kraft sum exceeds 1 one leaf is taken from the limit and the deepest non-empty level below the limit gives one leaf to the next
level as two (the sum falls by exactly one unit each time); then the levels are dealt out from the deepest: the least (count,
symbol) gets the longest code.  Codes are canonical (RFC 1951 3.2.2).

The block header: HLIT = last used literal / length symbol - 256 (end-of-block is always used), HDIST = 0: ONE distance code, of
length 1, in both Huffman codings (an incomplete one-code tree, which the RFC allows); its code is the bit 0 and distance 1 has no
extra bits.  The sequence of HLIT + 257 + 1 code lengths is sent with symbols 0..15, 17 and 18 only: a maximal run of z zeros is cut
greedily into pieces t = min(z, 138) while z >= 3 (18 for t >= 11, else 17) and the 0..2 zeros left are sent as they are."""
import zlib

import numpy as np

CHUNK_MAX = 65535
CHUNK_DEFAULT = 16384
MAX_MATCH = 258
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# the most a Huffman segment carries beyond its coded literals and matches: the 17 fixed header bits, 19 x 3 bits of code-length
# code lengths, at most 7 bits per sent code length (a 17 / 18 costs at most 14 bits for 3 or more), end-of-block (<= 15 bits),
# and the marker (3 bits, the padding inside the same byte count, 4 bytes)
HEADER_BOUND_BYTES = (17 + 57 + 287 * 7 + 15 + 7) // 8 + 5

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def length_symbol(length):
    """match length 3..258 -> (symbol 257..285, extra bits, extra value), from the table of RFC 1951 3.2.5."""
    k = max(i for i, b in enumerate(_LEN_BASE) if b <= length)
    return 257 + k, _LEN_EXTRA[k], length - _LEN_BASE[k]


def tokens(chunk, coding):
    """[(0, byte) | (1, length), ...] of one chunk (bytes) in coding 1 or 2."""
    n = len(chunk)
    if coding == 1:
        return [(0, b) for b in chunk]
    out, i = [(0, chunk[0])], 1
    while i < n:
        if chunk[i] != chunk[i - 1]:
            out.append((0, chunk[i]))
            i += 1
            continue
        q = i
        while q < n and chunk[q] == chunk[q - 1]:
            q += 1
        L = q - i
        if L < 3:
            out += [(0, chunk[i])] * L
        else:
            r = L % MAX_MATCH
            out += [(1, MAX_MATCH)] * (L // MAX_MATCH)
            out += [(1, r)] if r >= 3 else [(0, chunk[i])] * r
        i = q
    return out


def leaves_per_depth(a):
    """Sorted (ascending) counts of m >= 2 symbols -> {depth: leaves} of a minimum-redundancy code (Moffat and Katajainen, in
    place: a[] holds counts, then parent indices, then depths of internal nodes)."""
    a, m = list(a), len(a)
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= m or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    hist, avail, depth, root = {}, 1, 0, m - 2
    while avail > 0:
        used = 0
        while root >= 0 and a[root] == depth:
            used += 1
            root -= 1
        if avail > used:
            hist[depth] = avail - used
        avail, depth = 2 * used, depth + 1
    return hist


def huff_lengths(counts, limit):
    """counts [n] -> code lengths [n] (0 = unused)."""
    syms = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    lens = [0] * len(counts)
    if len(syms) == 1:
        lens[syms[0]] = 1
    if len(syms) < 2:
        return lens
    level = [0] * (limit + 1)
    for d, k in leaves_per_depth([counts[s] for s in syms]).items():
        level[min(d, limit)] += k
    total = sum(level[d] << (limit - d) for d in range(1, limit + 1))
    while total > 1 << limit:
        level[limit] -= 1
        for d in range(limit - 1, 0, -1):
            if level[d]:
                level[d] -= 1
                level[d + 1] += 2
                break
        total -= 1
    i = 0
    for d in range(limit, 0, -1):
        for _ in range(level[d]):
            lens[syms[i]] = d
            i += 1
    return lens


def canonical_codes(lens):
    """code lengths -> codes (RFC 1951 3.2.2), as integers to be sent from the most significant bit."""
    top = max(lens) if lens else 0
    count = [0] * (top + 2)
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = nxt[v]
            nxt[v] += 1
    return out


class Bits:
    """An LSB-first bit string."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits

    def code(self, code, nbits):            # a Huffman code: most significant bit first
        self.put(int(format(code, '0%db' % nbits)[::-1], 2) if nbits else 0, nbits)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, 'little')


def length_sequence(lens):
    """The code lengths of a block -> [(code-length symbol, extra bits, extra value), ...] by the rule in the module docstring."""
    out, i = [], 0
    while i < len(lens):
        if lens[i]:
            out.append((lens[i], 0, 0))
            i += 1
            continue
        z = 0
        while i + z < len(lens) and lens[i + z] == 0:
            z += 1
        i += z
        while z >= 3:
            t = min(z, 138)
            out.append((18, 7, t - 11) if t >= 11 else (17, 3, t - 3))
            z -= t
        out += [(0, 0, 0)] * z
    return out


def huffman_segment(chunk, coding, final):
    toks = tokens(chunk, coding)
    counts = [0] * 286
    counts[256] = 1
    for kind, v in toks:
        counts[v if kind == 0 else length_symbol(v)[0]] += 1
    lens = huff_lengths(counts, 15)
    codes = canonical_codes(lens)
    nlit = max(s for s in range(286) if lens[s]) + 1
    seq = length_sequence(lens[:nlit] + [1])
    cl_counts = [0] * 19
    for s, _, _ in seq:
        cl_counts[s] += 1
    cl_lens = huff_lengths(cl_counts, 7)
    cl_codes = canonical_codes(cl_lens)
    hclen = max(max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1, 4)
    w = Bits()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(nlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    for s, eb, ev in seq:
        w.code(cl_codes[s], cl_lens[s])
        w.put(ev, eb)
    for kind, v in toks:
        if kind == 0:
            w.code(codes[v], lens[v])
        else:
            s, eb, ev = length_symbol(v)
            w.code(codes[s], lens[s])
            w.put(ev, eb)
            w.put(0, 1)                      # the one distance code: distance 1
    w.code(codes[256], lens[256])
    if final:
        return w.bytes()
    w.put(0, 3)
    return w.bytes() + b'\x00\x00\xff\xff'


def segment(chunk, final):
    """One chunk -> (segment bytes, coding)."""
    n = len(chunk)
    best = bytes([1 if final else 0, n & 255, n >> 8, (n & 255) ^ 255, (n >> 8) ^ 255]) + bytes(chunk)
    coding = 0
    for c in (1, 2):
        s = huffman_segment(chunk, c, final)
        if len(s) < len(best):
            best, coding = s, c
    return best, coding


def adler32(data):
    """Adler-32 from per-chunk partial sums, as the kernels form it (not zlib's)."""
    a, b = 1, 0
    d = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64)
    for o in range(0, len(d), 4096):
        part = d[o:o + 4096]
        n = len(part)
        pa, pb = int(part.sum()), int((part * np.arange(n, 0, -1)).sum())
        b = (b + n * a + pb) % 65521
        a = (a + pa) % 65521
    return (b << 16) | a


def chunk_count(n, chunk_bytes=CHUNK_DEFAULT):
    return -(-n // chunk_bytes)


def deflate(data, chunk_bytes=CHUNK_DEFAULT, codings=None):
    """bytes (n >= 1) -> the zlib stream of the rule.  codings: a list that receives the coding of every chunk."""
    data = bytes(data)
    if not 1 <= chunk_bytes <= CHUNK_MAX or not data:
        raise ValueError("chunk_bytes in [1, %d] and at least one byte" % CHUNK_MAX)
    out = [b'\x78\x01']
    for o in range(0, len(data), chunk_bytes):
        seg, c = segment(data[o:o + chunk_bytes], o + chunk_bytes >= len(data))
        out.append(seg)
        if codings is not None:
            codings.append(c)
    out.append(adler32(data).to_bytes(4, 'big'))
    return b''.join(out)


def stream_bound(n, chunk_bytes=CHUNK_DEFAULT):
    """The most bytes deflate() returns for n bytes: stored wins at the latest."""
    return 2 + n + 5 * chunk_count(n, chunk_bytes) + 4


# ------------------------------------------------------------------------------------------------------------ test inputs
def fibonacci_bytes(n_symbols):
    """Bytes whose symbol counts follow the Fibonacci recurrence, shuffled, to be coded as ONE chunk: 1, 1, 3, 4, 7, 11, ... (the
    seeds 3, 4 rather than 2, 3, because the construction takes a leaf before an internal node of equal weight, and with 2, 3 the
    ties make the tree bushy).  With end-of-block (count 1) the unrestricted code is n_symbols deep — 16 symbols: 3569 bytes, 18:
    9347, 20: 24474, 22: 64077 — so the limit of 15 is passed and the repair rule runs; fibonacci_depth() is that depth, for the
    caller to assert."""
    fib = [1, 1, 3, 4]
    while len(fib) < n_symbols:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.RandomState(5)
    data = np.repeat(np.arange(n_symbols, dtype=np.uint8) * 7 + 3, fib[:n_symbols])
    return rng.permutation(data).tobytes()


def fibonacci_depth(data):
    counts = np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=256).tolist() + [1]
    return max(leaves_per_depth(sorted(c for c in counts if c)))


def runs_bytes(lengths, gap=2):
    """Runs of exactly the given lengths — a run of L is L bytes that equal their predecessor, so L + 1 equal bytes — each after
    `gap` bytes that differ from their neighbours."""
    out, v = [], 0
    for L in lengths:
        for _ in range(gap):
            v = (v + 37) & 255
            out.append(bytes([v]))
        v = (v + 37) & 255
        out.append(bytes([v]) * (L + 1))
    return b''.join(out)


def noisy_flow_scanlines(h=96, w=160, sigma=0.3, seed=2):
    """The filtered scanlines (Sub on every row: a fixed, stated choice) of a synthetic 16-bit KITTI flow map: smooth motion plus
    `sigma` px of noise, u16 = flow * 64 + 2^15, the valid channel 1.  Returns bytes."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    flow = np.stack([0.05 * xx + 0.02 * yy, 0.03 * yy - 4.0], axis=-1) + rng.randn(h, w, 2) * sigma
    px = np.concatenate([np.clip(np.round(flow * 64.0 + 32768.0), 0, 65535), np.ones((h, w, 1))], axis=-1).astype('>u2')
    raw = px.view(np.uint8).reshape(h, w * 6).astype(np.int16)
    sub = raw.copy()
    sub[:, 6:] -= raw[:, :-6]
    scan = np.empty((h, 1 + w * 6), dtype=np.uint8)
    scan[:, 0] = 1
    scan[:, 1:] = (sub & 255).astype(np.uint8)
    return scan.tobytes()


def mask_scanlines(h=96, w=160, seed=3):
    """Scanlines (filter None) of a 0 / 255 occlusion mask: a few rectangles."""
    rng = np.random.RandomState(seed)
    m = np.zeros((h, w), dtype=np.uint8)
    for _ in range(6):
        y, x = rng.randint(0, h - 8), rng.randint(0, w - 8)
        m[y:y + rng.randint(4, 30), x:x + rng.randint(4, 40)] = 255
    scan = np.zeros((h, 1 + w), dtype=np.uint8)
    scan[:, 1:] = m
    return scan.tobytes()


def zlib_stream(data, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(bytes(data)) + c.flush()


def noise_bytes(n, seed, top=40):
    """n bytes with a skewed histogram and hardly any runs: Huffman over literals wins on anything but a few bytes."""
    rng = np.random.RandomState(seed)
    return np.minimum(rng.randint(0, top, n), rng.randint(0, top, n)).astype(np.uint8).tobytes()


def fibonacci_symbols(chunk_bytes):
    """The most symbols whose fibonacci_bytes fit one chunk."""
    k = 4
    while len(fibonacci_bytes(k + 1)) <= chunk_bytes:
        k += 1
    return k


def cases(chunk_bytes):
    """[(name, bytes)]: the streams both deflate tests code at this chunk size — the lengths around a chunk (zeros and noise), all
    256 values uniformly (one chunk; stored must win), Fibonacci counts past depth 15 (one chunk), the run lengths around 3 and
    258, and a run that lies across a chunk boundary."""
    c = chunk_bytes
    out = []
    for k, n in enumerate((1, c - 1, c, c + 1, 2 * c + 3)):
        out += [('zeros_%d' % n, bytes(n)), ('noise_%d' % n, noise_bytes(n, 20 + k))]
    perm = np.random.RandomState(9).permutation(256).astype(np.uint8)
    out.append(('uniform', np.tile(perm, max(1, min(c, 8192) // 256)).tobytes()))
    out.append(('fibonacci', fibonacci_bytes(fibonacci_symbols(c))))
    out.append(('runs', runs_bytes([2, 3, 258, 259, 260, 516, 1, 257, 774])))
    out.append(('run_across', noise_bytes(c - 100, 31) + b'\x07' * 300 + noise_bytes(50, 32)))
    return out
