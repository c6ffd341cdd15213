"""A small PNG writer with a chosen filter per row, for the device-decoder tests.  Vectorised with numpy: on the encode side every
predictor (left, up, upper left) is known from the image itself, so even large all-Paeth frames are written in milliseconds, and
the expected result of decoding is simply the array that was encoded — the slow host decoder is never needed for them."""
import struct
import zlib

import numpy as np

CTYPE_OF_CHANNELS = {1: 0, 2: 4, 3: 2, 4: 6}
FILTERS = (0, 1, 2, 3, 4)          # None, Sub, Up, Average, Paeth


def sample_bytes(arr):
    """uint8 / uint16 [h, w, ch] -> (uint8 [h, w * bpp] as PNG stores the samples (16 bit: big-endian), depth, colour type, bpp)."""
    a = np.asarray(arr)
    assert a.ndim == 3 and a.dtype in (np.uint8, np.uint16), (a.dtype, a.shape)
    h, w, ch = a.shape
    depth = 8 * a.dtype.itemsize
    b = np.ascontiguousarray(a.astype('>u2') if depth == 16 else a).view(np.uint8).reshape(h, w * ch * depth // 8)
    return b, depth, CTYPE_OF_CHANNELS[ch], ch * depth // 8


def filter_rows(rows, bpp, filters):
    """uint8 [h, stride] + one filter type per row -> the PNG scanline stream, uint8 [h, 1 + stride]."""
    x = rows.astype(np.int32)
    h, stride = x.shape
    filters = np.asarray(filters, dtype=np.int32).reshape(h)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if stride > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :-bpp] if stride > bpp else 0
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, paeth])[filters, np.arange(h)]
    out = np.empty((h, 1 + stride), dtype=np.uint8)
    out[:, 0] = filters
    out[:, 1:] = (x - pred) & 255
    return out


def chunk(typ, body):
    return struct.pack('>I', len(body)) + typ + body + struct.pack('>I', zlib.crc32(typ + body) & 0xffffffff)


def png_file(w, h, depth, ctype, stream, interlace=0, level=1):
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, interlace)) +
            chunk(b'IDAT', zlib.compress(bytes(stream), level)) + chunk(b'IEND', b''))


def encode_png(arr, filters, level=1):
    """uint8 / uint16 [h, w, ch] -> PNG bytes with row y filtered by filters[y] (an int: every row)."""
    rows, depth, ctype, bpp = sample_bytes(arr)
    h = rows.shape[0]
    if np.isscalar(filters):
        filters = [filters] * h
    return png_file(arr.shape[1], h, depth, ctype, filter_rows(rows, bpp, filters).tobytes(), level=level)


def random_image(rs, h, w, ch, depth, values=None):
    """Uniform random samples, or bytes drawn from `values` (every BYTE of a 16-bit sample)."""
    if values is None:
        b = rs.randint(0, 256, size=(h, w, ch, depth // 8))
    else:
        b = np.asarray(values)[rs.randint(0, len(values), size=(h, w, ch, depth // 8))]
    b = b.astype(np.uint8)
    if depth == 8:
        return b.reshape(h, w, ch)
    return (b[..., 0].astype(np.uint16) << 8) | b[..., 1]


def random_filters(rs, h, first=None):
    f = rs.randint(0, 5, size=h)
    if first is not None:
        f[0] = first
    return f
