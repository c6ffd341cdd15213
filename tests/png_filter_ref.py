"""The PNG row-filter rule of unflow_png_filter (include/unflow_hip.h) written out independently in numpy, and the inputs of the
encode tests.  Host only.

Rule: for every row the five filtered rows of the PNG specification (None, Sub, Up, Average on the 9-bit sum, Paeth with ties
left, up, upper left; missing neighbours 0); cost = sum over the bytes b of a candidate of (b < 128 ? b : 256 - b) = sum of
|int8(b)|; the filter of least cost, the lowest number on a tie."""
import numpy as np

FILTER_NAMES = ('None', 'Sub', 'Up', 'Average', 'Paeth')


def raw_bytes(img):
    """uint8 [h,w] / [h,w,3], uint16 or int16 [h,w,3] -> (uint8 [h, w * bpp] raw PNG bytes, bpp, depth, colour type)."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, ch = a.shape
    ctype = {1: 0, 3: 2}[ch]
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a).reshape(h, w * ch), ch, 8, ctype
    if a.dtype in (np.uint16, np.int16):
        be = np.ascontiguousarray(a).view(np.uint16).astype('>u2')
        return be.view(np.uint8).reshape(h, w * ch * 2), 2 * ch, 16, ctype
    raise ValueError(a.dtype)


def filter_rows(raw, bpp):
    """raw uint8 [h, n] -> (scanlines uint8 [h, 1 + n], filters int [h])."""
    raw = np.asarray(raw, dtype=np.uint8)
    h, n = raw.shape
    cur = raw.astype(np.int16)
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    left = np.zeros_like(cur)
    left[:, bpp:] = cur[:, :-bpp] if n > bpp else 0
    ul = np.zeros_like(cur)
    ul[:, bpp:] = up[:, :-bpp] if n > bpp else 0
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cands = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth])          # [5, h, n] int16
    cands = (cands & 255).astype(np.uint8)
    cost = np.abs(cands.view(np.int8).astype(np.int64)).sum(axis=2)                               # [5, h]; |int8(128)| = 128
    filters = np.argmin(cost, axis=0)                                                             # first minimum: lowest number
    out = np.empty((h, 1 + n), dtype=np.uint8)
    out[:, 0] = filters
    out[:, 1:] = cands[filters, np.arange(h)]
    return out, filters


def reference_scanlines(img):
    """image -> (scanlines uint8 [h, 1 + w * bpp], filters [h], (h, w, depth, ctype))."""
    raw, bpp, depth, ctype = raw_bytes(img)
    scan, filters = filter_rows(raw, bpp)
    a = np.asarray(img)
    return scan, filters, (a.shape[0], a.shape[1], depth, ctype)


def random_image(rng, h, w, kind):
    """kind 'gray8' (values 0 / 1 / anything), 'rgb8', 'rgb16': smooth structure plus noise, so that several filters occur."""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'gray8':
        return rng.randint(0, 256, size=(h, w)).astype(np.uint8)
    ch = 3
    base = (yy[..., None] * np.array([3, 5, 7]) + xx[..., None] * np.array([11, 2, 6])).astype(np.int64)
    if kind == 'rgb8':
        return ((base + rng.randint(0, 4, size=(h, w, ch))) & 255).astype(np.uint8)
    if kind == 'rgb16':
        return ((base * 97 + rng.randint(0, 300, size=(h, w, ch))) & 65535).astype(np.uint16)
    raise ValueError(kind)


def five_filter_case(kind, w=48, seed=0):
    """An image ('rgb8' or 'rgb16', [h, w, 3]) whose rows are built so that each of the five filters wins at least one row —
    asserted here on the reference's histogram, a condition on the inputs: a first row (random), then blocks of (random row,
    constructed row): small values -> None, a horizontal ramp -> Sub, a copy of the row above -> Up, ((left + up) >> 1) + small
    noise -> Average, a tilted plane -> Paeth; and an all-zero row."""
    rng = np.random.RandomState(seed)
    dtype, top = (np.uint8, 256) if kind == 'rgb8' else (np.uint16, 65536)
    rnd = lambda: rng.randint(0, top, size=(w, 3)).astype(np.int64)       # noqa: E731
    rows = [rnd()]                                                        # the first row
    # None: small values (the row above is random, so Up / Average / Paeth cost a lot; Sub of small noise costs more than it)
    rows += [rnd(), rng.randint(0, 3, size=(w, 3)).astype(np.int64) * (1 if kind == 'rgb8' else 257)]
    # Sub: a horizontal ramp with a large random start, under a random row
    ramp = (rng.randint(top // 4, top // 2, size=(1, 3)) + np.arange(w)[:, None] * (np.array([1, 2, 1]) if kind == 'rgb8'
                                                                                   else np.array([257, 514, 257]))) % top
    rows += [rnd(), ramp]
    # Up: a copy of the random row above
    r = rnd()
    rows += [r, r.copy()]
    # Average: x = ((left + up) >> 1) + small noise, per byte lane, built byte by byte on the raw bytes below
    rows += [rnd(), None]
    avg_at = len(rows) - 1
    # Paeth: a tilted plane a * x + b * y over two rows (the second row's bytes are predicted exactly by left + up - upper left)
    plane = lambda y: ((np.arange(w)[:, None] * np.array([5, 3, 2]) + y * np.array([2, 7, 4]) + 40) * (1 if kind == 'rgb8' else 257)) % top   # noqa: E731
    rows += [plane(0), plane(1), plane(2)]
    rows += [np.zeros((w, 3), dtype=np.int64)]                            # an all-zero row
    rows[avg_at] = np.zeros((w, 3), dtype=np.int64)
    img = np.stack(rows).astype(dtype)
    # fill the Average row on the raw bytes: byte x = ((left + up) >> 1) + noise in {0, 1}
    raw, bpp, _, _ = raw_bytes(img)
    raw = raw.copy()
    for x in range(raw.shape[1]):
        left = int(raw[avg_at, x - bpp]) if x >= bpp else 0
        raw[avg_at, x] = (((left + int(raw[avg_at - 1, x])) >> 1) + int(rng.randint(0, 2))) & 255
    if kind == 'rgb8':
        img = raw.reshape(img.shape)
    else:
        img = raw.reshape(img.shape[0], w, 3, 2).astype(np.uint16).dot(np.array([256, 1], dtype=np.uint16)).astype(np.uint16)
    _, filters, _ = reference_scanlines(img)
    hist = np.bincount(filters, minlength=5)
    assert (hist > 0).all(), "five_filter_case(%s): filter histogram %s" % (kind, hist.tolist())
    assert filters[-1] == 0 and not img[-1].any()
    return img
