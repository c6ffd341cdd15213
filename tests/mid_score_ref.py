"""The definition of unflow_sequence_interpolate_score (include/unflow_hip.h) in numpy, its cases and the comparator of
tests/test_mid_score_gpu.py, proven without a GPU by tests/test_mid_score_cpu.py.  Not a test file.

The bytes come from mid_ref's quantisation (imported, not restated), the window sums are differences of int64 cumulative sums, the
SSIM expression is one numpy fp64 operation per rounding of the definition, and the sum over the windows is math.fsum, the exactly
rounded sum: so sse is compared by equality and ssim within ssim_bound, which is derived from the kernel's summation shape.

Mutants (MUTANTS) are deliberate mistakes of the mirror; tests/test_mid_score_cpu.py shows that each changes a case."""
import functools
import math

import numpy as np

import mid_ref as M
import warp_parity as WP

F32 = np.float32
KINDS = ('mid', 'blend', 'nearest')
WIN = 8
C1, C2 = 26634.24, 239708.16     # 4096 (0.01 * 255)^2, 4096 (0.03 * 255)^2
TILE_X, TILE_Y, CAP = 32, 16, 512        # the kernel's tile of window origins and its block cap per slot (csrc/interpolate_score.hip)
MUTANTS = ('window7', 'crossing', 'pitch_w', 'blend_swap', 'tie_im1', 'sse_halo', 'prev_slot0')
FULL_STEP = (2, -1)              # the integer translation per FULL-RATE frame of the synthetic clips (x, y)
SENTINEL_SSE, SENTINEL_SSIM = -777, -777.25


def quant(a):
    """mid_ref's 8.8 quantisation of staged values (uint8 or fp32) as int64; a NaN is 0, as fmaxf(c, 0) makes it on the device."""
    a = a.astype(np.float32)
    return M.quant(np.where(np.isnan(a), F32(0), a))


def byte_of(a):
    """The byte of staged values: (q + 128) / 256 by integer division; the byte itself for uint8."""
    return (quant(a) + 128) // 256


def _corner(im, h, w, pitch):
    """The (h, w) corner of a [Hmax, Wmax, 3] buffer read with rows `pitch` pixels apart."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return im.reshape(-1, 3)[(yy * pitch + xx).reshape(-1)].reshape(h, w, 3)


def candidates(im0, im1, mid, n, j, mutant=None):
    """The three candidates' bytes [3][h, w, 3] int64 of in-between frame j: im0, im1 staged values [h, w, 3], mid uint8 [h, w, 3]."""
    q0, q1 = quant(im0), quant(im1)
    a0, a1 = (j, n + 1 - j) if mutant == 'blend_swap' else (n + 1 - j, j)
    blend = (a0 * q0 + a1 * q1 + 128 * (n + 1)) // (256 * (n + 1))
    first = 2 * j < n + 1 if mutant == 'tie_im1' else 2 * j <= n + 1
    return [mid.astype(np.int64), blend, byte_of(im0 if first else im1)]


def _window_sums(a, k, crossing):
    """The sums over every k x k window of a [h, w, 3] int64, by cumulative sums: [h - k + 1, w - k + 1, 3] (empty when the frame is
    smaller than the window).  crossing (a mutant): the windows at all h x w origins, zeros beyond the frame."""
    if crossing:
        a = np.pad(a, ((0, k - 1), (0, k - 1), (0, 0)))
    h, w = a.shape[:2]
    if h < k or w < k:
        return np.zeros((0, 0, 3), np.int64)
    c = np.zeros((h + 1, w + 1, 3), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def ssim_terms(x, y, mutant=None):
    """The SSIM of every window of candidate x against truth y ([h, w, 3] int64 bytes): fp64 [h - 7, w - 7, 3], one numpy operation
    per rounding of the definition."""
    k = 7 if mutant == 'window7' else WIN
    S = lambda a: _window_sums(a, k, mutant == 'crossing')       # noqa: E731
    Sx, Sy, Sxx, Syy, Sxy = S(x), S(y), S(x * x), S(y * y), S(x * y)
    vx, vy, cxy = 64 * Sxx - Sx * Sx, 64 * Syy - Sy * Sy, 64 * Sxy - Sx * Sy
    for v in (2 * Sx * Sy, Sx * Sx + Sy * Sy, vx + vy, 2 * cxy):
        assert v.size == 0 or np.abs(v).max() < 2 ** 53
    a1 = (2 * Sx * Sy).astype(np.float64) + C1
    a2 = (2 * cxy).astype(np.float64) + C2
    b1 = (Sx * Sx + Sy * Sy).astype(np.float64) + C1
    b2 = (vx + vy).astype(np.float64) + C2
    num = a1 * a2
    den = b1 * b2
    return num / den


def _halo_weight(h, w):
    """Mutant sse_halo: how many tiles' halo regions (TILE + 7 to the right and below) hold each pixel."""
    def axis(n, t):
        c = np.zeros(n, np.int64)
        for o in range(0, n, t):
            c[o:o + t + WIN - 1] += 1
        return c
    return axis(h, TILE_Y)[:, None] * axis(w, TILE_X)[None, :]


def score_pair(im0, im1, mids, truths, h, w, n, mutant=None):
    """The scores of one pair: im0, im1 [Hmax, Wmax, 3] staged frames, mids uint8 [n, Hmax, Wmax, 3], truths [n, Hmax, Wmax, 3] in the
    staged dtype.  Returns (sse int64 [n, 3], ssim fp64 [n, 3], the sums of |SSIM| [n, 3] that ssim_bound takes)."""
    pitch = w if mutant == 'pitch_w' else im1.shape[1]
    a, b = _corner(im0, h, w, pitch), _corner(im1, h, w, pitch)
    sse, ssim, mag = np.zeros((n, 3), np.int64), np.zeros((n, 3)), np.zeros((n, 3))
    for j in range(1, n + 1):
        T = byte_of(_corner(truths[j - 1], h, w, pitch))
        for k, X in enumerate(candidates(a, b, _corner(mids[j - 1], h, w, pitch), n, j, mutant)):
            assert X.min() >= 0 and X.max() <= 255 and T.min() >= 0 and T.max() <= 255
            e2 = ((X - T) ** 2).sum(-1)
            sse[j - 1, k] = int((e2 * _halo_weight(h, w)).sum()) if mutant == 'sse_halo' else int(e2.sum())
            s = ssim_terms(X, T, mutant).reshape(-1)
            ssim[j - 1, k], mag[j - 1, k] = math.fsum(s), math.fsum(np.abs(s))
    return sse, ssim, mag


def windows(h, w):
    return max(h - WIN + 1, 0) * max(w - WIN + 1, 0)


def replay(case, prev, mutant=None):
    """One launch on `case` with prev [Hmax, Wmax, 3] (None while the carry source is 0: never read): ({scored slot: (sse, ssim,
    mag)}, the prev the launch leaves).  Mutant prev_slot0: prev is taken from frame slot 0, not from the last new frame."""
    h, w, n, fr = case['h'], case['w'], case['n'], case['frames']
    outs = {}
    for i in case['scored']:
        assert i > 0 or case['carry'] > 0
        outs[i] = score_pair(prev if i == 0 else fr[i - 1], fr[i], case['out_mid'][:, i], case['truth'][:, i], h, w, n, mutant)
    new_prev = np.zeros(fr.shape[1:], fr.dtype) if prev is None else prev.copy()
    new_prev[:h, :w] = fr[0 if mutant == 'prev_slot0' else case['k'] - 1, :h, :w]
    return outs, new_prev


def sum_depth(case):
    """The roundings on the longest path of the kernel's fixed-order fp64 sum: a thread's terms of one tile (2 origins x 3 channels),
    the wave's shuffle tree (6), the four waves (3), the block's tiles one after the other, the last block's lane over the partials
    (blocks / 64) and its tree (6)."""
    cd = lambda a, b: -(-a // b)          # noqa: E731
    blocks = min(cd(case['Wmax'], TILE_X) * cd(case['Hmax'], TILE_Y), CAP)
    tiles = cd(case['w'], TILE_X) * cd(case['h'], TILE_Y)
    return 6 + 6 + 3 + cd(tiles, blocks) + cd(blocks, 64) + 6


def ssim_bound(case, mag):
    """|kernel's sum - fsum| at the most, derived, not tuned: a term is six fp64 roundings of exact inputs (two adds and two more in
    the other factor, two products, one quotient: at most 6 * 2^-53 < 2^-50 relative, on terms of magnitude at most 1), and a sum
    along a path of d roundings is within d * 2^-53 * sum |term| (to first order; 2^-50 leaves room for the second)."""
    return mag * (2.0 ** -50 + sum_depth(case) * 2.0 ** -53)


def compare(case, outs, out_sse, out_ssim):
    """What one launch left in out_sse, out_ssim [n][Brows][3] (filled with the sentinels before) against the mirror's outs: sse equal,
    ssim within ssim_bound, the sentinels everywhere else.  Returns the worst observed fraction of the bound."""
    assert sorted(outs) == list(case['scored'])
    keep = np.ones(out_sse.shape, bool)
    worst = 0.0
    for i, (sse, ssim, mag) in outs.items():
        assert np.array_equal(out_sse[:, i], sse), ("slot %d: sse" % i, out_sse[:, i], sse)
        err, bound = np.abs(out_ssim[:, i] - ssim), ssim_bound(case, mag)
        assert (err <= bound).all(), ("slot %d: ssim" % i, out_ssim[:, i], ssim, err, bound)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
        keep[:, i] = False
    assert (out_sse[keep] == SENTINEL_SSE).all() and (out_ssim[keep] == SENTINEL_SSIM).all(), "slots that are not scored were written"
    return worst


# ------------------------------------------------------------------------------------------------- inputs
TRUTHS = ('self', 'offset', 'noise', 'texture')
SMALL = dict(B=2, Hmax=16, Wmax=24)
SHAPES = {'ragged': M.RAGGED, '9x11': dict(SMALL, h=9, w=11), '8x8': dict(SMALL, h=8, w=8), '7x20': dict(SMALL, h=7, w=20),
          'past-the-cap': M.BIG}


def draw_clip(rs, pairs, n, Hmax, Wmax, h, w, u8):
    """A full-rate clip of pairs * (n + 1) + 1 frames [., Hmax, Wmax, 3]: one random canvas seen through a window that moves by
    -FULL_STEP per frame, so every frame is the one before translated by FULL_STEP.  Outside the (h, w) corner: 255 / 1e3."""
    count = pairs * (n + 1) + 1
    pad_x, pad_y = abs(FULL_STEP[0]) * count, abs(FULL_STEP[1]) * count
    canvas = rs.randint(0, 256, size=(h + 2 * pad_y, w + 2 * pad_x, 3))
    if not u8:
        canvas = np.clip(canvas + rs.rand(*canvas.shape) * 0.999 - 0.5, 0, 255)
    out = np.full((count, Hmax, Wmax, 3), 255 if u8 else 1e3, np.uint8 if u8 else np.float32)
    for k in range(count):
        oy, ox = pad_y - FULL_STEP[1] * k, pad_x - FULL_STEP[0] * k
        out[k, :h, :w] = canvas[oy:oy + h, ox:ox + w]
    return out


def make_case(name, B, Hmax, Wmax, h, w, n, u8, pattern, truth, unheld=(), interp=True, seed=0):
    """One launch: the tables (held = 1; the slots of `unheld` with held = 0), the staged network frames of a translated full-rate
    clip, out_mid (interp: mid_ref's in-between frames on the true constant flow, else the true frames plus byte noise), and truth
    frames of kind `truth`.  fp32: out-of-range values and NaN are planted in the frames and the truths AFTER out_mid is formed (the
    scores take out_mid as it is)."""
    from unflow_amd.core.inference import sequence_tables
    rs = WP._rs('mid-score', name, n, u8, pattern, truth, seed)
    k, carry = M.PATTERNS[pattern]
    k = B if k is None else k
    carry = B if carry is None else carry
    tab, valid, _ = sequence_tables((h, w), k, B, carry, u8=u8, held=1)
    for i in unheld:
        assert i in valid
        tab[8 * B + 8 * i + 6] = 0
    clip = draw_clip(rs, B, n, Hmax, Wmax, h, w, u8)
    net = np.ascontiguousarray(clip[::n + 1])                     # prev, then the B staged frames
    true = np.stack([clip[j::n + 1][:B] for j in range(1, n + 1)])      # [n, B, ...]: frame j of pair slot i
    out_mid = np.full((n, B, Hmax, Wmax, 3), 0x5A, np.uint8)
    flow = np.full((Hmax, Wmax, 2), np.nan, np.float32)
    flow[:h, :w] = np.asarray(FULL_STEP, np.float32) * F32(n + 1)
    for i in valid:
        if interp:
            out_mid[:, i, :h, :w] = M.interpolate_pair(net[i], net[i + 1], flow, None, None, None, h, w, n)[0]
        else:
            out_mid[:, i, :h, :w] = np.clip(byte_of(true[:, i, :h, :w]) + rs.randint(-3, 4, size=(n, h, w, 3)), 0, 255)
    dt = np.uint8 if u8 else np.float32
    if truth == 'self':
        tr = out_mid.astype(dt)
    elif truth == 'offset':
        tr = np.clip(out_mid.astype(np.int64) + 5, 0, 255).astype(dt)
    elif truth == 'noise':
        tr = rs.randint(0, 256, size=out_mid.shape).astype(dt)
        if not u8:
            tr = (tr + rs.rand(*tr.shape).astype(np.float32) * F32(40) - F32(20)).astype(np.float32)      # below 0 and above 255 too
    else:
        tr = true.copy()
    net = net.copy()
    if not u8:                                                    # NaN, infinities and out-of-range values, frames and truths
        bad = (np.nan, np.inf, -np.inf, -3.5, 255.4, 300.0, 1e9, -0.0)
        for m, val in enumerate(bad):
            net[(m % (B + 1)), (3 * m + 1) % h, (5 * m + 2) % w, m % 3] = val
            tr[m % n, m % B, (2 * m + 3) % h, (7 * m + 1) % w, (m + 1) % 3] = val
    return dict(name=name, B=B, Hmax=Hmax, Wmax=Wmax, h=h, w=w, n=n, u8=u8, pattern=pattern, k=k, carry=carry, tab=tab, valid=valid,
                scored=[i for i in valid if i not in unheld], prev=net[0].copy(), frames=np.ascontiguousarray(net[1:]),
                out_mid=out_mid, truth=np.ascontiguousarray(tr), true=true,
                id='%s-n%d-%s-%s-%s%s' % (name, n, 'u8' if u8 else 'f32', pattern, truth, '-unheld' if unheld else ''))


def prev_of(case):
    return case['prev'] if case['carry'] > 0 else None


@functools.lru_cache(maxsize=None)
def entry_cases():
    """(id, case): the ragged shape with n in {1, 3}, uint8 and fp32 and the four truths crossed over them; every replay pattern; a
    pair that is not held out; the three small shapes (2 x 4 windows, one window, none); one pair past the block cap."""
    out = []
    for a, truth in enumerate(TRUTHS):
        for b, n in enumerate((1, 3)):
            for u8 in (True, False):
                if (a + b + u8) % 2 == 0 or truth == 'texture':
                    out.append(make_case('ragged', n=n, u8=u8, pattern='full', truth=truth, **M.RAGGED))
    for m, pattern in enumerate(('first', 'nopairs', 'short', 'short2')):
        out.append(make_case('ragged', n=(1, 3)[m % 2], u8=m < 2, pattern=pattern, truth='texture', **M.RAGGED))
    out.append(make_case('ragged', n=3, u8=True, pattern='full', truth='noise', unheld=(1,), **M.RAGGED))
    for m, shape in enumerate(('9x11', '8x8', '7x20')):
        out.append(make_case(shape, n=(3, 1, 3)[m], u8=m != 1, pattern='full', truth='texture', **SHAPES[shape]))
    out.append(make_case('past-the-cap', n=1, u8=True, pattern='full', truth='texture', interp=False, **M.BIG))
    return [(c['id'], c) for c in out]


@functools.lru_cache(maxsize=None)
def mirror_of(cid):
    """replay of entry case `cid` from its own prev, computed once and shared: (outs, new prev).  Read-only."""
    case = dict(entry_cases())[cid]
    return replay(case, prev_of(case))
