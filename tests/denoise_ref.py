"""The definition of unflow_sequence_denoise (include/unflow_hip.h) in numpy: its cases, the comparator of
tests/test_denoise_gpu.py and the noise scene of tests/test_denoise_cpu.py, which proves the mirror without a GPU.  Not a test file.

Everything is int64 except the flow's validity test and the rintf of its components (fp32, as on the device), so the comparison
with the kernel is equality on every output and on the state.

Mutants (MUTANTS) are deliberate mistakes of the mirror; the CPU test shows that each changes the result of at least one case."""
import functools

import numpy as np

import mid_ref as M
import track_ref as T
import warp_parity as WP

F32 = np.float32
LIMIT = F32(4096)                # a flow component of this magnitude (or not finite) makes the pixel FRESH
SIZE_MAX = 4096
TOLS, DEPTHS = (-1, 0, 1, 2, 3, 4), (1, 8, 64)
MUTANTS = ('in_place',           # rows updated in place: a tap reads the rows above it after their update
           'nearest_count',      # the count of the nearest tap in place of the minimum of the four
           'ignore_occ',         # the occlusion mask ignored
           'hist_all',           # the histogram over all pixels (a FRESH one in bin 0)
           'half_gt',            # M: the first bin with cum > half in place of >=
           'no_round',           # the rounding term of A' dropped
           'trunc',              # rintf becomes truncation
           'inside_off',         # INSIDE: PX < (w - 1) << 6 in place of <=
           'no_restart')         # the history not re-initialised at the start of a clip


def quant(c):
    """csrc/mid_common.h's 8.8 colour: fmaxf / fminf, so a NaN is 0."""
    assert c.dtype == np.float32
    return np.rint(np.fmin(np.fmax(c, F32(0)), F32(255)) * F32(256)).astype(np.int64)


def initial(hist, frame0, h0, w0, Hmax, Wmax):
    """The history at the start of a clip: q(frame-table slot 0), n = 1 on its (h, w); the rest is whatever the state holds."""
    hist = hist.copy()
    if 0 < h0 <= Hmax and 0 < w0 <= Wmax:
        hist[:h0, :w0, :3] = quant(np.ascontiguousarray(frame0[:h0, :w0]).astype(np.float32))
        hist[:h0, :w0, 3] = 1
    return hist


def _geometry(bw, occ, h, w, mutant=None):
    """(fresh, PX, PY) of a slot, int64 [h, w]; PX = PY = 0 where fresh."""
    flow = np.ascontiguousarray(bw[:h, :w])
    assert flow.dtype == np.float32
    with np.errstate(invalid='ignore'):
        valid = (np.abs(flow[..., 0]) < LIMIT) & (np.abs(flow[..., 1]) < LIMIT)
    f = np.where(valid[..., None], flow, F32(0)) * F32(64)
    assert f.dtype == np.float32
    UV = (np.trunc(f) if mutant == 'trunc' else np.rint(f)).astype(np.int64)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing='ij')
    PX, PY = (xx << 6) + UV[..., 0], (yy << 6) + UV[..., 1]
    off = 1 if mutant == 'inside_off' else 0
    inside = (PX >= 0) & (PX <= ((w - 1) << 6) - off) & (PY >= 0) & (PY <= ((h - 1) << 6) - off)
    masked = np.zeros((h, w), bool) if mutant == 'ignore_occ' else occ[:h, :w] != 0
    fresh = ~valid | ~inside | masked
    return fresh, np.where(fresh, 0, PX), np.where(fresh, 0, PY)


def _predict(src, PX, PY, h, w, mutant=None):
    """The four taps of the history src at (PX, PY), arrays of one shape: (pred [..., 3], np)."""
    ix, iy, qx, qy = PX >> 6, PY >> 6, PX & 63, PY & 63
    jx, jy = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    a, b, c, d = src[iy, ix], src[iy, jx], src[jy, ix], src[jy, jx]
    wx0, wx1, wy0, wy1 = (64 - qx)[..., None], qx[..., None], (64 - qy)[..., None], qy[..., None]
    s = wx0 * wy0 * a[..., :3] + wx1 * wy0 * b[..., :3] + wx0 * wy1 * c[..., :3] + wx1 * wy1 * d[..., :3]
    pred = (s + 2048) >> 12
    if mutant == 'nearest_count':
        n = np.where(qy < 32, np.where(qx < 32, a[..., 3], b[..., 3]), np.where(qx < 32, c[..., 3], d[..., 3]))
    else:
        n = np.minimum(np.minimum(a[..., 3], b[..., 3]), np.minimum(c[..., 3], d[..., 3]))
    return pred, n


def noise_level(E, counted):
    """(M, eligible): the median bin of E over the counted pixels."""
    hist = np.bincount(E[counted].reshape(-1), minlength=256)
    assert len(hist) == 256
    return hist, int(counted.sum())


def tolerance(tol, Mv):
    if tol >= 0:
        return tol
    return next((t for t in range(5) if (8 << t) >= 2 * Mv), 4)


def denoise_pair(frame, bw, occ, h, w, tol, depth, hist, mutant=None):
    """One valid pair: (dict(den uint8 [h, w, 3], stats int64 [8]), the history behind it).  hist int64 [Hmax, Wmax, 4]: the
    history before the pair (not changed)."""
    assert -1 <= tol <= 4 and 1 <= depth <= 64 and 1 <= h <= SIZE_MAX and 1 <= w <= SIZE_MAX and hist.dtype == np.int64
    cur = quant(np.ascontiguousarray(frame[:h, :w]).astype(np.float32))
    fresh, PX, PY = _geometry(bw, occ, h, w, mutant)
    pred, npv = _predict(hist, PX, PY, h, w, mutant)
    e = np.abs(pred - cur).sum(axis=-1)
    E = np.where(fresh, 0, np.minimum(e >> 8, 255))
    bins, eligible = noise_level(E, np.ones_like(fresh) if mutant == 'hist_all' else ~fresh)
    cum = np.cumsum(bins)
    half = (eligible + 1) // 2
    Mv = int((cum <= half).sum()) if mutant == 'half_gt' else int((cum < half).sum())
    t = tolerance(tol, Mv)
    rnd = 0 if mutant == 'no_round' else 1
    new = hist.copy()
    den = np.zeros((h, w, 3), np.uint8)
    nfresh = nrej = nsum = 0
    # the rows one by one only for the in-place mutant; the definition reads the history before the slot everywhere
    for y0, y1 in ([(y, y + 1) for y in range(h)] if mutant == 'in_place' else [(0, h)]):
        r = slice(y0, y1)
        if mutant == 'in_place':
            p, n = _predict(new, PX[r], PY[r], h, w, mutant)
            er = np.abs(p - cur[r]).sum(axis=-1)
        else:
            p, n, er = pred[r], npv[r], e[r]
        d = np.minimum(er >> (11 + t), 6)
        rejected = ~fresh[r] & (d == 6)
        neff = np.where(fresh[r] | rejected, 0, n >> d)
        A = (neff[..., None] * p + cur[r] + (((neff + 1) >> 1) * rnd)[..., None]) // (neff + 1)[..., None]
        nn = np.minimum(neff + 1, depth)
        new[r, :w, :3] = A
        new[r, :w, 3] = nn
        den[r] = ((A + 128) >> 8).astype(np.uint8)
        nfresh, nrej, nsum = nfresh + int(fresh[r].sum()), nrej + int(rejected.sum()), nsum + int(nn.sum())
    stats = np.array([t, Mv, eligible, nfresh, nrej, nsum, 0, 0], np.int64)
    return dict(den=den, stats=stats), new


def replay(case, state, mutant=None):
    """One launch: ({valid slot: denoise_pair's dict}, the state it leaves, uint16 [Hmax, Wmax, 4]).  state: the state on entry."""
    h, w, Hm, Wm = case['h'], case['w'], case['Hmax'], case['Wmax']
    hist = np.asarray(state).astype(np.int64).reshape(Hm, Wm, 4)
    if case['carry'] == 0 and mutant != 'no_restart':
        hist = initial(hist, case['frames'][0], int(case['tab'][0]), int(case['tab'][1]), Hm, Wm)
    outs = {}
    for i in case['valid']:
        outs[i], hist = denoise_pair(case['frames'][i], case['flow_bw'][i], case['occ'][i], h, w, case['tol'], case['depth'], hist,
                                     mutant)
    assert hist.min() >= 0 and hist.max() <= 0xffff
    return outs, hist.astype(np.uint16)


OUTPUTS = ('den', 'stats')


def compare(case, outs, got, sentinels):
    """The comparator of the GPU test: got = {name: what one launch left in that output, [Brows, ...] with Brows >= B, filled with
    sentinels[name] before the launch} against the mirror's outs: equal on every valid slot — every word and every pixel — and the
    sentinel everywhere else: slots that are no pairs, pixels outside (h, w), rows beyond B.  Returns the pixels compared."""
    h, w = case['h'], case['w']
    assert sorted(outs) == list(case['valid']) and sorted(got) == sorted(OUTPUTS)
    rest = {k: np.ones(got[k].shape, bool) for k in OUTPUTS}
    seen = 0
    for i, o in outs.items():
        assert np.array_equal(got['stats'][i].astype(np.int64), o['stats']), ("slot %d: stats" % i, got['stats'][i], o['stats'])
        rest['stats'][i] = False
        g = got['den'][i, :h, :w]
        bad = np.argwhere(g != o['den'])
        assert len(bad) == 0, ("slot %d: den differs at %d places, first %s: got %s, mirror %s"
                               % (i, len(bad), bad[0], g[tuple(bad[0])], o['den'][tuple(bad[0])]))
        rest['den'][i, :h, :w] = False
        seen += h * w
    for k in OUTPUTS:
        assert (got[k][rest[k]] == sentinels[k]).all(), "%s was written outside the valid pairs" % k
    return seen


# ------------------------------------------------------------------------------------------------- inputs
FLOW_KINDS = ('zero', 'shift', 'iid12', 'wild')
PATTERNS = M.PATTERNS            # first, nopairs, full (carried), short, short2 (two of three): (new frames, carry source)
RAGGED = dict(B=3, Hmax=40, Wmax=64, h=37, w=53)         # the pitch is not the width; more than one block per slot
FULL = dict(B=3, Hmax=40, Wmax=64, h=40, w=64)           # the frame fills its buffer
TINY = dict(B=3, Hmax=2, Wmax=3, h=1, w=1)               # one pixel: every tap is the pixel itself
BIG = dict(B=1, Hmax=600, Wmax=900, h=600, w=900)        # 540000 pixels: past the 2048 x 256 threads of a grid
STEP = M.STEP                    # the content of draw_frames' clips moves by STEP per frame: the backward flow is -STEP


def draw_frames(rs, B, Hmax, Wmax, h, w, u8, sigma=6.0):
    """[B, Hmax, Wmax, 3]: a smooth canvas with a little texture seen through a window that moves by -STEP per frame (frame k + 1
    is frame k translated by STEP), plus noise of its own per frame.  Outside the (h, w) corner: a constant the kernel must never
    read into a result (255 / 1e3)."""
    pad_x, pad_y = abs(STEP[0]) * B, abs(STEP[1]) * B
    yy, xx = np.meshgrid(np.arange(h + 2 * pad_y), np.arange(w + 2 * pad_x), indexing='ij')
    canvas = np.stack([128 + 70 * np.sin(xx / (7.0 + c) + c) * np.cos(yy / (5.0 + 2 * c)) for c in range(3)], axis=-1)
    canvas = canvas + rs.randn(*canvas.shape) * 12.0
    out = np.full((B, Hmax, Wmax, 3), 255 if u8 else 1e3, np.uint8 if u8 else np.float32)
    for k in range(B):
        oy, ox = pad_y - STEP[1] * k, pad_x - STEP[0] * k
        fr = np.clip(canvas[oy:oy + h, ox:ox + w] + rs.randn(h, w, 3) * sigma, 0, 255)
        out[k, :h, :w] = np.rint(fr) if u8 else fr
    return out


def draw_flows(rs, B, Hmax, Wmax, h, w, kind):
    """[B, Hmax, Wmax, 2] fp32 backward flows of `kind` in the (h, w) corner of every slot, NaN outside it (never to be read).
    zero; shift: -STEP, the clip's true motion (the taps of the last column and the first row touch the border exactly); iid12:
    i.i.d. +-12 px at sub-pixel positions (taps clamp and leave the frame); wild: shift with NaN, inf and 5000 px planted, and
    positions a 1/128 px either side of a tap boundary."""
    f = np.full((B, Hmax, Wmax, 2), np.nan, np.float32)
    if kind == 'zero':
        f[:, :h, :w] = 0
    elif kind in ('shift', 'wild'):
        f[:, :h, :w] = (-STEP[0], -STEP[1])
    elif kind == 'iid12':
        f[:, :h, :w] = (rs.rand(B, h, w, 2) * 24 - 12).astype(np.float32)
    else:
        raise ValueError(kind)
    if kind == 'wild':
        bad = (np.nan, np.inf, -np.inf, 4096.0, -4096.0, 4095.98, -4095.98, 5000.0, -5000.0, 1e7)
        for b in range(B):
            for m, val in enumerate(bad):
                f[b, (5 * m + b + 1) % h, (7 * m + 3 * b + 2) % w, (m + b) % 2] = val
            f[b, (b + 11) % h, (b + 13) % w] = (np.nan, np.inf)
            # halves of a 1/64 px step: rintf rounds to even, truncation does not
            f[b, h // 2, :w, 0] = (np.arange(w) % 7 - 3) + np.float32(0.5 / 64) * (2 * (np.arange(w) % 5) + 1)
            f[b, h // 2 + 1 if h > 1 else 0, :w, 1] = -(np.arange(w) % 3) * np.float32(1.5 / 64)
    return f


def draw_occ(rs, B, Hmax, Wmax, h, w, kind):
    """[B, Hmax, Wmax] uint8: 'none' (zero), 'random' (a fifth of the pixels, values 1 and 255) or 'blobs' (track_ref's discs) in the
    (h, w) corner, 1 outside it (never to be read)."""
    if kind == 'blobs':
        return T.draw_occ(rs, B, Hmax, Wmax, h, w)
    o = np.ones((B, Hmax, Wmax), np.uint8)
    o[:, :h, :w] = 0 if kind == 'none' else (rs.rand(B, h, w) < 0.2) * rs.choice([1, 255], size=(B, h, w))
    return o


def draw_state(rs, Hmax, Wmax, depth, carried):
    """uint16 [Hmax, Wmax, 4]: a history in mid-clip (colours anywhere in 0..65280, counts anywhere in 1..depth), or — nothing
    carried — poison no result may depend on."""
    if not carried:
        return rs.randint(0, 1 << 16, size=(Hmax, Wmax, 4)).astype(np.uint16)
    s = np.empty((Hmax, Wmax, 4), np.uint16)
    s[..., :3] = rs.randint(0, 65281, size=(Hmax, Wmax, 3))
    s[..., 3] = rs.randint(1, depth + 1, size=(Hmax, Wmax))
    return s


def make_case(name, B, Hmax, Wmax, h, w, u8, kind, occ, pattern, tol, depth, oversize=None, warm=False):
    """One launch: the tables of sequence_tables, B staged frames, the backward flows and masks, the options and the state on entry.
    oversize: a pair slot whose table row gets w = Wmax + 1 — no pair.  warm: the carried state is a history of the clip itself
    (the frame in front of it, counts of 1..depth), so that predictions are close and every d occurs."""
    from unflow_amd.core.inference import sequence_tables
    rs = WP._rs('denoise', name, u8, kind, occ, pattern, tol, depth, oversize, warm)
    k, carry = PATTERNS[pattern]
    k = B if k is None else k
    carry = B if carry is None else carry
    tab, valid, _ = sequence_tables((h, w), k, B, carry, u8=u8)
    if oversize is not None:
        tab = tab.copy()
        tab[8 * B + 8 * oversize + 1] = Wmax + 1
        valid = [i for i in valid if i != oversize]
    fr = draw_frames(rs, B + 1, Hmax, Wmax, h, w, u8)
    state = draw_state(rs, Hmax, Wmax, depth, carry > 0)
    if warm and carry:
        state[:h, :w, :3] = quant(np.ascontiguousarray(fr[0, :h, :w]).astype(np.float32))
    return dict(name=name, B=B, Hmax=Hmax, Wmax=Wmax, h=h, w=w, u8=u8, kind=kind, occ_kind=occ, pattern=pattern, k=k, carry=carry,
                tab=tab, valid=valid, frames=np.ascontiguousarray(fr[1:]), flow_bw=draw_flows(rs, B, Hmax, Wmax, h, w, kind),
                occ=draw_occ(rs, B, Hmax, Wmax, h, w, occ), tol=tol, depth=depth, state=state,
                id='%s-%s-%s-%s-%s-t%dd%d%s%s' % (name, 'u8' if u8 else 'f32', kind, occ, pattern, tol, depth,
                                                  '' if oversize is None else '-over%d' % oversize, '-warm' if warm else ''))


@functools.lru_cache(maxsize=None)
def entry_cases():
    """The launches of the entry-point tests, (id, case): every flow kind with every tolerance, the depths, the two frame types, the
    masks and the two shapes taking turns; every replay pattern in both frame types; an oversize slot; one pixel; one 600 x 900
    pair."""
    out, m = [], 0
    for kind in FLOW_KINDS:
        for tol in TOLS:
            shape = (RAGGED, FULL)[m % 2]
            out.append(make_case(('ragged', 'full')[m % 2], u8=(m // 2) % 2 == 0, kind=kind, occ=('random', 'none', 'blobs')[m % 3],
                                 pattern='full', tol=tol, depth=DEPTHS[(m // 2) % 3], warm=m % 4 < 2, **shape))
            m += 1
    for n, pattern in enumerate(('first', 'nopairs', 'short', 'short2')):
        for u8 in (False, True):
            out.append(make_case('ragged', u8=u8, kind=('shift', 'iid12')[n % 2], occ='random', pattern=pattern, tol=-1 if u8 else 2,
                                 depth=8, warm=True, **RAGGED))
    out.append(make_case('ragged', u8=True, kind='iid12', occ='random', pattern='full', tol=-1, depth=8, oversize=1, warm=True, **RAGGED))
    for pattern in ('full', 'first'):
        out.append(make_case('tiny', u8=pattern == 'full', kind='zero', occ='none', pattern=pattern, tol=-1, depth=8, **TINY))
    out.append(make_case('big', u8=True, kind='iid12', occ='blobs', pattern='full', tol=-1, depth=8, warm=True, **BIG))
    assert len({c['id'] for c in out}) == len(out)
    return [(c['id'], c) for c in out]


@functools.lru_cache(maxsize=None)
def mirror_of(cid):
    """replay of entry case `cid` from its own state, computed once and shared: (outs, new state).  Read-only."""
    case = dict(entry_cases())[cid]
    return replay(case, case['state'])


# ------------------------------------------------------------------------------------------------- the noise scene
SCENE = dict(H=40, W=64, T=12, side=16, x0=4, y0=12, speed=3)


@functools.lru_cache(maxsize=None)
def noise_scene(sigma, seed=0):
    """(clean float64 [T, H, W, 3], noisy uint8 [T, H, W, 3], bw fp32 [T - 1, H, W, 2], occ uint8 [T - 1, H, W]): a static smooth
    background, a textured square of `side` pixels that moves `speed` px per frame to the right, seeded Gaussian noise of standard
    deviation sigma; pair k (frames k, k + 1) has the exact backward flow on frame k + 1 (-speed on the square, 0 elsewhere) and
    the exact backward mask: the background that the square covered in frame k."""
    S = SCENE
    H, W, Tn, side = S['H'], S['W'], S['T'], S['side']
    rs = np.random.RandomState(1000 + seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    bg = np.stack([120 + 60 * np.sin(xx / (11.0 + 2 * c) + c) * np.cos(yy / (9.0 + c)) for c in range(3)], axis=-1)
    tex = rs.randint(30, 226, size=(side, side, 3)).astype(np.float64)
    clean = np.empty((Tn, H, W, 3))
    inside = np.zeros((Tn, H, W), bool)
    for k in range(Tn):
        x = S['x0'] + S['speed'] * k
        clean[k] = bg
        clean[k, S['y0']:S['y0'] + side, x:x + side] = tex
        inside[k, S['y0']:S['y0'] + side, x:x + side] = True
    noisy = np.rint(np.clip(clean + rs.randn(*clean.shape) * sigma, 0, 255)).astype(np.uint8)
    bw = np.zeros((Tn - 1, H, W, 2), np.float32)
    bw[..., 0] = np.where(inside[1:], -float(S['speed']), 0.0)
    occ = (inside[:-1] & ~inside[1:]).astype(np.uint8)
    for a in (clean, noisy, bw, occ):
        a.setflags(write=False)
    return clean, noisy, bw, occ


def filter_clip(noisy, bw, occ, tol=-1, depth=8):
    """The definition along a whole clip: (den uint8 [T - 1, H, W, 3] — frame k + 1 at [k] —, stats int64 [T - 1, 8])."""
    Tn, H, W = noisy.shape[:3]
    hist = initial(np.zeros((H, W, 4), np.int64), noisy[0], H, W, H, W)
    den, stats = [], []
    for k in range(Tn - 1):
        o, hist = denoise_pair(noisy[k + 1], bw[k], occ[k], H, W, tol, depth, hist)
        den.append(o['den'])
        stats.append(o['stats'])
    return np.stack(den), np.stack(stats)
