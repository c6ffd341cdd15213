"""The definition of unflow_sequence_interpolate (include/unflow_hip.h) in numpy, its cases, synthetic inputs and the
comparator of tests/test_interpolate_gpu.py, proven without a GPU by tests/test_interpolate_cpu.py.  Not a test file.

Every fp32 step of the definition is carried as fp32, one numpy operation per rounding (the library is built with
-ffp-contract=off, so the kernel rounds the same products and sums one by one); from the quantisation on everything is int64, and
integer sums do not depend on their order.  So the comparison with the kernel is equality, derived, not measured.

Mutants (MUTANTS) are deliberate mistakes of the mirror; tests/test_interpolate_cpu.py shows that each changes the result of at
least one case, i.e. that the case list would catch the same mistake in the kernel."""
import functools

import numpy as np

import track_ref as T
import warp_parity as WP

F32 = np.float32
LIMIT = F32(1e6)                 # a flow component of this magnitude (or not finite) contributes nothing
HOLE = 1024                      # weight sums below this are holes
N_MAX = 7
GRID_CAP = 2048 * 256            # the threads of one block row of the kernels' capped grid: more pixels take the grid-stride loop
MUTANTS = ('clamp', 'pitch_w', 'dir_swap', 'occ_blend', 'hole_x4', 'prev_slot0')
STEP = (4, -2)                   # the even-integer translation per frame of the synthetic clips (x, y)


def times(n, j):
    """(t, s) of in-between frame j of n, fp32 divisions."""
    return F32(j) / F32(n + 1), F32(n + 1 - j) / F32(n + 1)


def quant(c):
    """8.8 fixed point of fp32 colours in [0, 255]: (long)rintf(min(max(c, 0), 255) * 256)."""
    assert c.dtype == np.float32
    return np.rint(np.minimum(np.maximum(c, F32(0)), F32(255)) * F32(256)).astype(np.int64)


def _px(im, q):
    """The pixels at flat indices q of a [Hmax, Wmax, 3] frame (uint8 or fp32), as fp32."""
    return im.reshape(-1, 3)[q].astype(np.float32)


def _pass(here, other, flow, occ, h, w, pitch, w_here, w_other, a, Sc, Sw, mutant=None):
    """One splat pass of the definition into Sc [h, w, 3], Sw [h, w] int64: the pixels of `here` (im0 forward, im1 backward), blended
    with `other` warped by `flow`, moved by w_other * flow, tap weights times a.  Returns the sum of the kept taps' weights."""
    assert flow.dtype == np.float32 and w_here.dtype == np.float32 and w_other.dtype == np.float32
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    x, y = xx.reshape(-1).astype(np.int64), yy.reshape(-1).astype(np.int64)
    q = y * pitch + x
    f = flow.reshape(-1, 2)[q]
    with np.errstate(invalid='ignore'):
        ok = (np.abs(f[:, 0]) < LIMIT) & (np.abs(f[:, 1]) < LIMIT)       # NaN and inf compare false; before any integer conversion
    u, v = np.where(ok, f[:, 0], F32(0)), np.where(ok, f[:, 1], F32(0))
    idx, _, _, wts = T._taps(u, v, x, y, h, w, pitch, np.float32)
    wa, wb, wc, wd = (t[:, None] for t in wts)
    ta, tb, tc, td = (_px(other, i) for i in idx)
    warped = ((wa * ta + wb * tb) + wc * tc) + wd * td
    c0 = _px(here, q)
    c = w_here * c0 + w_other * warped
    assert c.dtype == np.float32
    if occ is not None and mutant != 'occ_blend':
        c = np.where((occ.reshape(-1)[q] != 0)[:, None], c0, c)
    cq = quant(c)
    px, py = x.astype(np.float32) + w_other * u, y.astype(np.float32) + w_other * v
    fx, fy = np.floor(px), np.floor(py)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    qx, qy = ((px - fx) * F32(64)).astype(np.int64), ((py - fy) * F32(64)).astype(np.int64)
    kept = 0
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = ix + dx, iy + dy
            W = (qx if dx else 64 - qx) * (qy if dy else 64 - qy) * int(a)
            keep = ok & (W > 0)
            if mutant == 'clamp':
                tx, ty = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
            else:
                keep &= (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)       # dropped, not clamped
            np.add.at(Sw, (ty[keep], tx[keep]), W[keep])
            np.add.at(Sc, (ty[keep], tx[keep]), W[keep, None] * cq[keep])
            kept += int(W[keep].sum())
    return kept


def interpolate_pair(im0, im1, fw, bw, occ_fw, occ_bw, h, w, n, mutant=None):
    """The n in-between frames of one pair: im0, im1 [Hmax, Wmax, 3] uint8 or fp32, fw (and bw, or None) [Hmax, Wmax, 2] fp32, occ_fw /
    occ_bw [Hmax, Wmax] uint8 (with bw), the frame (h, w) in their corner.  Returns (mid uint8 [n, h, w, 3], holes int64 [n], stats):
    stats per j = (Sw [h, w], the sum of the kept taps' weights)."""
    assert 1 <= n <= N_MAX and (bw is None) == (occ_fw is None) == (occ_bw is None)
    pitch = w if mutant == 'pitch_w' else fw.shape[1]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    q = (yy * pitch + xx).reshape(-1)
    q0, q1 = quant(_px(im0, q)).reshape(h, w, 3), quant(_px(im1, q)).reshape(h, w, 3)
    mid, holes, stats = np.zeros((n, h, w, 3), np.uint8), np.zeros(n, np.int64), []
    for j in range(1, n + 1):
        t, s = times(n, j)
        a_fw, a_bw = (j, n + 1 - j) if mutant == 'dir_swap' else (n + 1 - j, j)
        Sc, Sw = np.zeros((h, w, 3), np.int64), np.zeros((h, w), np.int64)
        kept = _pass(im0, im1, fw, occ_fw, h, w, pitch, s, t, a_fw, Sc, Sw, mutant)
        if bw is not None:
            kept += _pass(im1, im0, bw, occ_bw, h, w, pitch, t, s, a_bw, Sc, Sw, mutant)
        hole = Sw < (4 * HOLE if mutant == 'hole_x4' else HOLE)
        full = (Sc + Sw[..., None] * 128) // (np.maximum(Sw, 1)[..., None] * 256)
        blend = ((n + 1 - j) * q0 + j * q1 + (n + 1) * 128) // ((n + 1) * 256)
        out = np.where(hole[..., None], blend, full)
        assert out.min() >= 0 and out.max() <= 255
        mid[j - 1], holes[j - 1] = out, int(hole.sum())
        stats.append((Sw, kept))
    return mid, holes, stats


def replay(case, prev, mutant=None):
    """One launch on `case` (make_case) with prev [Hmax, Wmax, 3] in the staged dtype (None while the carry source is 0: never read):
    ({valid slot: (mid uint8 [n, h, w, 3], holes int64 [n])}, the prev the launch leaves, {slot: stats}).  Mutant prev_slot0: prev
    is taken from frame slot 0, not from the last new frame."""
    h, w, n, fr = case['h'], case['w'], case['n'], case['frames']
    outs, stats = {}, {}
    for i in case['valid']:
        assert i > 0 or case['carry'] > 0
        occ = (None, None) if case['occ'] is None else (case['occ'][0, i], case['occ'][1, i])
        mid, holes, st = interpolate_pair(prev if i == 0 else fr[i - 1], fr[i], case['flow_fw'][i],
                                          None if case['flow_bw'] is None else case['flow_bw'][i], occ[0], occ[1], h, w, n, mutant)
        outs[i], stats[i] = (mid, holes), st
    new_prev = np.zeros(fr.shape[1:], fr.dtype) if prev is None else prev.copy()
    new_prev[:h, :w] = fr[0 if mutant == 'prev_slot0' else case['k'] - 1, :h, :w]
    return outs, new_prev, stats


def compare(case, outs, out_mid, out_holes, sentinel, sentinel_holes):
    """The comparator of the GPU test: what one launch left in out_mid [n][Brows][Hmax][Wmax][3] and out_holes [n][Brows] (Brows >=
    B; filled with the sentinels before the launch) against the mirror's outs: equal at every pixel of every valid slot, the hole
    counts equal, and the sentinel everywhere else — slots that are no pairs, pixels outside (h, w), rows beyond B.  Returns the
    number of pixels compared."""
    h, w, n = case['h'], case['w'], case['n']
    assert sorted(outs) == list(case['valid'])
    rest = np.ones(out_mid.shape[:4], bool)
    seen = 0
    for i, (mid, holes) in outs.items():
        got = out_mid[:, i, :h, :w]
        bad = np.argwhere((got != mid).any(axis=-1))
        assert len(bad) == 0, ("slot %d: %d pixels differ, first (j - 1, y, x) %s: got %s, mirror %s"
                               % (i, len(bad), bad[0], got[tuple(bad[0])], mid[tuple(bad[0])]))
        assert np.array_equal(out_holes[:, i].astype(np.int64), holes), ("slot %d: holes" % i, out_holes[:, i], holes)
        rest[:, i, :h, :w] = False
        seen += n * h * w
    assert (out_mid[rest] == sentinel).all(), "pixels outside the valid pairs were written"
    keep = np.ones(out_holes.shape, bool)
    keep[:, list(outs)] = False
    assert (out_holes[keep] == sentinel_holes).all(), "hole counts of slots that are no pairs were written"
    return seen


# ------------------------------------------------------------------------------------------------- inputs
FLOW_KINDS = ('const', 'smooth', 'iid12', 'wild')
# replay patterns as (new frames k, carry source): a clip's first replay (slot 0 is no pair), a short first replay (one frame: no
# pair at all), a full carried replay (pair 0 reads prev), short carried replays (trailing slots are no pairs)
PATTERNS = {'first': (None, 0), 'nopairs': (1, 0), 'full': (None, None), 'short': (1, None), 'short2': (2, None)}
RAGGED = dict(B=3, Hmax=40, Wmax=64, h=37, w=53)        # the pitch is not the width; more than one block per pair (1961 pixels)
BIG = dict(B=1, Hmax=600, Wmax=900, h=600, w=900)       # one pair past GRID_CAP pixels


def draw_frames(rs, count, Hmax, Wmax, h, w, u8):
    """count + 1 frames [count + 1, Hmax, Wmax, 3] of one canvas seen through a window that moves by -STEP per frame, so that frame
    k + 1 is frame k translated by STEP (content at (x, y) moves to (x + 4, y - 2)); the first is the prev of a carried replay.
    Outside the (h, w) corner: a constant the kernel must never read into a result (255 / 1e3)."""
    n = count + 1
    pad_x, pad_y = abs(STEP[0]) * n, abs(STEP[1]) * n
    canvas = rs.randint(0, 256, size=(h + 2 * pad_y, w + 2 * pad_x, 3))
    if not u8:
        canvas = canvas + rs.rand(*canvas.shape) * 0.999 - 0.5          # fp32 frames are not integers
        canvas = np.clip(canvas, 0, 255)
    out = np.full((n, Hmax, Wmax, 3), 255 if u8 else 1e3, np.uint8 if u8 else np.float32)
    for k in range(n):
        oy, ox = pad_y - STEP[1] * k, pad_x - STEP[0] * k
        out[k, :h, :w] = canvas[oy:oy + h, ox:ox + w]
    return out


def draw_flows(rs, B, Hmax, Wmax, h, w, kind, sign=1.0):
    """[B, Hmax, Wmax, 2] fp32: a flow of `kind` in the (h, w) corner of every slot, NaN outside it (never to be read).  const: sign *
    STEP everywhere; smooth: track_ref's slow sine field of a few pixels; iid12: i.i.d. uniform +-12 px (collisions, many targets
    outside the frame); wild: smooth with NaN, inf, 1e7, +-1e6 (excluded) and 999999 (kept, lands far outside) planted."""
    if kind == 'const':
        f = np.full((B, Hmax, Wmax, 2), np.nan, np.float32)
        f[:, :h, :w] = np.asarray(STEP, np.float32) * F32(sign)
        return f
    if kind == 'iid12':
        f = np.full((B, Hmax, Wmax, 2), np.nan, np.float32)
        f[:, :h, :w] = (rs.rand(B, h, w, 2) * 24 - 12).astype(np.float32)
        return f
    f = T.draw_flows(rs, B, Hmax, Wmax, h, w, 'smooth')
    if kind == 'wild':
        bad = (np.nan, np.inf, -np.inf, 1e7, -1e7, 1e6, -1e6, 999999.0)
        for b in range(B):
            for m, val in enumerate(bad):
                f[b, (5 * m + b + 1) % h, (7 * m + 3 * b + 2) % w, (m + b) % 2] = val
            f[b, (b + 11) % h, (b + 13) % w] = (np.nan, np.inf)
    return f


def make_case(name, B, Hmax, Wmax, h, w, n, u8, bidir, kind, pattern, seed=0):
    """One launch: the tables of sequence_tables, B staged frames (and the prev of a carried replay), the flows and masks."""
    from unflow_amd.core.inference import sequence_tables
    rs = WP._rs('mid', name, n, u8, bidir, kind, pattern, seed)
    k, carry = PATTERNS[pattern]
    k = B if k is None else k
    carry = B if carry is None else carry
    tab, valid, _ = sequence_tables((h, w), k, B, carry, u8=u8)
    fr = draw_frames(rs, B, Hmax, Wmax, h, w, u8)
    return dict(name=name, B=B, Hmax=Hmax, Wmax=Wmax, h=h, w=w, n=n, u8=u8, bidir=bidir, kind=kind, pattern=pattern, k=k, carry=carry,
                tab=tab, valid=valid, prev=fr[0].copy(), frames=np.ascontiguousarray(fr[1:]),
                flow_fw=draw_flows(rs, B, Hmax, Wmax, h, w, kind),
                flow_bw=draw_flows(rs, B, Hmax, Wmax, h, w, kind, sign=-1.0) if bidir else None,
                occ=np.stack([T.draw_occ(rs, B, Hmax, Wmax, h, w) for _ in range(2)]) if bidir else None,
                id='%s-n%d-%s-%s-%s-%s' % (name, n, 'u8' if u8 else 'f32', 'bidir' if bidir else 'fw', kind, pattern))


def prev_of(case):
    """The prev a launch on `case` is given: the frame before its first one when it carries, None (never read) when it does not."""
    return case['prev'] if case['carry'] > 0 else None


@functools.lru_cache(maxsize=None)
def entry_cases():
    """The launches of the entry-point tests: (id, case) — every flow kind in one and in both directions, with n in {1, 3} and uint8
    and fp32 frames crossed over them, on the ragged shape; every replay pattern; and one pair past the grid's cap."""
    out = []
    for a, kind in enumerate(FLOW_KINDS):
        for b, bidir in enumerate((False, True)):
            for c, n in enumerate((1, 3)):
                out.append(make_case('ragged', n=n, u8=(a + b + c) % 2 == 0, bidir=bidir, kind=kind, pattern='full', **RAGGED))
    for m, pattern in enumerate(('first', 'nopairs', 'short', 'short2')):
        for bidir in (False, True):
            out.append(make_case('ragged', n=3 if bidir else 1, u8=(m % 2 == 0) != bidir, bidir=bidir, kind='smooth',
                                 pattern=pattern, **RAGGED))
    out.append(make_case('past-the-cap', n=1, u8=True, bidir=False, kind='smooth', pattern='full', **BIG))
    return [(c['id'], c) for c in out]


@functools.lru_cache(maxsize=None)
def mirror_of(cid):
    """replay of entry case `cid` from its own prev, computed once and shared: (outs, new prev, stats).  Read-only."""
    case = dict(entry_cases())[cid]
    return replay(case, prev_of(case))
