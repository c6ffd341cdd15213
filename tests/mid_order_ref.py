"""The definition of unflow_sequence_interpolate_ordered (include/unflow_hip.h) in numpy, on top of tests/mid_ref.py:
its cases, the occluder scene with its rendered truth, and the comparator of tests/test_interpolate_order_gpu.py, proven without a
GPU by tests/test_interpolate_order_cpu.py.  Not a test file.

As in mid_ref every fp32 step is one numpy operation per rounding (np.fmin where the kernel has fminf, np.fmax / np.fmin in the
quantisation, so that a NaN colour ends where the kernel puts it), and from the quantisation on everything is int64: the comparison
with the kernel is equality.  The hole test reads the weight word as the kernel packs it (Sw below bit 46, the conf-less weight mod
2^18 above) and is asserted to be the conf-less sum's test on every case.  order = 0 is mid_ref.interpolate_pair, which
tests/test_interpolate_order_cpu.py shows case by case.

Mutants (MUTANTS) are deliberate mistakes of the mirror; the CPU test shows that each changes the result of at least one case."""
import functools

import numpy as np

import mid_ref as M
import track_ref as T

F32 = np.float32
ORDER_MAX = 4
FLOOR = 6                        # d at which conf is 1 and the pixel keeps its own colour
E_CAP = F32(765)
PIXELS_MAX = 1 << 23             # order >= 1: Hmax * Wmax above this is refused
SW_BITS = 46                     # the weight word: Sw in bits [0, 46), the conf-less weight sum mod 2^18 above
ORDERS = (1, 2, 4)
MUTANTS = ('sw_no_conf',         # conf left out of the weight sum
           'shift_k',            # e >> k in place of e >> (6 - k)
           'mask_conf64',        # a masked pixel at conf 64
           'floor_blend',        # a floor pixel still blended
           'hole_blend',         # a one-direction hole gets the temporal blend
           'e_max',              # the largest channel difference in place of their sum
           'no_cap',             # d not capped at 6
           'hole_sw')            # the hole test on the conf-weighted sum: holes that a confident sliver closes
compare = M.compare              # the comparator with sentinels: one definition for both entries


def quant(c):
    """mid_ref.quant with the kernel's fmaxf / fminf: a NaN colour is 0."""
    assert c.dtype == np.float32
    return np.rint(np.fmin(np.fmax(c, F32(0)), F32(255)) * F32(256)).astype(np.int64)


def _pass(here, other, flow, occ, h, w, pitch, w_here, w_other, a, Sc, Sw, Sw0, order, mutant=None, tally=None):
    """One splat pass of the ordered definition (mid_ref._pass with conf) into Sc, Sw and the conf-less weight sum Sw0: returns the
    sum of the kept taps' weights.  tally: a dict that collects, over the pixels whose flow is kept, the histogram of d ('d', masked
    pixels apart as 'masked') and the number of blended and unblended pixels."""
    assert flow.dtype == np.float32 and w_here.dtype == np.float32 and w_other.dtype == np.float32
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    x, y = xx.reshape(-1).astype(np.int64), yy.reshape(-1).astype(np.int64)
    q = y * pitch + x
    f = flow.reshape(-1, 2)[q]
    with np.errstate(invalid='ignore'):
        ok = (np.abs(f[:, 0]) < M.LIMIT) & (np.abs(f[:, 1]) < M.LIMIT)
    u, v = np.where(ok, f[:, 0], F32(0)), np.where(ok, f[:, 1], F32(0))
    idx, _, _, wts = T._taps(u, v, x, y, h, w, pitch, np.float32)
    wa, wb, wc, wd = (t[:, None] for t in wts)
    ta, tb, tc, td = (M._px(other, i) for i in idx)
    with np.errstate(invalid='ignore'):
        wp = ((wa * ta + wb * tb) + wc * tc) + wd * td
        c0 = M._px(here, q)
        blended = w_here * c0 + w_other * wp
        assert blended.dtype == np.float32
        masked = np.zeros(len(q), bool) if occ is None else occ.reshape(-1)[q] != 0
        if order == 0:
            conf, floor = np.ones(len(q), np.int64), np.zeros(len(q), bool)
            d = np.zeros(len(q), np.int64)
        else:
            dr, dg, db = (np.abs(c0[:, k] - wp[:, k]) for k in range(3))
            e = np.fmin(np.maximum(np.maximum(dr, dg), db) if mutant == 'e_max' else (dr + dg) + db, E_CAP)       # a NaN gives 765
            assert e.dtype == np.float32 and not np.isnan(e).any()
            d = e.astype(np.int64) >> (order if mutant == 'shift_k' else 6 - order)
            if mutant != 'no_cap':
                d = np.minimum(d, FLOOR)
            conf = 64 >> np.minimum(d, 63)
            floor = d == FLOOR
            conf = np.where(masked, 64 if mutant == 'mask_conf64' else 1, conf)
    own = masked | (floor & (mutant != 'floor_blend'))
    cq = quant(np.where(own[:, None], c0, blended))
    if tally is not None:
        tally['masked'] = tally.get('masked', 0) + int((ok & masked).sum())
        tally['d'] = tally.get('d', 0) + np.bincount(np.minimum(d[ok & ~masked], FLOOR), minlength=FLOOR + 1)
        tally['blended'] = tally.get('blended', 0) + int((ok & ~own).sum())
        tally['unblended'] = tally.get('unblended', 0) + int((ok & own).sum())
    px, py = x.astype(np.float32) + w_other * u, y.astype(np.float32) + w_other * v
    fx, fy = np.floor(px), np.floor(py)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    qx, qy = ((px - fx) * F32(64)).astype(np.int64), ((py - fy) * F32(64)).astype(np.int64)
    kept = 0
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = ix + dx, iy + dy
            wx, wy = (qx if dx else 64 - qx), (qy if dy else 64 - qy)
            W0 = wx * wy * int(a)
            W = W0 * conf
            keep = ok & (wx > 0) & (wy > 0) & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)           # dropped, not clamped
            Wsum = W0 if mutant == 'sw_no_conf' else W
            np.add.at(Sw, (ty[keep], tx[keep]), Wsum[keep])
            np.add.at(Sw0, (ty[keep], tx[keep]), W0[keep])
            np.add.at(Sc, (ty[keep], tx[keep]), W[keep, None] * cq[keep])
            kept += int(Wsum[keep].sum())
    return kept


def interpolate_pair(im0, im1, fw, bw, occ_fw, occ_bw, h, w, n, order, mutant=None, tally=None):
    """mid_ref.interpolate_pair at `order`: (mid uint8 [n, h, w, 3], holes int64 [n], stats), stats per j = (Sw, kept weights, the
    hole mask)."""
    assert 1 <= n <= M.N_MAX and 0 <= order <= ORDER_MAX and (bw is None) == (occ_fw is None) == (occ_bw is None)
    assert fw.shape[0] * fw.shape[1] <= PIXELS_MAX or order == 0
    pitch = fw.shape[1]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    q = (yy * pitch + xx).reshape(-1)
    q0, q1 = quant(M._px(im0, q)).reshape(h, w, 3), quant(M._px(im1, q)).reshape(h, w, 3)
    mid, holes, stats = np.zeros((n, h, w, 3), np.uint8), np.zeros(n, np.int64), []
    for j in range(1, n + 1):
        t, s = M.times(n, j)
        Sc, Sw, Sw0 = np.zeros((h, w, 3), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
        kept = _pass(im0, im1, fw, occ_fw, h, w, pitch, s, t, n + 1 - j, Sc, Sw, Sw0, order, mutant, tally)
        if bw is not None:
            kept += _pass(im1, im0, bw, occ_bw, h, w, pitch, t, s, j, Sc, Sw, Sw0, order, mutant, tally)
        assert Sw.min() >= 0 and Sc.min() >= 0 and Sc.max() < 2 ** 62 and Sw.max() < 1 << SW_BITS
        # a hole: the CONF-LESS weight below the threshold, as read out of the weight word, which keeps Sw in its low 46 bits and
        # Sw0 mod 2^18 above them (mutant hole_sw tests the weighted sum, which a confident sliver lifts over the threshold)
        top = Sw0 & ((1 << 64 - SW_BITS) - 1)
        hole = (Sw < M.HOLE) | ((Sw < 64 * M.HOLE) & (top < M.HOLE))
        if mutant is None:
            assert np.array_equal(hole, Sw0 < M.HOLE)              # Sw0 <= Sw <= 64 Sw0: the word decides exactly
        if mutant == 'hole_sw':
            hole = Sw < M.HOLE
        full = (Sc + Sw[..., None] * 128) // (np.maximum(Sw, 1)[..., None] * 256)
        if order >= 1 and bw is None and mutant != 'hole_blend':
            fill = (q1 + 128) // 256                               # one direction: the later frame
        else:
            fill = ((n + 1 - j) * q0 + j * q1 + (n + 1) * 128) // ((n + 1) * 256)
        out = np.where(hole[..., None], fill, full)
        assert mutant is not None or (out.min() >= 0 and out.max() <= 255)
        out = out & 255                                            # a mutant's quotient may not fit the byte the kernel would write
        mid[j - 1], holes[j - 1] = out, int(hole.sum())
        stats.append((Sw, kept, hole))
    return mid, holes, stats


def replay(case, prev, order=None, mutant=None, tally=None):
    """mid_ref.replay at the case's order (or `order`): ({valid slot: (mid, holes)}, the prev the launch leaves, {slot: stats})."""
    h, w, n, fr = case['h'], case['w'], case['n'], case['frames']
    order = case['order'] if order is None else order
    outs, stats = {}, {}
    for i in case['valid']:
        assert i > 0 or case['carry'] > 0
        occ = (None, None) if case['occ'] is None else (case['occ'][0, i], case['occ'][1, i])
        mid, holes, st = interpolate_pair(prev if i == 0 else fr[i - 1], fr[i], case['flow_fw'][i],
                                          None if case['flow_bw'] is None else case['flow_bw'][i], occ[0], occ[1], h, w, n, order,
                                          mutant, tally)
        outs[i], stats[i] = (mid, holes), st
    new_prev = np.zeros(fr.shape[1:], fr.dtype) if prev is None else prev.copy()
    new_prev[:h, :w] = fr[case['k'] - 1, :h, :w]
    return outs, new_prev, stats


# ------------------------------------------------------------------------------------------------- the occluder scene
SCENE = dict(Hmax=40, Wmax=64, h=37, w=53, side=16, x0=14, y0=10, move=8)


def _render(bg, sq, x):
    s = SCENE
    im = bg.copy()
    im[s['y0']:s['y0'] + s['side'], x:x + s['side']] = sq
    return im


@functools.lru_cache(maxsize=None)
def scene(n, bidir):
    """A 16 x 16 square of colours in [192, 256) that moves 8 px in +x over a static background of colours in [0, 64), with the
    exact flows and (both directions) the exact occlusion masks, as one carried launch with one pair: (case without an order, truth
    uint8 [n, h, w, 3]), truth frame j with the square at x0 + 8 j / (n + 1)."""
    from unflow_amd.core.inference import sequence_tables
    s = SCENE
    Hm, Wm, h, w, side, x0, y0, move = (s[k] for k in ('Hmax', 'Wmax', 'h', 'w', 'side', 'x0', 'y0', 'move'))
    rs = np.random.RandomState(0)
    bg = rs.randint(0, 64, (h, w, 3)).astype(np.uint8)
    sq = rs.randint(192, 256, (side, side, 3)).astype(np.uint8)
    assert move % (n + 1) == 0
    fr = np.full((2, Hm, Wm, 3), 255, np.uint8)
    fr[0, :h, :w], fr[1, :h, :w] = _render(bg, sq, x0), _render(bg, sq, x0 + move)
    truth = np.stack([_render(bg, sq, x0 + move * j // (n + 1)) for j in range(1, n + 1)])
    rows = slice(y0, y0 + side)
    fw = np.full((1, Hm, Wm, 2), np.nan, np.float32)
    bw = fw.copy()
    fw[0, :h, :w], bw[0, :h, :w] = 0, 0
    fw[0, rows, x0:x0 + side] = (move, 0)
    bw[0, rows, x0 + move:x0 + move + side] = (-move, 0)
    occ = np.ones((2, 1, Hm, Wm), np.uint8)
    occ[:, 0, :h, :w] = 0
    occ[0, 0, rows, x0 + side:x0 + side + move] = 1          # background of frame 0 that the square covers in frame 1
    occ[1, 0, rows, x0:x0 + move] = 1                        # background of frame 1 that the square covered in frame 0
    tab, valid, _ = sequence_tables((h, w), 1, 1, 1, u8=True)
    case = dict(name='occluder', B=1, Hmax=Hm, Wmax=Wm, h=h, w=w, n=n, u8=True, bidir=bidir, kind='exact', pattern='carried', k=1,
                carry=1, tab=tab, valid=valid, prev=fr[0].copy(), frames=np.ascontiguousarray(fr[1:]), flow_fw=fw,
                flow_bw=bw if bidir else None, occ=occ if bidir else None,
                id='occluder-n%d-u8-%s-exact-carried' % (n, 'bidir' if bidir else 'fw'))
    return case, truth


def scene_scores(n, bidir, order):
    """(SSE against the rendered truth summed over the n frames, the largest per-channel error, the hole counts) of the scene."""
    case, truth = scene(n, bidir)
    mid, holes = replay(case, case['prev'], order)[0][0]
    err = mid[:, :case['h'], :case['w']].astype(np.int64) - truth
    return int((err * err).sum()), int(np.abs(err).max()), holes.tolist()


# ------------------------------------------------------------------------------------------------- cases
def _ordered(case, order):
    return dict(case, order=order, id='%s-k%d' % (case['id'], order))


def plant_nans(case):
    """fp32 frames with NaN colours planted: whole pixels and single channels, in prev and in every staged frame, inside (h, w)."""
    assert not case['u8']
    fr, prev = case['frames'].copy(), case['prev'].copy()
    h, w = case['h'], case['w']
    for b in range(fr.shape[0]):
        for m in range(6):
            fr[b, (7 * m + b + 3) % h, (11 * m + 5 * b + 1) % w, slice(None) if m % 2 else m % 3] = np.nan
    for m in range(6):
        prev[(5 * m + 2) % h, (13 * m + 4) % w, slice(None) if m % 2 else m % 3] = np.nan
    return dict(case, frames=fr, prev=prev, name='nan', id='nan-' + case['id'])


@functools.lru_cache(maxsize=None)
def entry_cases():
    """The launches of the entry-point tests, (id, case) with case['order']: mid_ref's ragged cases — the four flow kinds in one and
    in both directions, n in {1, 3}, uint8 and fp32 — at every order of ORDERS; its replay patterns, the orders taking turns; the
    occluder scene; one pair past the grid's cap; and fp32 frames with NaN colours planted."""
    out, turn = [], 0
    for cid, case in M.entry_cases():
        if case['name'] != 'ragged':
            out.append(_ordered(case, 1))                       # past the cap
        elif case['pattern'] == 'full':
            out += [_ordered(case, k) for k in ORDERS]
        else:
            out.append(_ordered(case, ORDERS[turn % len(ORDERS)]))
            turn += 1
    for n in (1, 3):
        for bidir in (False, True):
            out.append(_ordered(scene(n, bidir)[0], 2))
    for bidir, kind, k in ((False, 'smooth', 1), (True, 'smooth', 2), (True, 'const', 4)):
        base = M.make_case('ragged', n=3 if bidir else 1, u8=False, bidir=bidir, kind=kind, pattern='full', **M.RAGGED)
        out.append(_ordered(plant_nans(base), k))
    assert len({c['id'] for c in out}) == len(out)
    return [(c['id'], c) for c in out]


@functools.lru_cache(maxsize=None)
def mirror_of(cid):
    """replay of entry case `cid` from its own prev, computed once and shared: (outs, new prev, stats).  Read-only."""
    case = dict(entry_cases())[cid]
    return replay(case, M.prev_of(case))
