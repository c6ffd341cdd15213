"""The definition of unflow_sequence_track (include/unflow_hip.h) in numpy, its cases, synthetic inputs and the
comparator of tests/test_track_gpu.py, proven without a GPU by tests/test_track_cpu.py.  Not a test file.

One step function, used two ways — the split of tests/warp_parity.py: the taps and every flag are integer decisions on fp32 values
(floorf of the fp32 displacement chooses the taps; a weight is zero or not; the new fp32 displacement is inside the frame or not),
part of the definition; everything after the tap choice — weights, products, sums — is carried in `dt`:

    float64   the mirror;
    float32   every operation rounded on its own, the yardstick of what fp32 arithmetic delivers on the same inputs.

The standing bound is warp_parity.bound_of: max(1e-6, 2 x the yardstick's own distance from the mirror), of the tensor's max."""
import functools

import numpy as np
import torch

import warp_parity as WP

LIMIT = np.float32(1e6)          # a displacement component of this magnitude (or not finite) ends a track
GRID_CAP = 2048 * 256            # the threads of the kernel's capped grid: more tracks take its grid-stride loop
MUTANTS = ('anchor_sample', 'pitch_w', 'occ_after', 'dead_move', 'bound_w', 'reinit')


def grid_anchors(h, w, S):
    """The dense anchors of stride S over (h, w), row-major: int64 [gh * gw, 2] of (x, y)."""
    gy, gx = np.meshgrid(np.arange(0, h, S), np.arange(0, w, S), indexing='ij')
    return np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1).astype(np.int64)


def _taps(u, v, x, y, h, w, pitch, dt):
    """image_warp's taps (csrc/image_warp.h) of (x, y) displaced by fp32 (u, v): flat indices ia..id with rows `pitch` apart,
    the fractions and the four weights in dt."""
    assert u.dtype == np.float32 and v.dtype == np.float32
    fu, fv = np.floor(u), np.floor(v)
    xw, yw = u.astype(dt) - fu.astype(dt), v.astype(dt) - fv.astype(dt)
    one = dt(1)
    wa, wb, wc, wd = (one - xw) * (one - yw), (one - xw) * yw, xw * (one - yw), xw * yw
    xi, yi = x + fu.astype(np.int64), y + fv.astype(np.int64)
    x0, x1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    y0, y1 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    return (y0 * pitch + x0, y1 * pitch + x0, y0 * pitch + x1, y1 * pitch + x1), xw, yw, (wa, wb, wc, wd)


def _occluded(occ, idx, xw, yw):
    o = [occ.reshape(-1)[i] != 0 for i in idx]
    return o[0] | ((yw > 0) & o[1]) | ((xw > 0) & o[2]) | ((xw > 0) & (yw > 0) & o[3])


def in_frame(disp32, anchors, h, w, bound_w=False):
    """The in-frame flag of fp32 displacements: finite and below LIMIT first, then 0 <= xi and (xi < w - 1 or (xi == w - 1 and
    xw == 0)), likewise in y.  Mutant bound_w: w and h in place of w - 1 and h - 1."""
    assert disp32.dtype == np.float32
    with np.errstate(invalid='ignore'):
        fin = (np.abs(disp32) < LIMIT).all(axis=1)           # NaN and inf compare false
    d = np.where(fin[:, None], disp32, np.float32(0))
    f = np.floor(d)
    frac = d - f
    ok = fin
    for k, size in ((0, w), (1, h)):
        p = anchors[:, k] + f[:, k].astype(np.int64)
        last = size if bound_w else size - 1
        ok = ok & (p >= 0) & ((p < last) | ((p == last) & (frac[:, k] == 0)))
    return ok


def step(disp, alive, anchors, flow, occ, h, w, dt, mutant=None, frame_disp=None):
    """One step of the definition for one pair slot.  disp [N, 2] fp32 and alive [N] bool: the tracks before; anchors int64 [N, 2];
    flow [Hmax, Wmax, 2] fp32 and occ [Hmax, Wmax] uint8 or None: the slot's maps, the frame (h, w) in their corner.  Returns
    (disp in dt, alive).  frame_disp: the fp32 displacements the in-frame flag is decided on instead of this function's own
    rounded to fp32 — the comparator passes the kernel's, the fp32 input both sides share.
    Mutants: anchor_sample — the flow is sampled at the anchor, not at the current position; pitch_w — rows w apart, not Wmax;
    occ_after — occlusion tested after the step, at the new position; dead_move — dead tracks keep moving; bound_w — in_frame's."""
    assert disp.dtype == np.float32 and alive.dtype == bool
    dt = np.dtype(dt).type
    x, y = anchors[:, 0], anchors[:, 1]
    live = alive & (x >= 0) & (x < w) & (y >= 0) & (y < h)
    moving = live | ((x >= 0) & (x < w) & (y >= 0) & (y < h)) if mutant == 'dead_move' else live
    with np.errstate(invalid='ignore'):
        sane = np.isfinite(disp).all(axis=1) & (np.abs(disp) < LIMIT).all(axis=1)
    cur = np.where((moving & sane)[:, None], disp, np.float32(0))       # (a dead track's displacement may be anything)
    at = np.zeros_like(cur) if mutant == 'anchor_sample' else cur
    pitch = w if mutant == 'pitch_w' else flow.shape[1]
    idx, xw, yw, wts = _taps(at[:, 0], at[:, 1], x, y, h, w, pitch, dt)
    if occ is not None and mutant != 'occ_after':
        live = live & ~_occluded(occ, idx, xw, yw)
    fl = flow.reshape(-1, 2)
    with np.errstate(invalid='ignore', over='ignore'):
        a, b, c, d = (fl[i].astype(dt) for i in idx)
        wa, wb, wc, wd = (t[:, None] for t in wts)
        val = ((wa * a + wb * b) + wc * c) + wd * d
        adv = live | moving if mutant == 'dead_move' else live
        new = np.where(adv[:, None], disp.astype(dt) + val, disp.astype(dt))
        new32 = new.astype(np.float32)
    if occ is not None and mutant == 'occ_after':
        safe = np.where(in_frame(new32, anchors, h, w)[:, None], new32, np.float32(0))
        idx2, xw2, yw2, _ = _taps(safe[:, 0], safe[:, 1], x, y, h, w, pitch, dt)
        live = live & ~_occluded(occ, idx2, xw2, yw2)
    decide = new32 if frame_disp is None else np.where(live[:, None], frame_disp, new32)
    live = live & in_frame(decide, anchors, h, w, bound_w=(mutant == 'bound_w'))
    return new, live


def replay(case, state, dt=np.float32, mutant=None):
    """One launch on `case` (make_case) from state (disp [N, 2] fp32, alive [N] bool), chained in dt with fp32 outputs, as the
    kernel stores them: ({slot: (disp fp32, alive)} of the valid slots, the new state).  Mutant reinit: the state is
    re-initialised on every launch, whatever the carry source."""
    N = case['N']
    if case['carry'] == 0 or mutant == 'reinit':
        disp, alive = np.zeros((N, 2), np.float32), np.ones(N, bool)
    else:
        disp, alive = state[0].copy(), state[1].copy()
    outs = {}
    for i in case['valid']:
        new, alive = step(disp, alive, case['anchors'], case['flow'][i], None if case['occ'] is None else case['occ'][i],
                          case['h'], case['w'], dt, mutant)
        disp = new.astype(np.float32)
        outs[i] = (disp, alive)
    return outs, (disp, alive)


def compare_disp(got, yard, mirror):
    """disp of one slot against the mirror, the bound from the yardstick: non-finite values where the mirror has them (NaN for
    NaN, the same infinity); the rest within bound_of(yardstick, mirror) of the tensor's max, where the tensor is the elements
    below LIMIT — the few elements thrown past it are held to the same ratio of their own magnitude, so that one 1e6 does not
    widen every other track's bound.  Returns the worst ratio over bound."""
    assert got.dtype == np.float32 and got.shape == mirror.shape, (got.dtype, got.shape, mirror.shape)
    fin = np.isfinite(mirror)
    for a in (got, yard):
        assert np.array_equal(np.isfinite(a), fin) and np.array_equal(np.isnan(a), np.isnan(mirror)), "non-finite elements differ"
        assert np.array_equal(a[~fin & ~np.isnan(mirror)], mirror[~fin & ~np.isnan(mirror)]), "infinities differ"
    far = fin & (np.abs(mirror) >= LIMIT)
    near = fin & ~far
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[near], dtype=np.float64))      # noqa: E731
    bound, _ = WP.bound_of(t(yard), t(mirror))
    worst = WP.check(t(got), t(mirror), bound) / bound if near.any() else 0.0
    if far.any():
        r = float((np.abs(got[far].astype(np.float64) - mirror[far]) / np.abs(mirror[far])).max())
        assert r <= bound, ("thrown tracks", r, bound)
        worst = max(worst, r / bound)
    return worst


def check_replay(case, state, outs, new_state):
    """The comparator of the GPU test: what one launch wrote — outs {slot: (disp fp32 [N, 2], alive bool [N])} and the new state —
    against the definition, step by step.  Slot i is compared with the mirror seeded from the launch's OWN output of the valid
    slot before it; for the first valid slot the seed is the state (carry source above 0) or disp = 0, alive = 1 (carry source 0).
    alive bit for bit; disp by compare_disp; a track dead in the seed keeps its disp bit for bit; the new state is the last valid
    slot's output (the seed when there is none) bit for bit.  Returns the worst ratio over bound."""
    N = case['N']
    assert sorted(outs) == list(case['valid']), (sorted(outs), case['valid'])
    if case['carry'] == 0:
        seed = (np.zeros((N, 2), np.float32), np.ones(N, bool))
    else:
        seed = (state[0], state[1])
    worst = 0.0
    for i in case['valid']:
        got_d, got_a = outs[i]
        assert got_d.dtype == np.float32 and got_d.shape == (N, 2) and got_a.dtype == bool and got_a.shape == (N,)
        args = (seed[0], seed[1], case['anchors'], case['flow'][i], None if case['occ'] is None else case['occ'][i],
                case['h'], case['w'])
        mir_d, mir_a = step(*args, np.float64, frame_disp=got_d)
        yar_d, yar_a = step(*args, np.float32, frame_disp=got_d)
        assert np.array_equal(mir_a, yar_a)                 # the flags are integer decisions: the two precisions agree
        bad = int((got_a != mir_a).sum())
        assert bad == 0, ("slot %d: alive differs" % i, bad, np.flatnonzero(got_a != mir_a)[:8])
        dead = ~seed[1]
        assert np.array_equal(got_d[dead].view(np.int32), seed[0][dead].view(np.int32)), "slot %d: a dead track moved" % i
        worst = max(worst, compare_disp(got_d, yar_d.astype(np.float32), mir_d))
        seed = (got_d, got_a)
    assert np.array_equal(new_state[0].view(np.int32), seed[0].view(np.int32)) and np.array_equal(new_state[1], seed[1]), "state"
    return worst


# ------------------------------------------------------------------------------------------------- inputs
FLOW_KINDS = ('smooth', 'torn', 'far', 'zero', 'const', 'tiny')
CONST_FLOW = (2.0, -1.0)
# replay patterns as (new frames k, carry source): sequence_tables' valid slots — a clip's first replay (slot 0 is no pair), a
# full later replay, a short later replay (trailing slots are no pairs), a short first replay (one frame: no pair at all)
PATTERNS = {'first': (None, 0), 'full': (None, None), 'short': (1, None), 'nopairs': (1, 0)}


def draw_flows(rs, B, Hmax, Wmax, h, w, kind):
    """[B, Hmax, Wmax, 2] fp32: a flow of `kind` in the (h, w) corner of every slot, NaN outside it (never to be read).
    smooth: a slow sine field of a few pixels; torn, far, tiny: warp_parity.draw_flow's sets — far with a 1e6 and a NaN planted;
    zero; const: CONST_FLOW everywhere."""
    f = np.full((B, Hmax, Wmax, 2), np.nan, np.float32)
    if kind == 'smooth':
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        ph = rs.rand(B, 4) * 6.28
        u = np.stack([2.3 * np.sin(xx / 9.0 + p[0]) + 1.1 * np.cos(yy / 7.0 + p[1]) for p in ph])
        v = np.stack([1.7 * np.sin(yy / 8.0 + p[2]) - 0.9 * np.cos(xx / 11.0 + p[3]) for p in ph])
        core = np.stack([u, v], axis=-1)
    elif kind == 'zero':
        core = np.zeros((B, h, w, 2))
    elif kind == 'const':
        core = np.broadcast_to(np.asarray(CONST_FLOW), (B, h, w, 2))
    else:
        core = WP.draw_flow(rs, B, h, w, {'far': 'far', 'torn': 'torn', 'tiny': 'tiny'}[kind])
    f[:, :h, :w] = core
    if kind == 'far':
        for b in range(B):
            f[b, (b + 1) % h, (2 * b + 3) % w] = (1e6, 0.25)
            f[b, (b + 2) % h, (3 * b + 1) % w, b % 2] = np.nan
            f[b, (b + 3) % h, (b + 5) % w] = (-3e6, np.inf)
    return f


def draw_occ(rs, B, Hmax, Wmax, h, w):
    """[B, Hmax, Wmax] uint8: a blob mask per slot — two discs — in the (h, w) corner, 1 outside it (never to be read)."""
    o = np.ones((B, Hmax, Wmax), np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    for b in range(B):
        m = np.zeros((h, w), bool)
        for _ in range(2):
            cy, cx, r = rs.rand() * h, rs.rand() * w, 1.0 + rs.rand() * min(h, w) / 5.0
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        o[b, :h, :w] = m
    return o


def make_case(name, B, Hmax, Wmax, h, w, anchors, kind, occ, pattern, Ncap=None, seed=0):
    """One launch: anchors an int S (the dense grid) or an int array [N, 2]."""
    from unflow_amd.core.inference import sequence_tables, track_grid
    rs = WP._rs('track', name, kind, occ, pattern, seed)
    if isinstance(anchors, int):
        S, pts = anchors, grid_anchors(h, w, anchors)
        assert len(pts) == int(np.prod(track_grid((h, w), S)))
    else:
        S, pts = 0, np.asarray(anchors, dtype=np.int64)
    N = len(pts)
    k, carry = PATTERNS[pattern]
    k = B if k is None else k
    carry = B if carry is None else carry
    tab, valid, _ = sequence_tables((h, w), k, B, carry, track=(S, N))
    return dict(name=name, B=B, Hmax=Hmax, Wmax=Wmax, h=h, w=w, S=S, N=N, Ncap=N + 3 if Ncap is None else Ncap, anchors=pts,
                sparse=S == 0, kind=kind, carry=carry, valid=valid, tab=tab, flow=draw_flows(rs, B, Hmax, Wmax, h, w, kind),
                occ=draw_occ(rs, B, Hmax, Wmax, h, w) if occ else None, pattern=pattern,
                id='%s-%s-%s-%s' % (name, kind, 'occ' if occ else 'noocc', pattern))


def draw_state(case):
    """A state in mid-clip for a launch with a carry source above 0: most tracks alive at a few pixels' displacement inside the
    frame, a fifth dead with what they had."""
    rs, N = WP._rs('track-state', case['id']), case['N']
    disp = (rs.randn(N, 2) * 2.0).astype(np.float32)
    alive = in_frame(disp, case['anchors'], case['h'], case['w']) & (rs.rand(N) > 0.2)
    return disp, alive


def sparse_points(rs, n, h, w, outside=True):
    """n anchors inside (h, w); with outside (and n > 1) one of them is moved out of the frame."""
    p = np.stack([rs.randint(0, w, size=n), rs.randint(0, h, size=n)], axis=1).astype(np.int64)
    if outside and n > 1:
        p[n // 2] = (w, h // 2)
    return p


SMALL = dict(B=3, Hmax=9, Wmax=11, h=7, w=10)          # the pitch is not the width
RAGGED = dict(B=4, Hmax=40, Wmax=56, h=37, w=53)       # ragged grids for S = 2, 3; more than one block at S = 1 (1961 tracks)


@functools.lru_cache(maxsize=None)
def entry_cases():
    """The launches of the entry-point tests: (id, case) — every flow kind with a blob mask and with occ_fw = NULL on the two
    dense S = 1 shapes, the ragged grids, the sparse tables, every replay pattern, and one launch past the grid's cap."""
    out = []
    for kind in FLOW_KINDS:
        for occ in (True, False):
            out.append(make_case('small', anchors=1, kind=kind, occ=occ, pattern='full', **SMALL))
            out.append(make_case('ragged-S1', anchors=1, kind=kind, occ=occ, pattern='first', **RAGGED))
    for S in (2, 3):
        for kind, occ in (('smooth', True), ('far', False)):
            out.append(make_case('ragged-S%d' % S, anchors=S, kind=kind, occ=occ, pattern='full', **RAGGED))
    rs = WP._rs('track-points')
    for n in (1, 65):
        pts = sparse_points(rs, n, RAGGED['h'], RAGGED['w'])
        for kind, occ, pattern in (('smooth', True, 'full'), ('far', False, 'first')):
            out.append(make_case('sparse-%d' % n, anchors=pts, kind=kind, occ=occ, pattern=pattern, **RAGGED))
    for pattern in ('short', 'nopairs', 'first'):
        out.append(make_case('small', anchors=1, kind='smooth', occ=True, pattern=pattern, **SMALL))
        out.append(make_case('ragged-S2', anchors=2, kind='smooth', occ=False, pattern=pattern, **RAGGED))
    big = sparse_points(rs, GRID_CAP + 77, RAGGED['h'], RAGGED['w'])
    out.append(make_case('past-the-cap', anchors=big, kind='smooth', occ=True, pattern='full', **dict(RAGGED, B=2)))
    return [(c['id'], c) for c in out]
