"""The definition of unflow_sequence_stabilise (include/unflow_hip.h) in numpy: its cases and the comparator of
tests/test_stabilise_gpu.py, proven without a GPU by tests/test_stabilise_cpu.py.  Not a test file.

Everything is int64 (Python integers where a sum is formed) except the solve, which is a sequence of scalar fp64 operations in the
header's order — Python floats: every +, -, *, / is one IEEE operation rounded on its own, an int -> float conversion is correctly
rounded — so the comparison with the kernel is equality on every output.

Mutants (MUTANTS) are deliberate mistakes of the mirror; the CPU test shows that each changes the result of at least one case."""
import functools

import numpy as np

import mid_ref as M
import track_ref as T
import warp_parity as WP

F32 = np.float32
LIMIT = F32(4096)                # a flow component of this magnitude (or not finite) makes the pixel invalid
ONE = 1 << 24                    # 1 in the linear part of a path
IDENTITY = (0, ONE, 0, 0, 0, ONE)
T_MAX, L_MAX, DT_MAX, DL_MAX = 1 << 28, 1 << 23, 1 << 30, 1 << 26
N_MIN = 16                       # fewer weighted pixels: degenerate
SIZE_MAX = 4096
TOLS, ITERS, FOLLOWS = (0, 2, 4), (0, 1, 3), (0, 3)
MUTANTS = ('centre_half',        # the centre off by a half pixel: X = 2 x - w + 2
           'floor_one',          # weight 1 in place of 0 from six halvings on
           'no_schedule',        # k_r = k in every iteration
           'd_after_m',          # D o M in place of M o D
           'decay_first',        # the decay applied to D before composing
           'fit_occluded',       # occluded pixels fitted
           'border_clamp',       # the border clamped in place of uncovered
           'no_round')           # the rounding term of the >> 9 dropped


def quant(c):
    """csrc/mid_common.h's 8.8 colour: fmaxf / fminf, so a NaN is 0."""
    assert c.dtype == np.float32
    return np.rint(np.fmin(np.fmax(c, F32(0)), F32(255)) * F32(256)).astype(np.int64)


def coords(h, w, mutant=None):
    """(X, Y) int64 [h, w]: half pixels about the frame centre."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing='ij')
    off = 1 if mutant == 'centre_half' else 0
    return 2 * xx - (w - 1) + off, 2 * yy - (h - 1) + off


def quantise(flow):
    """flow fp32 [h, w, 2] -> (valid, U, V): the validity test before any conversion, then rintf(u * 64)."""
    assert flow.dtype == np.float32
    with np.errstate(invalid='ignore'):
        valid = (np.abs(flow[..., 0]) < LIMIT) & (np.abs(flow[..., 1]) < LIMIT)
    f = np.where(valid[..., None], flow, F32(0)) * F32(64)
    assert f.dtype == np.float32
    UV = np.rint(f).astype(np.int64)
    return valid, UV[..., 0], UV[..., 1]


def residual(P, X, Y, U, V, mutant=None):
    """e = |r_u| + |r_v| in 2^-16 px, int64."""
    rnd = 0 if mutant == 'no_round' else 256
    pu = P[0] + ((P[1] * X + P[2] * Y + rnd) >> 9)
    pv = P[3] + ((P[4] * X + P[5] * Y + rnd) >> 9)
    return np.abs((U << 10) - pu) + np.abs((V << 10) - pv)


def _round_clamp(v, lim):
    x = float(np.rint(np.float64(v)))
    if not x < lim:
        x = float(lim)
    if x < -lim:
        x = float(-lim)
    return int(x)


def solve(S):
    """The thirteen integer sums -> P (a list of six Python ints), or None: degenerate.  Scalar fp64, the header's order."""
    if S[12] < N_MIN:
        return None
    A00, A01, A02, A11, A12, A22 = (float(int(v)) for v in S[:6])
    a00 = A00
    if not a00 > 0.0:
        return None
    m1 = A01 / a00
    m2 = A02 / a00
    a11 = A11 - m1 * A01
    a12 = A12 - m1 * A02
    a22 = A22 - m2 * A02
    if not a11 > 0.0:
        return None
    m3 = a12 / a11
    a22 = a22 - m3 * a12
    if not a22 > 0.0:
        return None
    P = []
    for c in range(2):
        b0, b1, b2 = (float(int(v)) for v in S[6 + 3 * c:9 + 3 * c])
        b1p = b1 - m1 * b0
        b2p = (b2 - m2 * b0) - m3 * b1p
        p2 = b2p / a22
        p1 = (b1p - a12 * p2) / a11
        p0 = ((b0 - A01 * p1) - A02 * p2) / a00
        P += [_round_clamp(p0 * 1024.0, T_MAX), _round_clamp(p1 * 524288.0, L_MAX), _round_clamp(p2 * 524288.0, L_MAX)]
    return P


def sums_of(g, X, Y, U, V):
    s = lambda a: int(a.sum())            # noqa: E731
    gX, gY, gU, gV = g * X, g * Y, g * U, g * V
    return [s(g), s(gX), s(gY), s(gX * X), s(gX * Y), s(gY * Y), s(gU), s(gU * X), s(gU * Y), s(gV), s(gV * X), s(gV * Y), s(g > 0)]


def fit(flow, occ, h, w, k, R, mutant=None):
    """The fit of one pair: (P, the status word, n of the last successful iteration, what the other steps need)."""
    assert 0 <= k <= 4 and 0 <= R <= 4 and 1 <= h <= SIZE_MAX and 1 <= w <= SIZE_MAX
    valid, U, V = quantise(np.ascontiguousarray(flow[:h, :w]))
    masked = np.zeros((h, w), bool) if occ is None else occ[:h, :w] != 0
    elig = valid if mutant == 'fit_occluded' else valid & ~masked
    X, Y = coords(h, w, mutant)
    P, ok, n_last, trace = [0] * 6, 0, 0, []
    for r in range(R + 1):
        if r == 0:
            g = elig.astype(np.int64)
        else:
            kr = k if mutant == 'no_schedule' else max(0, k - (R - r))
            d = np.minimum(residual(P, X, Y, U, V, mutant) >> (17 - kr), 6)
            g = np.where(d >= 6, 1 if mutant == 'floor_one' else 0, 64 >> d) * elig
        S = sums_of(g, X, Y, U, V)
        assert max(abs(v) for v in S) < 2 ** 62
        new = solve(S)
        trace.append((S, new))
        if new is None:
            break
        P, ok, n_last = new, ok + 1, S[12]
    return P, (0 if ok else 1) | (ok << 8), n_last, dict(valid=valid, masked=masked, elig=elig, U=U, V=V, X=X, Y=Y, trace=trace)


def compose(D, P, s, mutant=None):
    """The path after one pair: M o D, the follow decay, the clamps.  D, P: six Python ints."""
    D = [int(v) for v in D]
    if mutant == 'decay_first' and s:
        D = [i + (v - i) - ((v - i) >> s) for v, i in zip(D, IDENTITY)]
    half = 1 << 23
    Ml = (ONE + P[1], P[2], P[4], ONE + P[5])                 # xx, xy, yx, yy
    Dt, Dl = (D[0], D[3]), (D[1], D[2], D[4], D[5])
    if mutant == 'd_after_m':
        A, Bm, t0, t1 = Dl, Ml, (P[0], P[3]), Dt              # D o M: Dt + Dl T, Dl Ml
    else:
        A, Bm, t0, t1 = Ml, Dl, Dt, (P[0], P[3])              # M o D: T + Ml Dt, Ml Dl
    nt = (t1[0] + ((A[0] * t0[0] + A[1] * t0[1] + half) >> 24), t1[1] + ((A[2] * t0[0] + A[3] * t0[1] + half) >> 24))
    nl = ((A[0] * Bm[0] + A[1] * Bm[2] + half) >> 24, (A[0] * Bm[1] + A[1] * Bm[3] + half) >> 24,
          (A[2] * Bm[0] + A[3] * Bm[2] + half) >> 24, (A[2] * Bm[1] + A[3] * Bm[3] + half) >> 24)
    N = [nt[0], nl[0], nl[1], nt[1], nl[2], nl[3]]
    out = []
    for j, (v, i) in enumerate(zip(N, IDENTITY)):
        if s and mutant != 'decay_first':
            E = v - i
            v = i + E - (E >> s)
        lim = DT_MAX if j in (0, 3) else DL_MAX
        out.append(min(max(v, -lim), lim))
    return out


def stabilised(frame, D, h, w, mutant=None):
    """The later frame sampled at D: (uint8 [h, w, 3], the uncovered pixels)."""
    X, Y = coords(h, w, mutant)
    rnd = 0 if mutant == 'no_round' else 256
    Px = 2 * (D[0] + ((D[1] * X + D[2] * Y + rnd) >> 9)) + ((w - 1) << 16)
    Py = 2 * (D[3] + ((D[4] * X + D[5] * Y + rnd) >> 9)) + ((h - 1) << 16)
    covered = (Px >= 0) & (Px <= (w - 1) << 17) & (Py >= 0) & (Py <= (h - 1) << 17)
    if mutant == 'border_clamp':
        Px, Py = np.clip(Px, 0, (w - 1) << 17), np.clip(Py, 0, (h - 1) << 17)
        covered = np.ones_like(covered)
    Px, Py = np.where(covered, Px, 0), np.where(covered, Py, 0)
    ix, iy, qx, qy = Px >> 17, Py >> 17, ((Px >> 9) & 255)[..., None], ((Py >> 9) & 255)[..., None]
    jx, jy = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    q = quant(np.ascontiguousarray(frame[:h, :w]).astype(np.float32))
    s = (256 - qx) * (256 - qy) * q[iy, ix] + qx * (256 - qy) * q[iy, jx] + (256 - qx) * qy * q[jy, ix] + qx * qy * q[jy, jx]
    out = (s + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return np.where(covered[..., None], out, 0).astype(np.uint8), int((~covered).sum())


def stabilise_pair(frame, flow, occ, h, w, k, R, s, D, mutant=None):
    """One valid pair: dict(motion int64 [8], path int64 [8], resid uint8 [h, w], stab uint8 [h, w, 3], counts int64 [4]) and the
    fit's details; D: the path before the pair."""
    P, status, n_last, info = fit(flow, occ, h, w, k, R, mutant)
    e = residual(P, info['X'], info['Y'], info['U'], info['V'], mutant)
    resid = np.where(info['valid'], np.minimum(e >> 14, 255), 255).astype(np.uint8)
    moving = info['elig'] & (np.minimum(e >> (17 - k), 6) >= 6)
    D = compose(D, P, s, mutant)
    stab, bare = stabilised(frame, D, h, w, mutant)
    counts = np.array([info['valid'].sum(), (info['valid'] & ~info['elig']).sum(), moving.sum(), bare], np.int64)
    return dict(motion=np.array(P + [status, n_last], np.int64), path=np.array(D + [0, 0], np.int64), resid=resid, stab=stab,
                counts=counts), info


def replay(case, path, mutant=None):
    """One launch: ({valid slot: stabilise_pair's dict}, the path state it leaves, {slot: the fit's details}).  path: the state on
    entry (eight ints), read only with a carry source above 0."""
    h, w = case['h'], case['w']
    D = list(IDENTITY) if case['carry'] == 0 else [int(v) for v in path[:6]]
    outs, infos = {}, {}
    for i in case['valid']:
        occ = None if case['occ'] is None else case['occ'][i]
        outs[i], infos[i] = stabilise_pair(case['frames'][i], case['flow_fw'][i], occ, h, w, case['tol'], case['iters'], case['follow'], D,
                                           mutant)
        D = [int(v) for v in outs[i]['path'][:6]]
    new_path = np.array(D + [0, 0], np.int64) if case['valid'] else np.asarray(path, np.int64).copy()
    return outs, new_path, infos


OUTPUTS = ('motion', 'path', 'resid', 'stab', 'counts')


def compare(case, outs, got, sentinels):
    """The comparator of the GPU test: got = {name: what one launch left in that output, [Brows, ...] with Brows >= B, filled with
    sentinels[name] before the launch} against the mirror's outs: equal on every valid slot — every word and every pixel — and the
    sentinel everywhere else: slots that are no pairs, pixels outside (h, w), rows beyond B.  Returns the pixels compared."""
    h, w = case['h'], case['w']
    assert sorted(outs) == list(case['valid']) and sorted(got) == sorted(OUTPUTS)
    rest = {k: np.ones(got[k].shape, bool) for k in OUTPUTS}
    seen = 0
    for i, o in outs.items():
        for k in ('motion', 'path', 'counts'):
            assert np.array_equal(got[k][i].astype(np.int64), o[k]), ("slot %d: %s" % (i, k), got[k][i], o[k])
            rest[k][i] = False
        for k in ('resid', 'stab'):
            g = got[k][i, :h, :w]
            bad = np.argwhere(g != o[k])
            assert len(bad) == 0, ("slot %d: %s differs at %d places, first %s: got %s, mirror %s"
                                   % (i, k, len(bad), bad[0], g[tuple(bad[0])], o[k][tuple(bad[0])]))
            rest[k][i, :h, :w] = False
        seen += h * w
    for k in OUTPUTS:
        assert (got[k][rest[k]] == sentinels[k]).all(), "%s was written outside the valid pairs" % k
    return seen


# ------------------------------------------------------------------------------------------------- inputs
FLOW_KINDS = ('affine', 'block', 'smooth', 'iid12', 'wild', 'few', 'column', 'diagonal')
PATTERNS = M.PATTERNS            # first, nopairs, full (carried), short, short2 (two of three): (new frames, carry source)
SHAPES = {'odd': dict(B=3, Hmax=40, Wmax=64, h=37, w=53),       # integer centre; the pitch is not the width
          'even': dict(B=3, Hmax=40, Wmax=64, h=40, w=64)}      # half-integer centre; the frame fills its buffer
BIG = dict(B=1, Hmax=600, Wmax=900, h=600, w=900)               # one pair past a block row's threads
AFFINE_T = (3.25, -1.5)          # px; with AFFINE_L per pixel: exact at 1/64 px about an integer centre
AFFINE_L = ((1 / 64, 1 / 32), (-1 / 32, 1 / 64))
BLOCK = dict(y0=9, x0=20, side=16, move=(-5.0, 6.0))


def affine_flow(h, w, T_=AFFINE_T, L=AFFINE_L):
    """fp32 [h, w, 2]: u = Tu + Lux (x - cx) + Luy (y - cy), v likewise, about the frame centre."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    dx, dy = xx - (w - 1) / 2, yy - (h - 1) / 2
    return np.stack([T_[0] + L[0][0] * dx + L[0][1] * dy, T_[1] + L[1][0] * dx + L[1][1] * dy], axis=-1).astype(np.float32)


def affine_words(T_=AFFINE_T, L=AFFINE_L):
    """The model words of affine_flow: T in 2^-16 px, L in 2^-24 per pixel."""
    return [int(T_[0] * 65536), int(L[0][0] * ONE), int(L[0][1] * ONE), int(T_[1] * 65536), int(L[1][0] * ONE), int(L[1][1] * ONE)]


def draw_flows(rs, B, Hmax, Wmax, h, w, kind):
    """[B, Hmax, Wmax, 2] fp32: a flow of `kind` in the (h, w) corner of every slot, NaN outside it (never to be read)."""
    f = np.full((B, Hmax, Wmax, 2), np.nan, np.float32)
    if kind in ('affine', 'block'):
        for b in range(B):
            f[b, :h, :w] = affine_flow(h, w, (AFFINE_T[0] - b, AFFINE_T[1] + 0.5 * b))
            if kind == 'block':
                y0, x0, side = BLOCK['y0'], BLOCK['x0'] + b, BLOCK['side']
                f[b, y0:y0 + side, x0:x0 + side] = BLOCK['move']
    elif kind == 'iid12':
        f[:, :h, :w] = (rs.rand(B, h, w, 2) * 24 - 12).astype(np.float32)
    else:
        f = T.draw_flows(rs, B, Hmax, Wmax, h, w, 'smooth')
    if kind == 'wild':
        bad = (np.nan, np.inf, -np.inf, 4096.0, -4096.0, 4095.98, -4095.98, 1e7)
        for b in range(B):
            for m, val in enumerate(bad):
                f[b, (5 * m + b + 1) % h, (7 * m + 3 * b + 2) % w, (m + b) % 2] = val
            f[b, (b + 11) % h, (b + 13) % w] = (np.nan, np.inf)
    keep = None
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    if kind == 'few':                                         # fewer than 16 valid pixels
        keep = (yy % 13 == 4) & (xx % 17 == 6)
        assert 3 <= keep.sum() < N_MIN
    elif kind == 'column':                                    # one valid column
        keep = xx == w // 3
    elif kind == 'diagonal':                                  # one valid diagonal
        keep = xx == yy
    if keep is not None:
        f[:, :h, :w][:, ~keep] = np.nan
    return f


def draw_path(rs):
    """A path state in mid-clip: a few pixels of translation, a linear part near the identity."""
    D = np.array(IDENTITY + (0, 0), np.int64)
    D[[0, 3]] += rs.randint(-6 << 16, 6 << 16, 2)
    D[[1, 2, 4, 5]] += rs.randint(-(ONE >> 5), ONE >> 5, 4)
    return D


def make_case(name, B, Hmax, Wmax, h, w, u8, bidir, kind, pattern, tol, iters, follow):
    """One launch: the tables of sequence_tables, B staged frames, the forward flows, the forward masks of a bidirectional
    estimator (blobs), the options and the path state on entry (poisoned when nothing is carried)."""
    from unflow_amd.core.inference import sequence_tables
    rs = WP._rs('stabilise', name, u8, bidir, kind, pattern, tol, iters, follow)
    k, carry = PATTERNS[pattern]
    k = B if k is None else k
    carry = B if carry is None else carry
    tab, valid, _ = sequence_tables((h, w), k, B, carry, u8=u8)
    fr = M.draw_frames(rs, B, Hmax, Wmax, h, w, u8)
    path = draw_path(rs) if carry else np.full(8, -(1 << 62) + 12345, np.int64)
    return dict(name=name, B=B, Hmax=Hmax, Wmax=Wmax, h=h, w=w, u8=u8, bidir=bidir, kind=kind, pattern=pattern, k=k, carry=carry,
                tab=tab, valid=valid, frames=np.ascontiguousarray(fr[1:]), flow_fw=draw_flows(rs, B, Hmax, Wmax, h, w, kind),
                occ=T.draw_occ(rs, B, Hmax, Wmax, h, w) if bidir else None, tol=tol, iters=iters, follow=follow, path=path,
                id='%s-%s-%s-%s-%s-k%dR%ds%d' % (name, 'u8' if u8 else 'f32', 'bidir' if bidir else 'fw', kind, pattern, tol, iters,
                                                   follow))


@functools.lru_cache(maxsize=None)
def entry_cases():
    """The launches of the entry-point tests, (id, case): every flow kind at every (tol, iters) of TOLS x ITERS, the two shapes, the
    two frame types, one and both directions and the two follows taking turns with periods that do not divide nine; every replay
    pattern in one and in both directions; and one 600 x 900 pair."""
    out, m = [], 0
    for kind in FLOW_KINDS:
        for tol in TOLS:
            for iters in ITERS:
                shape = ('odd', 'even')[m % 2]
                out.append(make_case(shape, u8=(m // 4) % 2 == 0, bidir=(m // 8) % 2 == 1, kind=kind, pattern='full', tol=tol,
                                     iters=iters, follow=FOLLOWS[(m // 2) % 2], **SHAPES[shape]))
                m += 1
    for n, pattern in enumerate(('first', 'nopairs', 'short', 'short2')):
        for bidir in (False, True):
            out.append(make_case('odd', u8=(n % 2 == 0) != bidir, bidir=bidir, kind='block' if bidir else 'smooth', pattern=pattern,
                                 tol=2, iters=3, follow=3 if bidir else 0, **SHAPES['odd']))
    out.append(make_case('big', u8=True, bidir=False, kind='smooth', pattern='full', tol=2, iters=3, follow=0, **BIG))
    assert len({c['id'] for c in out}) == len(out)
    return [(c['id'], c) for c in out]


@functools.lru_cache(maxsize=None)
def mirror_of(cid):
    """replay of entry case `cid` from its own path state, computed once and shared: (outs, new path, infos).  Read-only."""
    case = dict(entry_cases())[cid]
    return replay(case, case['path'])
