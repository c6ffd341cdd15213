"""No GPU: the definition of unflow_sequence_stabilise as tests/stabilise_ref.py states it — what the fit recovers and
where it gives up, the path in lock and follow mode, the composition against exact rational arithmetic, the mutants of the mirror,
and the host side of the option: the table rows, the file list, the option parser, the command line and the entry's refusals."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import stabilise_ref as R

CASES = R.entry_cases()
BY_ID = dict(CASES)
H, W, HM, WM = 37, 53, 40, 64
WORDS = R.affine_words()


def _in_buffer(core):
    f = np.full((HM, WM, 2), np.nan, np.float32)
    f[:H, :W] = core
    return f


def _affine():
    return _in_buffer(R.affine_flow(H, W))


def _block():
    f = _affine()
    b = R.BLOCK
    f[b['y0']:b['y0'] + b['side'], b['x0']:b['x0'] + b['side']] = b['move']
    return f


# ------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("k", range(5))
def test_the_dyadic_affine_is_recovered_exactly(k):
    """Translation (3.25, -1.5), coefficients 1 / 64 and +-1 / 32 about an integer centre: every quantised flow is exact, and the
    fit returns the model's words at every tolerance; all pixels are used and the residual map is zero."""
    assert WORDS == [212992, 262144, 524288, -98304, -524288, 262144]
    P, status, n, info = R.fit(_affine(), None, H, W, k, 3)
    assert P == WORDS and status == 4 << 8 and n == H * W
    assert not R.residual(P, info['X'], info['Y'], info['U'], info['V']).any()


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("iters", range(5))
def test_the_occluder_is_voted_out(k, iters):
    """A 16 x 16 block of the 37 x 53 frame moves (-5, 6) instead: 256 outliers of 1961 pixels.  The background's model comes back
    exactly for k <= 3 from one reweighted fit on and for k = 4 from two on, from the 1705 background pixels."""
    P, status, n, info = R.fit(_block(), None, H, W, k, iters)
    exact = iters >= (2 if k == 4 else 1)
    assert (P == WORDS) == exact, (k, iters, P)
    if exact:
        # (k = 3 with one reweighted fit is exact from the 121 pixels that the contaminated first fit leaves within reach)
        assert status == (iters + 1) << 8 and n == (121 if (k, iters) == (3, 1) else H * W - 256)
        e = R.residual(P, info['X'], info['Y'], info['U'], info['V'])
        b = R.BLOCK
        inside = np.zeros((H, W), bool)
        inside[b['y0']:b['y0'] + b['side'], b['x0']:b['x0'] + b['side']] = True
        assert not e[~inside].any() and (e[inside] >> (17 - k) >= 6).all()         # the block is what moves


def test_tolerance_four_with_one_iteration_keeps_the_contaminated_fit():
    """k = 4, R = 1: under the contaminated first fit no pixel is within six halvings of 1 / 8 px, the second iteration has no usable
    weight, is degenerate and keeps the first fit — one successful iteration, all pixels."""
    first = R.fit(_block(), None, H, W, 4, 0)
    P, status, n, info = R.fit(_block(), None, H, W, 4, 1)
    assert P == first[0] and P != WORDS and status == 1 << 8 and n == H * W
    S, new = info['trace'][1]
    assert new is None and S[12] < R.N_MIN


def test_the_masked_fit_needs_no_iteration():
    """With the block under the occlusion mask the first fit (R = 0) sees the background alone and is exact; the occluded pixels
    are valid, not eligible, and never counted as moving."""
    b = R.BLOCK
    occ = np.ones((HM, WM), np.uint8)
    occ[:H, :W] = 0
    occ[b['y0']:b['y0'] + b['side'], b['x0']:b['x0'] + b['side']] = 1
    P, status, n, _ = R.fit(_block(), occ, H, W, 2, 0)
    assert P == WORDS and status == 1 << 8 and n == H * W - 256
    frame = np.zeros((HM, WM, 3), np.uint8)
    out, _ = R.stabilise_pair(frame, _block(), occ, H, W, 2, 0, 0, list(R.IDENTITY))
    assert out['counts'].tolist()[:3] == [H * W, 256, 0]
    assert R.fit(_block(), None, H, W, 2, 0)[0] != WORDS                      # unmasked, the block pulls the first fit


@pytest.mark.parametrize("kind", ['few', 'column', 'diagonal', 'nan'])
def test_degenerate_inputs_give_the_identity(kind):
    """Fewer than 16 valid pixels, one valid column, one valid diagonal, no valid pixel: P = 0, status 1, no iteration counted, and
    the path does not move."""
    rs = np.random.RandomState(5)
    for name, shape in R.SHAPES.items():
        h, w = shape['h'], shape['w']
        if kind == 'nan':
            f = np.full((1, HM, WM, 2), np.nan, np.float32)
        else:
            f = R.draw_flows(rs, 1, HM, WM, h, w, kind)
        for iters in (0, 3):
            P, status, n, info = R.fit(f[0], None, h, w, 2, iters)
            assert P == [0] * 6 and status == 1 and n == 0, (kind, name, P, status)
            assert len(info['trace']) == 1                                    # the loop ended at its first iteration
        assert (info['valid'].sum() >= R.N_MIN) == (kind in ('column', 'diagonal'))
        D = R.draw_path(rs).tolist()[:6]
        assert R.compose(D, P, 0) == D


def test_invalid_components_are_tested_before_any_conversion():
    f = _affine()
    bad = [np.nan, np.inf, -np.inf, 4096.0, -4096.0, 1e30]
    for m, v in enumerate(bad):
        f[3 + m, 5 + 2 * m, m % 2] = v
    f[20, 20] = (4095.98, -4095.98)
    valid, U, V = R.quantise(np.ascontiguousarray(f[:H, :W]))
    assert valid.sum() == H * W - len(bad) and valid[20, 20]
    assert U[20, 20] == int(np.rint(np.float32(4095.98) * np.float32(64))) == -V[20, 20] and abs(U[20, 20]) < 1 << 18
    out, _ = R.stabilise_pair(np.zeros((HM, WM, 3), np.uint8), f, None, H, W, 2, 3, 0, list(R.IDENTITY))
    assert out['counts'][0] == H * W - len(bad) and (out['resid'][~valid] == 255).all() and out['resid'][20, 20] == 255
    assert out['motion'][:6].tolist() == WORDS                                # the wild pixel is voted out, the rest is exact


# ------------------------------------------------------------------------------------------------- the path
def test_lock_mode_shows_every_frame_of_a_shaken_clip_in_the_first_frames_coordinates():
    """One texture seen through a window that is shaken by integer offsets, the flows exact: with follow = 0 every stabilised frame
    equals frame 0 bit for bit where it is covered, and the uncovered pixels are the border the accumulated offset leaves."""
    rs = np.random.RandomState(11)
    pad = 12
    canvas = rs.randint(0, 256, (H + 2 * pad, W + 2 * pad, 3)).astype(np.uint8)
    shake = [(3, -2), (-5, 1), (4, 4), (-1, -6), (2, 3)]                      # the content's move per pair, (x, y)
    frames, pos = [], np.zeros(2, int)
    for d in [(0, 0)] + shake:
        pos += d
        fr = np.full((HM, WM, 3), 255, np.uint8)
        fr[:H, :W] = canvas[pad - pos[1]:pad - pos[1] + H, pad - pos[0]:pad - pos[0] + W]
        frames.append(fr)
    D, total = list(R.IDENTITY), np.zeros(2, int)
    for n, d in enumerate(shake):
        flow = _in_buffer(np.broadcast_to(np.asarray(d, np.float32), (H, W, 2)))
        out, _ = R.stabilise_pair(frames[n + 1], flow, None, H, W, 2, 3, 0, D)
        total += d
        assert out['motion'][:6].tolist() == [d[0] << 16, 0, 0, d[1] << 16, 0, 0]
        D = out['path'][:6].tolist()
        assert D == [int(total[0]) << 16, R.ONE, 0, int(total[1]) << 16, 0, R.ONE]
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        covered = (xx + total[0] >= 0) & (xx + total[0] < W) & (yy + total[1] >= 0) & (yy + total[1] < H)
        border = H * W - (H - abs(int(total[1]))) * (W - abs(int(total[0])))
        assert out['counts'][3] == border == (~covered).sum() and border > 0
        assert np.array_equal(out['stab'][covered], frames[0][:H, :W][covered])
        assert not out['stab'][~covered].any()
        assert not out['resid'].any() and out['counts'].tolist()[:3] == [H * W, 0, 0]


def test_follow_mode_by_hand():
    """s = 3 from the identity under the dyadic model: every word of D' loses an eighth of its offset from the identity, the shift
    rounding towards minus infinity; a still pair then decays what is left by another eighth."""
    D = R.compose(list(R.IDENTITY), WORDS, 3)
    # D' = {212992, 2^24 + 262144, 524288, -98304, -524288, 2^24 + 262144}; E >> 3 = 26624, 32768, 65536, -12288, -65536, 32768
    assert D == [186368, R.ONE + 229376, 458752, -86016, -458752, R.ONE + 229376]
    assert R.compose(list(R.IDENTITY), WORDS, 0) == [212992, R.ONE + 262144, 524288, -98304, -524288, R.ONE + 262144]
    still = R.compose(D, [0] * 6, 3)
    assert still == [186368 - 23296, R.ONE + 229376 - 28672, 458752 - 57344, -86016 + 10752, -458752 + 57344, R.ONE + 229376 - 28672]
    assert R.compose([-7, R.ONE, 0, 7, 0, R.ONE], [0] * 6, 3) == [-6, R.ONE, 0, 7, 0, R.ONE]      # -7 - (-7 >> 3) = -7 + 1
    # the clamps
    far = R.compose([R.DT_MAX, R.DL_MAX, 0, -R.DT_MAX, 0, R.DL_MAX], [R.T_MAX, R.L_MAX, 0, -R.T_MAX, 0, R.L_MAX], 0)
    assert far == [R.DT_MAX, R.DL_MAX, 0, -R.DT_MAX, 0, R.DL_MAX]


def test_composition_equals_exact_rational_arithmetic_on_small_words():
    """M o D on random small words: the integer form — two products summed, one rounding — is floor(exact + 1 / 2) of the rational
    map composition in the path's units, entry by entry."""
    rs = np.random.RandomState(3)
    for _ in range(200):
        P = [int(v) for v in rs.randint(-(1 << 20), 1 << 20, 6)]
        D = [int(v) for v in rs.randint(-(1 << 20), 1 << 20, 6)]
        D[1] += R.ONE
        D[5] += R.ONE
        Ml = [[Fraction(R.ONE + P[1], R.ONE), Fraction(P[2], R.ONE)], [Fraction(P[4], R.ONE), Fraction(R.ONE + P[5], R.ONE)]]
        Dl = [[Fraction(D[1], R.ONE), Fraction(D[2], R.ONE)], [Fraction(D[4], R.ONE), Fraction(D[5], R.ONE)]]
        Dt = [Fraction(D[0], 65536), Fraction(D[3], 65536)]
        rnd = lambda x: (x + Fraction(1, 2)).__floor__()          # noqa: E731
        want_t = [P[3 * i] + rnd((Ml[i][0] * Dt[0] + Ml[i][1] * Dt[1]) * 65536) for i in range(2)]
        want_l = [[rnd((Ml[i][0] * Dl[0][j] + Ml[i][1] * Dl[1][j]) * R.ONE) for j in range(2)] for i in range(2)]
        got = R.compose(D, P, 0)
        assert got == [want_t[0], want_l[0][0], want_l[0][1], want_t[1], want_l[1][0], want_l[1][1]]


def test_the_stabilised_frame_interpolates_in_fixed_point():
    """A half-pixel path on a ramp: the byte is the rounded mean of the two neighbours' 8.8 colours, the last column's neighbour is
    itself, and one step further the pixel is uncovered."""
    fr = np.zeros((HM, WM, 3), np.float32)
    fr[:H, :W] = (np.arange(W, dtype=np.float32) * 4 + 0.25)[None, :, None]
    out, bare = R.stabilised(fr, [1 << 15, R.ONE, 0, 0, 0, R.ONE], H, W)
    q = R.quant(fr[0, :W, 0])
    assert bare == H and (out[:, W - 1] == 0).all()
    assert np.array_equal(out[5, :W - 1, 1], (128 * 256 * (q[:-1] + q[1:]) + (1 << 23)) >> 24)
    out, bare = R.stabilised(fr, list(R.IDENTITY), H, W)
    assert bare == 0 and np.array_equal(out[7, :, 2], (q * 65536 + (1 << 23)) >> 24)


# ------------------------------------------------------------------------------------------------- the mirror and its mutants
SMALL = [cid for cid, c in CASES if c['name'] != 'big']


def _equal(a, b):
    return sorted(a[0]) == sorted(b[0]) and np.array_equal(a[1], b[1]) and \
        all(np.array_equal(a[0][i][k], b[0][i][k]) for i in a[0] for k in R.OUTPUTS)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_a_case(mutant):
    caught = []
    for cid in SMALL:
        case = BY_ID[cid]
        if not _equal(R.replay(case, case['path'], mutant), R.mirror_of(cid)):
            caught.append(cid)
            if len(caught) == 3:
                break
    print(mutant, caught)
    assert caught, mutant


def test_the_case_list_crosses_what_the_issue_lists():
    full = [c for _, c in CASES if c['pattern'] == 'full' and c['name'] != 'big']
    for kind in R.FLOW_KINDS:
        mine = [c for c in full if c['kind'] == kind]
        assert {(c['tol'], c['iters']) for c in mine} == {(k, r) for k in R.TOLS for r in R.ITERS}
        assert {c['name'] for c in mine} == {'odd', 'even'} and {c['follow'] for c in mine} == set(R.FOLLOWS)
        assert {c['u8'] for c in mine} == {False, True}
    assert {(c['u8'], c['bidir']) for c in full} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c['pattern'] for _, c in CASES} == {'first', 'nopairs', 'full', 'short', 'short2'}
    big = BY_ID[[cid for cid in BY_ID if cid.startswith('big')][0]]
    assert big['h'] * big['w'] > 2048 * 256 and (big['h'], big['w']) == (600, 900)
    assert all((c['occ'] is not None) == c['bidir'] for _, c in CASES)
    # every weight, and the floor, occurs often: a GPU test against this mirror cannot pass with one of them dead
    seen = np.zeros(7, np.int64)
    for cid in SMALL:
        case = BY_ID[cid]
        if case['iters'] == 0:
            continue
        for i, info in R.mirror_of(cid)[2].items():
            P = R.mirror_of(cid)[0][i]['motion'][:6].tolist()
            e = R.residual(P, info['X'], info['Y'], info['U'], info['V'])
            seen += np.bincount(np.minimum(e[info['elig']] >> (17 - case['tol']), 6), minlength=7)
    assert (seen > 100).all(), seen


def test_replay_patterns_and_the_path_state():
    """A first replay starts from the identity whatever the state holds; a replay without a pair leaves the state alone; a carried
    one continues from it."""
    first = next(c for _, c in CASES if c['pattern'] == 'first' and not c['bidir'])
    a = R.replay(first, first['path'])
    b = R.replay(first, np.arange(8, dtype=np.int64) * 1000)
    assert first['carry'] == 0 and first['valid'] == [1, 2] and _equal(a, b)
    none = next(c for _, c in CASES if c['pattern'] == 'nopairs')
    outs, path, _ = R.replay(none, none['path'])
    assert outs == {} and np.array_equal(path, none['path'])
    full = BY_ID['odd-u8-fw-affine-full-k0R0s0']
    moved = R.replay(full, full['path'])
    assert full['carry'] > 0 and not _equal(moved, R.replay(full, np.array(R.IDENTITY + (0, 0), np.int64)))
    short2 = next(c for _, c in CASES if c['pattern'] == 'short2')
    assert short2['valid'] == [0, 1] and short2['B'] == 3


def test_mirror_is_deterministic_and_leaves_its_inputs_alone():
    cid = SMALL[7]
    case = BY_ID[cid]
    before = {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}
    assert _equal(R.replay(case, case['path']), R.mirror_of(cid))
    assert all(np.array_equal(case[k], v, equal_nan=v.dtype.kind == 'f') for k, v in before.items())


# ------------------------------------------------------------------------------------------------- the host side
def test_table_rows_and_file_list():
    from unflow_amd.core import inference as I
    plain = I.output_buffers(2, 8, 16, 5, 3, True, held_out=True)
    rows = I.output_buffers(2, 8, 16, 5, 3, True, held_out=True, stabilise=True)
    assert rows[:len(plain)] == plain and I.output_buffers(2, 8, 16) == I.output_buffers(2, 8, 16, stabilise=False)
    import torch
    assert [(r[0], r[1], r[2], r[3], r[4]) for r in rows[len(plain):]] == [
        ('stab', 'out_stab', (2, 8, 16, 3), torch.uint8, 'stabilise'),
        ('stab_resid', 'out_stab_resid', (2, 8, 16), torch.uint8, 'stabilise'),
        ('stab_motion', 'out_stab_motion', (2, 8), torch.int64, 'stabilise'),
        ('stab_path', 'out_stab_path', (2, 8), torch.int64, 'stabilise'),
        ('stab_counts', 'out_stab_counts', (2, 4), torch.int32, 'stabilise')]
    assert I.FlowEstimator.STAB_WANT == tuple(r[0] for r in rows[len(plain):])
    base = I.pair_files(7, 'png', True, True, I.sequence_visual_files(7, True), track=True, mid=2)
    files = I.pair_files(7, 'png', True, True, I.sequence_visual_files(7, True), track=True, mid=2, stab=True)
    assert files[:len(base)] == base and files[len(base):] == [('000007_stab.png', ('png', 'stab', 0)),
                                                               ('000007_motion.png', ('png', 'stab_resid', 0))]
    assert I.pair_files(7, 'flo', stab=True)[1:] == files[len(base):]
    assert I.filter_entries(I.pair_files(0, 'flo', stab=True), [(1, 5, 6)], 2) == [('stab', 1, 5, 6), ('stab_resid', 1, 5, 6)]


def test_the_option_parser():
    from unflow_amd.core import inference as I
    assert I.stabilise_option(None) is None and I.stabilise_option(False) is None
    assert I.stabilise_option(True) == dict(tol=2, iters=3, follow=0) == I.STABILISE_DEFAULTS
    assert I.stabilise_option(dict(follow=8, tol=0)) == dict(tol=0, iters=3, follow=8)
    assert I.stabilise_option({}) == I.STABILISE_DEFAULTS
    for bad in (1, 'yes', dict(tol=5), dict(tol=-1), dict(iters=5), dict(follow=9), dict(follow=-1), dict(tol=2.0), dict(tol=True),
                dict(steps=1), [2, 3, 0]):
        with pytest.raises(ValueError, match="stabilise"):
            I.stabilise_option(bad)
    with pytest.raises(ValueError, match="stabilise.*needs sequence=True"):
        I.FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), stabilise=True)
    with pytest.raises(ValueError, match="stabilise\\['iters'\\]"):
        I.FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), sequence=True, stabilise=dict(iters=7))


def test_camera_matrix():
    from unflow_amd.core.inference import camera_matrix
    A = camera_matrix(WORDS + [0, 0], H, W)
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    assert A.shape == (2, 3) and A.dtype == np.float64
    assert np.array_equal(A[:, :2], np.array([[1 + 1 / 64, 1 / 32], [-1 / 32, 1 + 1 / 64]]))
    flow = R.affine_flow(H, W).astype(np.float64)
    for x, y in ((0, 0), (52, 36), (26, 18), (7, 30)):
        assert np.allclose(A @ [x, y, 1], np.array([x, y]) + flow[y, x], atol=1e-12)
    assert np.allclose(A @ [c[0], c[1], 1], c + [3.25, -1.5])
    Dm = camera_matrix([5 << 16, R.ONE, 0, -(3 << 16), 0, R.ONE], H, W, path=True)
    assert np.array_equal(Dm, np.array([[1.0, 0.0, 5.0], [0.0, 1.0, -3.0]]))
    assert np.array_equal(camera_matrix(list(R.IDENTITY), 40, 64, path=True), np.array([[1.0, 0, 0], [0, 1.0, 0]]))


def test_the_command_line_checks_the_flags():
    from unflow_amd import sequence as S
    ap = S.parser()
    a = ap.parse_args(['--ex', 'x', '--frames', 'd'])
    assert a.stabilise is False and a.stabilise_tol is None and a.stabilise_iters is None and a.stabilise_follow is None
    a = ap.parse_args(['--ex', 'x', '--frames', 'd', '--stabilise', '--stabilise_tol', '3', '--stabilise_follow', '4'])
    assert a.stabilise and (a.stabilise_tol, a.stabilise_iters, a.stabilise_follow) == (3, None, 4)
    for bad, msg in ((['--stabilise_tol', '2'], 'needs --stabilise'), (['--stabilise', '--stabilise_tol', '5'], '0..4'),
                     (['--stabilise', '--stabilise_iters', '-1'], '0..4'), (['--stabilise', '--stabilise_follow', '9'], '0..8')):
        with pytest.raises(SystemExit) as err:
            S.parse_args(['--ex', 'x', '--frames', '.'] + bad)
        assert err.value.code == 2, (bad, msg)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from unflow_amd import _lib, build
    build.build()
    L = _lib.lib()
    one = ctypes.c_void_p(16)            # never dereferenced: the arguments are refused before anything is launched
    nul = ctypes.c_void_p(0)

    def call(B=2, Hm=40, Wm=64, tol=2, iters=3, follow=0, null=None, odd=None):
        p = {k: one for k in ('frames', 'tab', 'flow', 'occ', 'path', 'ws', 'motion', 'opath', 'resid', 'stab', 'counts')}
        if null:
            p[null] = nul
        if odd:
            p[odd] = ctypes.c_void_p(20)
        return L.unflow_sequence_stabilise(p['frames'], p['tab'], B, Hm, Wm, p['flow'], p['occ'], tol, iters, follow, p['path'], p['ws'],
                                           p['motion'], p['opath'], p['resid'], p['stab'], p['counts'], nul)
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(Hm=0), dict(Wm=0), dict(Hm=4097), dict(Wm=4097), dict(tol=-1), dict(tol=5),
               dict(iters=-1), dict(iters=5), dict(follow=-1), dict(follow=9)):
        assert call(**kw) == -5, kw
    for name in ('frames', 'tab', 'flow', 'path', 'ws', 'motion', 'opath', 'resid', 'stab', 'counts'):
        assert call(null=name) == -1, name
    for name in ('path', 'ws', 'motion', 'opath', 'flow'):
        assert call(odd=name) == -7, name
    assert call(null='frames', B=0) == -1                                     # the NULL test comes first
    size = L.unflow_sequence_stabilise_workspace_bytes
    assert size.restype is ctypes.c_size_t and L.unflow_sequence_stabilise.restype is ctypes.c_int
    assert size(0) == 0 and size(-1) == 0 and size(65536) == 0 and size(1) > 0 and size(3) == 3 * size(1) and size(1) % 8 == 0


def test_the_symbol_is_declared_and_the_build_needs_no_change():
    import os
    from unflow_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'unflow_hip.h')) as f:
        header = f.read()
    assert 'int unflow_sequence_stabilise(const void* frames, const int* tab, int B, int Hmax, int Wmax' in header
    assert 'size_t unflow_sequence_stabilise_workspace_bytes(int B);' in header
    src = os.path.join(root, 'unflow_amd', 'csrc', 'stabilise.hip')
    assert src in build.sources() and '-ffp-contract=off' in build.flags_for(src)
    with open(src) as f:
        text = f.read()
    assert 'asm' not in text and 'hipMemset' not in text and 'atomicAdd(float' not in text
