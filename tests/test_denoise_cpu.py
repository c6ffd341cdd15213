"""Temporal denoising along a clip without a GPU: tests/denoise_ref.py, the numpy definition the kernel is held to by
tests/test_denoise_gpu.py, is itself checked here — by hand on small inputs, on the noise scene, by its mutants — beside the host
side of the option (the parser, the table rows, the file list, the command line) and the entry's argument checks."""
import ctypes

import numpy as np
import pytest

import denoise_ref as R

CASES = R.entry_cases()
BY_ID = dict(CASES)
SMALL = [cid for cid, c in CASES if c['name'] != 'big']


def _hist(colours, n):
    """int64 [h, w, 4]: 8.8 colours (one grey value per pixel) with counts n."""
    c = np.asarray(colours, np.int64)
    return np.concatenate([np.repeat(c[..., None], 3, axis=-1), np.broadcast_to(np.asarray(n, np.int64), c.shape)[..., None]], axis=-1)


def _grey(v, dtype=np.uint8):
    return np.repeat(np.asarray(v, dtype)[..., None], 3, axis=-1)


# ------------------------------------------------------------------------------------------------- the definition by hand
def test_one_step_by_hand():
    """A 1 x 4 frame, zero flow but for one half-pixel fetch; counts 1, 3, 64, 64; tol 0 (d = e >> 11).  The count is the minimum
    over the four taps, the zero-weight neighbour to the right included: pixel 0 has min(1, 3), pixel 2 min(64, 64)."""
    hist = _hist([[100 << 8, 104 << 8, 50 << 8, 200 << 8]], [[1, 3, 64, 64]])
    frame = _grey([[100, 100, 50, 10]])
    bw = np.zeros((1, 4, 2), np.float32)
    bw[0, 1, 0] = -0.5                                    # pixel 1 fetches half way between pixels 0 and 1: 102, count min(1, 3)
    occ = np.zeros((1, 4), np.uint8)
    out, new = R.denoise_pair(frame, bw, occ, 1, 4, 0, 8, hist)
    # pixel 0: e = 0, neff = 1: (100 + 100) / 2; pixel 1: pred 102, e = 3 * 512, d = 0, neff = 1: (102 + 100 + 1) / 2 in 8.8
    # pixel 2: neff = 64, n' = min(65, 8); pixel 3: e = 3 * 190 * 256 >> 11 >= 6: rejected
    assert new[0, :, 0].tolist() == [100 << 8, ((102 << 8) + (100 << 8) + 1) // 2, 50 << 8, 10 << 8]
    assert new[0, :, 3].tolist() == [2, 2, 8, 1]
    assert out['den'][0, :, 0].tolist() == [100, 101, 50, 10] and (out['den'][..., 0] == out['den'][..., 2]).all()
    # E = e >> 8 = {0, 6, 0, 570 -> 255}: half = 2, the cumulative count reaches 2 in bin 0
    assert out['stats'].tolist() == [0, 0, 4, 0, 1, 13, 0, 0]
    assert hist[0, 1, 0] == 104 << 8                     # the history before the pair is not changed


def test_a_larger_distance_halves_the_history_weight():
    """d = e >> (11 + t): at t = 0 a grey distance of 3 levels (e = 3 * 3 * 256 = 2304) gives d = 1, neff = np >> 1."""
    hist = _hist([[103 << 8]], [[8]])
    frame = _grey([[100]])
    z, o = np.zeros((1, 1, 2), np.float32), np.zeros((1, 1), np.uint8)
    out, new = R.denoise_pair(frame, z, o, 1, 1, 0, 64, hist)
    assert new[0, 0].tolist() == [(4 * (103 << 8) + (100 << 8) + 2) // 5] * 3 + [5]
    out, new = R.denoise_pair(frame, z, o, 1, 1, 1, 64, hist)                 # t = 1: d = 0, the whole history counts
    assert new[0, 0].tolist() == [(8 * (103 << 8) + (100 << 8) + 4) // 9] * 3 + [9]
    assert R.denoise_pair(frame, z, o, 1, 1, 1, 4, hist)[1][0, 0, 3] == 4     # depth bounds the count, not this step's weight


def test_fresh_pixels_take_the_frame_and_start_a_history():
    hist = _hist(np.full((3, 5), 200 << 8), 64)           # 64 >> d >= 2 for every d < 6: only a FRESH pixel gets n' = 1
    frame = _grey(np.arange(15).reshape(3, 5) * 10)
    bw = np.zeros((3, 5, 2), np.float32)
    occ = np.zeros((3, 5), np.uint8)
    bw[0, 0] = (-1.0 / 64, 0)                             # leaves the frame by 1/64 px
    bw[0, 4] = (1.0 / 64, 0)
    bw[2, 2] = (0, 1.0 / 64)
    bw[1, 1] = (np.nan, 0)
    bw[1, 2] = (0, np.inf)
    bw[1, 3] = (4096.0, 0)
    bw[0, 2] = (-4095.99, 0)                              # valid, but far outside
    occ[2, 0] = 255
    out, new = R.denoise_pair(frame, bw, occ, 3, 5, 4, 8, hist)
    fresh = np.zeros((3, 5), bool)
    for y, x in ((0, 0), (0, 4), (2, 2), (1, 1), (1, 2), (1, 3), (0, 2), (2, 0)):
        fresh[y, x] = True
    assert np.array_equal(new[..., 3] == 1, fresh) and int(out['stats'][3]) == 8 and int(out['stats'][2]) == 7
    assert np.array_equal(out['den'][fresh], frame[fresh]) and np.array_equal(new[fresh][:, :3], frame[fresh].astype(np.int64) << 8)
    # the last column and row are inside: PX = (w - 1) << 6 exactly
    bw[:] = 0
    bw[:, 3, 0] = 1.0
    occ[:] = 0
    out, _ = R.denoise_pair(frame, bw, occ, 3, 5, 4, 8, hist)
    assert int(out['stats'][3]) == 0


def test_the_noise_level_is_the_lower_median_and_chooses_the_tolerance():
    bins = np.zeros(256, np.int64)
    for Mv, t in ((0, 0), (4, 0), (5, 1), (8, 1), (9, 2), (16, 2), (17, 3), (32, 3), (33, 4), (64, 4), (65, 4), (255, 4)):
        assert R.tolerance(-1, Mv) == t, Mv
        assert all(R.tolerance(k, Mv) == k for k in range(5))
    # a frame whose distances are known: grey offsets 0, 1, 2, 3 levels -> E = 3 * offset (three channels), four pixels each
    off = np.repeat(np.arange(4), 4).reshape(4, 4)
    hist = _hist(np.full((4, 4), 100 << 8), 1)
    z, o = np.zeros((4, 4, 2), np.float32), np.zeros((4, 4), np.uint8)
    out, _ = R.denoise_pair(_grey(100 + off), z, o, 4, 4, -1, 8, hist)
    assert out['stats'][:3].tolist() == [0, 3, 16]        # half = 8: reached by the bins 0 and 3; 8 << 0 >= 6
    o[0] = 1                                              # the four pixels of distance 0 become FRESH: 12 eligible, half = 6
    out, _ = R.denoise_pair(_grey(100 + off), z, o, 4, 4, -1, 8, hist)
    assert out['stats'][:4].tolist() == [1, 6, 12, 4]     # bins 3, 6 reach 8 >= 6 at bin 6; 8 << 1 >= 12
    o[:] = 1
    out, _ = R.denoise_pair(_grey(100 + off), z, o, 4, 4, -1, 8, hist)
    assert out['stats'][:4].tolist() == [0, 0, 0, 16]     # nothing eligible: M = 0


def test_uint8_and_fp32_frames_share_the_quantisation():
    rs = np.random.RandomState(5)
    fr = rs.randint(0, 256, size=(6, 7, 3)).astype(np.uint8)
    hist = np.concatenate([rs.randint(0, 65281, size=(6, 7, 3)), rs.randint(1, 9, size=(6, 7, 1))], axis=-1).astype(np.int64)
    bw = (rs.rand(6, 7, 2) * 4 - 2).astype(np.float32)
    occ = (rs.rand(6, 7) < 0.2).astype(np.uint8)
    a = R.denoise_pair(fr, bw, occ, 6, 7, -1, 8, hist)
    b = R.denoise_pair(fr.astype(np.float32), bw, occ, 6, 7, -1, 8, hist)
    assert np.array_equal(a[0]['den'], b[0]['den']) and np.array_equal(a[1], b[1]) and np.array_equal(a[0]['stats'], b[0]['stats'])
    q = R.quant(np.array([np.nan, -3.0, 0.001, 12.5, 254.999, 255.0, 300.0, np.inf], np.float32))
    assert q.tolist() == [0, 0, 0, 3200, 65280, 65280, 65280, 65280]


def test_a_static_noisy_clip_converges_to_the_running_mean():
    """Zero flow, no mask, tol 4, depth 64 on a constant image with small noise: the history is the rounded running mean and the
    count grows by one per frame."""
    rs = np.random.RandomState(3)
    frames = np.clip(np.rint(120 + rs.randn(9, 5, 6, 3) * 2), 0, 255).astype(np.uint8)
    z, o = np.zeros((5, 6, 2), np.float32), np.zeros((5, 6), np.uint8)
    hist = R.initial(np.zeros((5, 6, 4), np.int64), frames[0], 5, 6, 5, 6)
    for k in range(1, 9):
        out, hist = R.denoise_pair(frames[k], z, o, 5, 6, 4, 64, hist)
        assert (hist[..., 3] == k + 1).all() and int(out['stats'][5]) == 30 * (k + 1)
    mean = frames.astype(np.float64).mean(axis=0) * 256
    assert np.abs(hist[..., :3] - mean).max() <= 8        # eight roundings of at most half a unit each, and then some


# ------------------------------------------------------------------------------------------------- the noise scene
@pytest.mark.parametrize("sigma", [5, 10, 20])
def test_the_noise_scene(sigma):
    """40 x 64, 12 frames, a static smooth background and a textured square moving 3 px per frame, exact backward flows and masks,
    tol='auto', depth=8, squared error against the clean frames over frames 4..11: (a) a quarter of the noisy frames' at most;
    (b) at most 0.8 of the same filter's given zero flows and no mask.  Measured (noisy / denoised, zero-flow / denoised, t):
    sigma 5: 5.66, 1.71, 2; sigma 10: 5.93, 2.55, 3; sigma 20: 5.80, 2.46, 4."""
    clean, noisy, bw, occ = R.noise_scene(sigma)
    S = R.SCENE
    assert noisy.shape == (12, 40, 64, 3) and S['speed'] == 3 and S['side'] == 16
    den, stats = R.filter_clip(noisy, bw, occ)
    still, _ = R.filter_clip(noisy, np.zeros_like(bw), np.zeros_like(occ))

    def sse(a):                                           # a[k] is frame k + 1
        return float(((a[3:].astype(np.float64) - clean[4:]) ** 2).sum())
    n, d, z = sse(noisy[1:]), sse(den), sse(still)
    print("sigma %d: noisy / denoised %.3f, zero-flow / denoised %.3f, t %s, M %s" % (sigma, n / d, z / d, stats[3:, 0].tolist(),
                                                                                    stats[3:, 1].tolist()))
    assert d <= n / 4, (n, d)
    assert d <= 0.8 * z, (z, d)
    assert set(stats[3:, 0].tolist()) == {{5: 2, 10: 3, 20: 4}[sigma]}
    # the occluded strip behind the square is FRESH in every pair: 16 rows of 3 pixels
    assert (stats[:, 3] == 48).all() and occ.sum(axis=(1, 2)).tolist() == [48] * 11


# ------------------------------------------------------------------------------------------------- the cases and the mutants
def _equal(a, b):
    return sorted(a[0]) == sorted(b[0]) and np.array_equal(a[1], b[1]) and \
        all(np.array_equal(a[0][i][k], b[0][i][k]) for i in a[0] for k in R.OUTPUTS)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_a_case(mutant):
    caught = []
    for cid in SMALL:
        case = BY_ID[cid]
        if not _equal(R.replay(case, case['state'], mutant), R.mirror_of(cid)):
            caught.append(cid)
            if len(caught) == 3:
                break
    print(mutant, caught)
    assert caught, mutant


def test_the_mutant_list_is_the_issues():
    assert set(R.MUTANTS) >= {'in_place', 'nearest_count', 'ignore_occ', 'hist_all', 'half_gt', 'no_round', 'trunc', 'inside_off',
                              'no_restart'}


def test_the_case_list_crosses_what_the_issue_lists():
    full = [c for _, c in CASES if c['pattern'] == 'full' and c['name'] in ('ragged', 'full') and c['tab'][8 * c['B'] + 9] <= c['Wmax']]
    for kind in R.FLOW_KINDS:
        mine = [c for c in full if c['kind'] == kind]
        assert {c['tol'] for c in mine} >= set(R.TOLS) and {c['u8'] for c in mine} == {False, True}
        assert {c['name'] for c in mine} == {'ragged', 'full'}
    assert {c['depth'] for c in full} == {1, 8, 64} and {c['occ_kind'] for c in full} == {'none', 'random', 'blobs'}
    assert R.RAGGED == dict(B=3, Hmax=40, Wmax=64, h=37, w=53)
    assert {(c['pattern'], c['u8']) for _, c in CASES} >= {(p, u) for p in ('first', 'nopairs', 'full', 'short', 'short2')
                                                           for u in (False, True)}
    short2 = next(c for _, c in CASES if c['pattern'] == 'short2')
    assert short2['valid'] == [0, 1] and short2['B'] == 3 and short2['k'] == 2
    over = next(c for _, c in CASES if 'over1' in c['id'])
    assert over['valid'] == [0, 2] and over['tab'][8 * over['B'] + 8 + 1] == over['Wmax'] + 1
    tiny = [c for _, c in CASES if c['name'] == 'tiny']
    assert {(c['h'], c['w']) for c in tiny} == {(1, 1)} and {c['carry'] > 0 for c in tiny} == {False, True}
    big = next(c for _, c in CASES if c['name'] == 'big')
    assert big['Hmax'] * big['Wmax'] > 2048 * 256         # csrc/common.h stream_grid's cap times the block
    wild = next(c for _, c in CASES if c['kind'] == 'wild')
    f = wild['flow_bw'][:, :wild['h'], :wild['w']]
    assert np.isnan(f).any() and np.isinf(f).any() and (np.abs(f[np.isfinite(f)]) >= 5000).any()
    # every d, both sources of a FRESH pixel and clamped taps occur often: a GPU test against this mirror cannot pass with one dead
    seen = np.zeros(7, np.int64)
    for cid in SMALL:
        case = BY_ID[cid]
        hist = case['state'].astype(np.int64)
        if case['carry'] == 0:
            hist = R.initial(hist, case['frames'][0], case['h'], case['w'], case['Hmax'], case['Wmax'])
        for i in case['valid'][:1]:
            h, w = case['h'], case['w']
            fresh, PX, PY = R._geometry(case['flow_bw'][i], case['occ'][i], h, w)
            pred, _ = R._predict(hist, PX, PY, h, w)
            cur = R.quant(np.ascontiguousarray(case['frames'][i][:h, :w]).astype(np.float32))
            t = int(R.mirror_of(cid)[0][i]['stats'][0])
            seen += np.bincount(np.minimum(np.abs(pred - cur).sum(axis=-1)[~fresh] >> (11 + t), 6), minlength=7)
    assert (seen > 100).all(), seen


def test_replay_patterns_and_the_state():
    """A first replay starts from its first frame whatever the state holds; a first replay without a pair leaves that initial
    history; a carried one continues from the state, and one without a pair leaves it alone."""
    first = next(c for _, c in CASES if c['pattern'] == 'first' and c['name'] == 'ragged')
    a = R.replay(first, first['state'])
    b = R.replay(first, np.zeros_like(first['state']))
    h, w = first['h'], first['w']
    assert first['carry'] == 0 and first['valid'] == [1, 2]
    assert sorted(a[0]) == sorted(b[0]) and all(np.array_equal(a[0][i][k], b[0][i][k]) for i in a[0] for k in R.OUTPUTS)
    assert np.array_equal(a[1][:h, :w], b[1][:h, :w]) and np.array_equal(a[1][h:], first['state'][h:])     # outside (h, w): untouched
    none = next(c for _, c in CASES if c['pattern'] == 'nopairs')
    outs, state = R.replay(none, none['state'])
    assert outs == {} and (state[:h, :w, 3] == 1).all() and np.array_equal(state[:, w:], none['state'][:, w:])
    assert np.array_equal(state[:h, :w, :3].astype(np.int64),
                          R.quant(np.ascontiguousarray(none['frames'][0][:h, :w]).astype(np.float32)))
    short = next(c for _, c in CASES if c['pattern'] == 'short')
    moved = R.replay(short, short['state'])
    assert short['carry'] > 0 and not _equal(moved, R.replay(short, np.ones_like(short['state'])))
    # two launches chained equal one launch over both (the state is all that is carried)
    full = next(c for _, c in CASES if c['pattern'] == 'full' and c['kind'] == 'iid12' and c['depth'] == 8)
    outs, state = R.replay(full, full['state'])
    one = dict(full, valid=[0])
    o1, s1 = R.replay(one, full['state'])
    hist = s1.astype(np.int64)
    for i in (1, 2):
        o, hist = R.denoise_pair(full['frames'][i], full['flow_bw'][i], full['occ'][i], full['h'], full['w'], full['tol'], full['depth'],
                                 hist)
        assert np.array_equal(o['den'], outs[i]['den'])
    assert np.array_equal(hist.astype(np.uint16), state)


def test_mirror_is_deterministic_and_leaves_its_inputs_alone():
    cid = SMALL[7]
    case = BY_ID[cid]
    before = {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}
    assert _equal(R.replay(case, case['state']), R.mirror_of(cid))
    assert all(np.array_equal(case[k], v, equal_nan=v.dtype.kind == 'f') for k, v in before.items())


# ------------------------------------------------------------------------------------------------- the host side
def test_table_rows_and_file_list_are_unchanged_without_the_keywords():
    from unflow_amd.core import inference as I
    import torch
    plain = I.output_buffers(2, 8, 16, 5, 3, True, held_out=True, stabilise=True)
    rows = I.output_buffers(2, 8, 16, 5, 3, True, held_out=True, stabilise=True, denoise=True)
    assert rows[:len(plain)] == plain and I.output_buffers(2, 8, 16) == I.output_buffers(2, 8, 16, denoise=False)
    assert not any(r[4] == 'denoise' for r in plain) and [r[0] for r in I.output_buffers(2, 8, 16, 5, 3, True, held_out=True)] == \
        [r[0] for r in plain if r[4] != 'stabilise']
    assert [tuple(r) for r in rows[len(plain):]] == [('den', 'out_den', (2, 8, 16, 3), torch.uint8, 'denoise'),
                                                     ('den_stats', 'out_den_stats', (2, 8), torch.int32, 'denoise')]
    assert I.FlowEstimator.DEN_WANT == tuple(r[0] for r in rows[len(plain):])
    base = I.pair_files(7, 'png', True, True, I.sequence_visual_files(7, True), track=True, mid=2, stab=True)
    files = I.pair_files(7, 'png', True, True, I.sequence_visual_files(7, True), track=True, mid=2, stab=True, den=True)
    assert files[:len(base)] == base and files[len(base):] == [('000007_den.png', ('png', 'den', 0))]
    assert I.pair_files(7, 'png', True, True, I.sequence_visual_files(7, True), track=True, mid=2, stab=True, den=False) == base
    assert I.pair_files(7, 'flo', den=True)[1:] == files[len(base):] and I.pair_files(7, 'flo') == [('000007_10.flo', ('flo', 'flow'))]
    assert I.filter_entries(I.pair_files(0, 'flo', den=True), [(1, 5, 6)], 2) == [('den', 1, 5, 6)]


def test_the_option_parser():
    from unflow_amd.core import inference as I
    assert I.denoise_option(None) is None and I.denoise_option(False) is None
    assert I.denoise_option(True) == dict(tol='auto', depth=8) == I.DENOISE_DEFAULTS
    assert I.denoise_option(dict(depth=64, tol=0)) == dict(tol=0, depth=64)
    assert I.denoise_option({}) == I.DENOISE_DEFAULTS and I.denoise_option(dict(tol='auto', depth=1)) == dict(tol='auto', depth=1)
    for bad in (1, 'yes', dict(tol=5), dict(tol=-1), dict(tol='automatic'), dict(depth=0), dict(depth=65), dict(depth='auto'),
                dict(tol=2.0), dict(tol=True), dict(iters=1), [2, 8]):
        with pytest.raises(ValueError, match="denoise"):
            I.denoise_option(bad)
    for seq in (False, True):
        with pytest.raises(ValueError, match="denoise.*along the backward flow.*sequence='bidirectional'"):
            I.FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), sequence=seq, denoise=True)
    with pytest.raises(ValueError, match="denoise\\['depth'\\]"):
        I.FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), sequence='bidirectional', denoise=dict(depth=100))
    with pytest.raises(ValueError, match="denoise\\['tol'\\] is 'auto' or an int in 0..4"):
        I.FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), sequence='bidirectional', denoise=dict(tol=7))


def test_the_command_line_checks_the_flags(capsys, tmp_path):
    from unflow_amd import sequence as S
    from unflow_amd.core.input import write_png_rgb8
    for k in range(2):
        write_png_rgb8(str(tmp_path / ("%d.png" % k)), np.zeros((4, 6, 3), np.uint8))
    a = S.parse_args(['--ex', 'x', '--frames', str(tmp_path), '--occlusion'])
    assert a.denoise is False and a.denoise_option is None
    a = S.parse_args(['--ex', 'x', '--frames', str(tmp_path), '--occlusion', '--denoise'])
    assert a.denoise_option is True
    a = S.parse_args(['--ex', 'x', '--frames', str(tmp_path), '--output_backward', '--denoise', '--denoise_tol', '3', '--denoise_depth', '16'])
    assert a.denoise_option == dict(tol=3, depth=16)
    a = S.parse_args(['--ex', 'x', '--frames', str(tmp_path), '--output_backward', '--denoise', '--denoise_tol', 'auto'])
    assert a.denoise_option == dict(tol='auto')
    for bad, msg in ((['--occlusion', '--denoise_tol', '2'], 'needs --denoise'), (['--occlusion', '--denoise_depth', '2'], 'needs --denoise'),
                     (['--occlusion', '--denoise', '--denoise_tol', '5'], 'auto or an integer in 0..4'),
                     (['--occlusion', '--denoise', '--denoise_tol', '-1'], None),
                     (['--occlusion', '--denoise', '--denoise_depth', '65'], '1..64'),
                     (['--occlusion', '--denoise', '--denoise_depth', '0'], '1..64'),
                     (['--denoise'], 'both directions along the clip; add --output_backward or --occlusion')):
        with pytest.raises(SystemExit) as err:
            S.parse_args(['--ex', 'x', '--frames', str(tmp_path)] + bad)
        assert err.value.code == 2, bad
        assert msg is None or msg in capsys.readouterr().err, bad


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from unflow_amd import _lib, build
    build.build()
    L = _lib.lib()
    one = ctypes.c_void_p(16)            # never dereferenced: the arguments are refused before anything is launched
    nul = ctypes.c_void_p(0)
    names = ('frames', 'tab', 'flow', 'occ', 'state', 'ws', 'den', 'stats')

    def call(B=2, Hm=40, Wm=64, tol=-1, depth=8, null=None, odd=None):
        p = {k: one for k in names}
        if null:
            p[null] = nul
        if odd:
            p[odd] = ctypes.c_void_p(20)
        return L.unflow_sequence_denoise(p['frames'], p['tab'], B, Hm, Wm, p['flow'], p['occ'], tol, depth, p['state'], p['ws'],
                                         p['den'], p['stats'], nul)
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(Hm=0), dict(Wm=0), dict(Hm=4097), dict(Wm=4097), dict(tol=-2), dict(tol=5),
               dict(depth=0), dict(depth=65), dict(depth=-8)):
        assert call(**kw) == -5, kw
    for name in names:
        assert call(null=name) == -1, name
    for name in ('state', 'ws', 'flow'):
        assert call(odd=name) == -7, name
    assert call(null='occ', B=0) == -1                                        # the NULL test comes first
    size = L.unflow_sequence_denoise_workspace_bytes
    assert size.restype is ctypes.c_size_t and L.unflow_sequence_denoise.restype is ctypes.c_int
    assert size(0, 8, 8) == 0 and size(65536, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 8, 4097) == 0
    assert size(3, 40, 64) == 3 * 256 * 4 + 2 * 40 * 64 * 8 and size(1, 4096, 4096) == 1024 + (1 << 28)


def test_the_symbol_is_declared_and_the_build_needs_no_change():
    import os
    from unflow_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'unflow_hip.h')) as f:
        header = f.read()
    assert 'int unflow_sequence_denoise(const void* frames, const int* tab, int B, int Hmax, int Wmax, const float* flow_bw,' in header
    assert 'size_t unflow_sequence_denoise_workspace_bytes(int B, int Hmax, int Wmax);' in header
    src = os.path.join(root, 'unflow_amd', 'csrc', 'denoise.hip')
    assert src in build.sources() and '-ffp-contract=off' in build.flags_for(src)
    with open(src) as f:
        text = f.read()
    assert 'asm' not in text and 'hipMemset' not in text and 'atomicAdd(float' not in text
    assert 'mid_q(' in text and 'rintf(fminf' not in text                     # one definition of the quantisation: mid_common.h's
