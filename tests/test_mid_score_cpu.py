"""CPU: the numpy mirror of unflow_sequence_interpolate_score (tests/mid_score_ref.py) proven without a GPU — hand
cases, a condition on a translated texture, coverage of the case list, every mutant of the mirror caught by a case — and the
host-side checks: the table word, the output table, the option, the entry's refusals and the command's flags."""
import ctypes

import numpy as np
import pytest

import mid_ref as M
import mid_score_ref as R

CASES = R.entry_cases()
BY_ID = dict(CASES)
SMALL = [cid for cid, c in CASES if c['name'] != 'past-the-cap']


# ------------------------------------------------------------------------------------------------- hand cases
def _bytes(rs, h, w, lo=0, hi=256):
    return rs.randint(lo, hi, size=(h, w, 3)).astype(np.uint8)


def test_truth_equal_to_the_candidate_gives_zero_error_and_ssim_one_in_every_window():
    rs = np.random.RandomState(1)
    h, w = 19, 23
    im0, im1, mid = _bytes(rs, h, w), _bytes(rs, h, w), _bytes(rs, h, w)
    s = R.ssim_terms(mid.astype(np.int64), mid.astype(np.int64))
    assert s.shape == (h - 7, w - 7, 3) and (s == 1.0).all()
    sse, ssim, mag = R.score_pair(im0, im1, mid[None], mid[None], h, w, 1)
    assert sse[0, 0] == 0 and ssim[0, 0] == 3 * (h - 7) * (w - 7) == R.windows(h, w) * 3 and mag[0, 0] == ssim[0, 0]
    assert sse[0, 1] > 0 and sse[0, 2] > 0 and ssim[0, 1] < ssim[0, 0]


@pytest.mark.parametrize("d", [1, 5, -7])
def test_a_constant_offset_gives_3hw_d_squared(d):
    rs = np.random.RandomState(2)
    h, w = 11, 30
    mid = _bytes(rs, h, w, 10, 240)
    truth = (mid.astype(np.int64) + d).astype(np.uint8)
    sse, _, _ = R.score_pair(mid, mid, mid[None], truth[None], h, w, 1)
    assert sse[0].tolist() == [3 * h * w * d * d] * 3          # im0 = im1 = mid: blend and nearest are mid too


def test_the_nearest_frame_at_the_tie_is_im0_and_blend_is_weighted_towards_the_nearer_frame():
    rs = np.random.RandomState(3)
    h, w = 8, 9
    im0, im1 = _bytes(rs, h, w), _bytes(rs, h, w)
    for n in (1, 3, 5):
        for j in range(1, n + 1):
            _, blend, near = R.candidates(im0, im1, im0, n, j)
            assert np.array_equal(near, im0 if 2 * j <= n + 1 else im1), (n, j)
            a, b = im0.astype(np.int64), im1.astype(np.int64)
            assert np.array_equal(blend, ((n + 1 - j) * 256 * a + j * 256 * b + 128 * (n + 1)) // (256 * (n + 1)))
    assert np.array_equal(R.candidates(im0, im1, im0, 3, 2)[2], im0)            # 2 j = n + 1
    # fp32: the byte is (q + 128) / 256, NaN is 0, values outside [0, 255] are clamped
    v = np.array([[[np.nan, -4.0, 300.0], [254.5, 0.498, 0.5]]], np.float32)
    assert R.byte_of(v).tolist() == [[[0, 0, 255], [255, 0, 1]]]


def test_blend_is_the_value_a_hole_gets_from_the_interpolation():
    """mid_ref's own holes (the border a one-direction translation uncovers, and those of the torn flow): there out_mid IS the
    blend candidate."""
    seen = 0
    for cid in ('ragged-n1-u8-fw-const-full', 'ragged-n3-f32-fw-iid12-full'):
        case = dict(M.entry_cases())[cid]
        outs, _, stats = M.mirror_of(cid)
        h, w, n = case['h'], case['w'], case['n']
        for i in case['valid']:
            im0 = (case['prev'] if i == 0 else case['frames'][i - 1])[:h, :w]
            for j in range(1, n + 1):
                hole = stats[i][j - 1][0] < M.HOLE
                blend = R.candidates(im0, case['frames'][i][:h, :w], outs[i][0][j - 1], n, j)[1]
                assert hole.sum() == outs[i][1][j - 1] and np.array_equal(blend[hole], outs[i][0][j - 1][hole])
                seen += int(hole.sum())
    assert seen > 100


# ------------------------------------------------------------------------------------------------- a condition on the reference alone
@pytest.mark.parametrize("cid", ['ragged-n1-u8-full-texture', 'ragged-n1-f32-full-texture', 'ragged-n3-u8-full-texture'])
def test_motion_compensation_beats_the_blend_on_a_translated_texture(cid):
    """A random texture translated by an even constant flow, the in-between frames mid_ref's on that flow, the truths the texture
    at the in-between positions: the interpolated frame is closer to the truth than the blend of two unrelated textures, by both
    measures, in every slot and at every j.  No margin is fixed."""
    case = BY_ID[cid]
    assert case['truth'].shape == case['true'].shape
    for i, (sse, ssim, _) in R.mirror_of(cid)[0].items():
        assert (sse[:, 0] < sse[:, 1]).all() and (ssim[:, 0] > ssim[:, 1]).all(), (i, sse, ssim)
        assert (sse[:, 0] < sse[:, 2]).all() and (ssim[:, 0] > ssim[:, 2]).all(), (i, sse, ssim)


# ------------------------------------------------------------------------------------------------- coverage and mutants
def test_the_cases_cover_every_kind_windows_and_their_absence():
    kinds_nonzero = np.zeros(3, bool)
    with_windows = without = unheld = unscored = 0
    dtypes, ns = set(), set()
    for cid in SMALL:
        case = BY_ID[cid]
        outs, _ = R.mirror_of(cid)
        dtypes.add(case['u8'])
        ns.add(case['n'])
        unheld += len(case['valid']) - len(case['scored'])
        unscored += case['B'] - len(case['valid'])
        for sse, ssim, mag in outs.values():
            kinds_nonzero |= (sse > 0).any(0)
            if R.windows(case['h'], case['w']):
                with_windows += 1
                assert (mag > 0).all()
            else:
                without += 1
                assert (ssim == 0).all() and (mag == 0).all() and (sse > 0).any()
    assert kinds_nonzero.all() and with_windows and without and unheld and unscored and dtypes == {True, False} and ns == {1, 3}
    assert R.windows(9, 11) == 8 and R.windows(8, 8) == 1 and R.windows(7, 20) == 0
    big = BY_ID['past-the-cap-n1-u8-full-texture']
    assert -(-big['w'] // R.TILE_X) * -(-big['h'] // R.TILE_Y) > R.CAP              # more tiles than blocks: the grid-stride loop
    fp = BY_ID['ragged-n3-f32-full-noise'] if 'ragged-n3-f32-full-noise' in BY_ID else BY_ID['ragged-n1-f32-full-noise']
    assert np.isnan(fp['truth']).any() and np.isnan(np.concatenate([fp['prev'][None], fp['frames']])).any()
    assert (fp['truth'][np.isfinite(fp['truth'])] > 255).any() and (fp['truth'][np.isfinite(fp['truth'])] < 0).any()


def _two_replays(case, mutant):
    """A first replay of the clip and a carried one behind it, prev handed from the one to the other."""
    first = R.make_case('chain', n=case['n'], u8=case['u8'], pattern='first', truth=case['truth_kind'], **M.RAGGED)
    _, prev = R.replay(first, None, mutant)
    return R.replay(case, prev, mutant)[0]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_a_case(mutant):
    caught = []
    for cid in SMALL:
        case = BY_ID[cid]
        if mutant == 'prev_slot0':
            if case['name'] != 'ragged' or case['pattern'] != 'full' or 0 not in case['scored']:
                continue
            case = dict(case, truth_kind=cid.split('-')[4])
            good, bad = _two_replays(case, None), _two_replays(case, mutant)
        else:
            good, bad = R.mirror_of(cid)[0], R.replay(case, R.prev_of(case), mutant)[0]
        if any(not np.array_equal(good[i][0], bad[i][0]) or not np.array_equal(good[i][1], bad[i][1]) for i in good):
            caught.append(cid)
    print(mutant, len(caught), caught[:4])
    assert caught, mutant


def test_mirror_leaves_its_inputs_alone_and_the_bound_is_small():
    cid = 'ragged-n3-u8-full-noise'
    case = BY_ID[cid]
    before = {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}
    a, pa = R.replay(case, R.prev_of(case))
    b, pb = R.mirror_of(cid)
    assert all(np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]) for i in a) and np.array_equal(pa, pb)
    assert all(np.array_equal(v, case[k]) for k, v in before.items())
    assert R.sum_depth(case) == 6 + 6 + 3 + 1 + 1 + 6
    assert R.sum_depth(BY_ID['past-the-cap-n1-u8-full-texture']) == 6 + 6 + 3 + 3 + 8 + 6
    assert all((R.ssim_bound(case, mag) < 1e-10).all() for _, _, mag in a.values())


# ------------------------------------------------------------------------------------------------- host side
def test_the_table_word_and_the_output_rows():
    from unflow_amd.core import inference as I
    plain, _, _ = I.sequence_tables((5, 6), 2, 3, 3, u8=True, nmaps=2)
    held, valid, _ = I.sequence_tables((5, 6), 2, 3, 3, u8=True, nmaps=2, held=1)
    assert valid == [0, 1] and np.array_equal(I.sequence_tables((5, 6), 2, 3, 3, u8=True, nmaps=2, held=0)[0], plain)
    diff = np.flatnonzero(plain != held)
    assert diff.tolist() == [8 * 3 + 6, 8 * 3 + 8 + 6] and (held[diff] == 1).all() and (plain[6::8] == 0).all()
    rows, more = I.output_buffers(2, 8, 16, 5, 3, True), I.output_buffers(2, 8, 16, 5, 3, True, held_out=True)
    assert more[:-2] == rows and I.output_buffers(2, 8, 16, 5, 3, True, held_out=False) == rows
    assert [(r[0], r[1], r[2], r[4]) for r in more[-2:]] == [('mid_sse', 'out_mid_sse', (3, 2, 3), 'held_out'),
                                                             ('mid_ssim', 'out_mid_ssim', (3, 2, 3), 'held_out')]
    assert I.output_buffers(2, 8, 16, 5, 3, held_out=True)[:-2] == I.output_buffers(2, 8, 16, 5, 3)
    assert I.MID_KINDS == R.KINDS and I.mid_windows(9, 11) == 3 * 8 and I.mid_windows(7, 20) == 0
    assert I.mid_psnr(0, 10) == np.inf and abs(float(I.mid_psnr(3 * 255 ** 2, 3)) - 0.0) < 1e-12
    assert np.isnan(I.mid_mean_ssim(np.zeros(3), 0)).all() and I.mid_mean_ssim(np.array([6.0]), 24)[0] == 0.25


def test_the_option_is_checked_before_anything_is_built():
    from unflow_amd.core.inference import FlowEstimator
    for kw in (dict(sequence=True), dict(sequence='bidirectional'), dict()):
        with pytest.raises(ValueError, match="held_out.*interpolate=n"):
            FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), held_out=True, **kw)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from unflow_amd import _lib, build
    build.build()
    L = _lib.lib()
    one = ctypes.c_void_p(16)            # never dereferenced: the arguments are refused before anything is launched
    nul = ctypes.c_void_p(0)

    def call(n=1, B=1, Hmax=4, Wmax=4, **kw):
        a = dict(frames=one, tab=one, out_mid=one, truth=one, prev=one, ws=one, sse=one, ssim=one)
        a.update(kw)
        return L.unflow_sequence_interpolate_score(a['frames'], a['tab'], B, Hmax, Wmax, n, a['out_mid'], a['truth'], a['prev'],
                                                   a['ws'], a['sse'], a['ssim'], nul)
    assert call(n=0) == -5 and call(n=8) == -5 and call(B=0) == -5 and call(B=65536) == -5 and call(Hmax=0) == -5
    assert call(Hmax=1 << 16, Wmax=1 << 15) == -5
    for name in ('frames', 'tab', 'out_mid', 'truth', 'prev', 'ws', 'sse', 'ssim'):
        assert call(**{name: nul}) == -1, name
    ws = L.unflow_sequence_interpolate_score_workspace_bytes
    assert ws(3, 2, 40, 64) == 2 * (7 * 3 * (R.CAP + 1) * 8 + 8) and ws(3, 2, 40, 64) % 8 == 0
    assert ws(0, 2, 40, 64) == 0 and ws(8, 2, 40, 64) == 0 and ws(1, 0, 40, 64) == 0 and ws(1, 1, 1 << 16, 1 << 15) == 0


def test_the_command_line_flags(tmp_path, capsys):
    from unflow_amd import sequence as S
    from unflow_amd.core.input import write_png_rgb8
    rs = np.random.RandomState(0)
    for i in range(8):
        write_png_rgb8(str(tmp_path / ("f%03d.png" % i)), rs.randint(0, 256, size=(9, 12, 3)).astype(np.uint8))
    base = ['--ex', 'x', '--frames', str(tmp_path)]
    with pytest.raises(SystemExit) as err:
        S.parse_args(base + ['--held_out'])
    assert err.value.code == 2 and '--held_out' in capsys.readouterr().err and '--interpolate' in S.__doc__
    a = S.parse_args(base + ['--interpolate', '2', '--held_out'])
    assert a.held_out and len(a.full_rate) == 7 and a.dropped == 1 and [f[-8:] for f in a.files] == ['f000.png', 'f003.png', 'f006.png']
    a = S.parse_args(base + ['--interpolate', '6', '--held_out'])
    assert len(a.full_rate) == 8 and a.dropped == 0 and len(a.files) == 2
    with pytest.raises(SystemExit):
        S.parse_args(base + ['--interpolate', '7', '--held_out'])             # 8 frames hold no pair with 7 held-out frames
    a = S.parse_args(base + ['--interpolate', '2'])
    assert not a.held_out and a.full_rate is None and len(a.files) == 8
    scores = {'holes': 0.25, 'holes_j': [0.25, 0.25]}
    for k, kind in enumerate(R.KINDS):
        scores.update({'psnr/' + kind: 30.0 + k, 'ssim/' + kind: 0.9 - k / 10, 'psnr_j/' + kind: [30.0, 31.0], 'ssim_j/' + kind: [0.5, 0.6]})
    lines = S.held_out_table(scores, 2)
    assert [ln.split()[0] for ln in lines[1:]] == ['mid', 'blend', 'nearest', 'holes'] and '31.0000' in lines[2] and '25.0000 %' in lines[4]
