"""CPU: the numpy mirror of unflow_sequence_interpolate (tests/mid_ref.py) proven without a GPU — a translated frame
comes out translated by half, bit for bit; the weight sums account for every kept tap; every mutant of the mirror is caught by the
case list; both branches of the normalisation are taken; and the host-side checks of the option and the entry point."""
import ctypes

import numpy as np
import pytest

import mid_ref as M

CASES = M.entry_cases()
BY_ID = dict(CASES)
SMALL = [cid for cid, c in CASES if c['name'] == 'ragged']


@pytest.mark.parametrize("bidir", [False, True])
def test_translation_gives_the_half_shifted_frame_bit_for_bit(bidir):
    """const flow STEP = (4, -2), n = 1, uint8: the in-between frame is frame 0 moved by (2, -1) wherever that pixel is inside the
    frame in both frames (the interior: there the warped other frame is the pixel itself, not a clamped edge) — both directions
    agree on it, occluded or not."""
    case = M.make_case('translation', n=1, u8=True, bidir=bidir, kind='const', pattern='full', **M.RAGGED)
    outs, _, _ = M.replay(case, M.prev_of(case))
    h, w = case['h'], case['w']
    sx, sy = M.STEP
    assert sx > 0 > sy and sx % 2 == 0 and sy % 2 == 0
    hx, hy = sx // 2, sy // 2
    for i in case['valid']:
        im0 = (case['prev'] if i == 0 else case['frames'][i - 1])[:h, :w]
        mid = outs[i][0][0]
        # target (x, y) = source (x - hx, y - hy), the source with x < w - sx and y >= -sy
        assert np.array_equal(mid[-hy:h + hy, hx:w - hx], im0[-sy:, :w - sx]), i
        if not bidir:                                  # one direction: exactly the uncovered border is holes
            assert outs[i][1][0] == h * w - (h + hy) * (w - hx)


@pytest.mark.parametrize("cid", SMALL)
def test_weight_sums_equal_the_kept_taps(cid):
    _, _, stats = M.mirror_of(cid)
    for i, per_j in stats.items():
        for Sw, kept in per_j:
            assert int(Sw.sum()) == kept and (Sw >= 0).all()


def test_both_branches_of_the_normalisation_are_taken():
    """Over the case list at least 100 hole pixels and 100 normalised pixels (in fact on several single cases), so that a GPU test
    against this mirror cannot pass with the hole path dead."""
    holes = full = 0
    for cid in SMALL:
        case = BY_ID[cid]
        outs, _, _ = M.mirror_of(cid)
        for mid, hl in outs.values():
            holes += int(hl.sum())
            full += case['n'] * case['h'] * case['w'] - int(hl.sum())
    assert holes >= 100 and full >= 100, (holes, full)
    for cid in ('ragged-n1-u8-fw-const-full', 'ragged-n1-u8-fw-iid12-full'):
        outs, _, _ = M.mirror_of(cid)
        assert sum(int(hl.sum()) for _, hl in outs.values()) >= 100, cid


def _two_replays(case, mutant):
    """A first replay of the clip and a carried one behind it, prev handed from the one to the other."""
    first = M.make_case('chain', n=case['n'], u8=case['u8'], bidir=case['bidir'], kind=case['kind'], pattern='first', **M.RAGGED)
    _, prev, _ = M.replay(first, None, mutant)
    outs, _, _ = M.replay(case, prev, mutant)
    return outs


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_fails_a_case(mutant):
    caught = []
    for cid in SMALL:
        case = BY_ID[cid]
        if mutant == 'prev_slot0':
            if case['pattern'] != 'full' or case['kind'] != 'smooth':
                continue
            good, bad = _two_replays(case, None), _two_replays(case, mutant)
        else:
            good, bad = M.mirror_of(cid)[0], M.replay(case, M.prev_of(case), mutant)[0]
        if any(not np.array_equal(good[i][0], bad[i][0]) or not np.array_equal(good[i][1], bad[i][1]) for i in good):
            caught.append(cid)
    print(mutant, len(caught), caught[:4])
    assert caught, mutant


def test_mirror_is_deterministic_and_leaves_its_inputs_alone():
    cid = 'ragged-n1-u8-fw-iid12-full'
    case = BY_ID[cid]
    before = {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}
    a, pa, _ = M.replay(case, M.prev_of(case))
    b, pb, _ = M.mirror_of(cid)
    assert all(np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]) for i in a) and np.array_equal(pa, pb)
    assert all(np.array_equal(v, case[k], equal_nan=v.dtype.kind == 'f') for k, v in before.items())


def test_hole_shares_of_the_flow_kinds():
    """The hole shares stay where the definition was sized: a few per cent on a smooth field, about a tenth for i.i.d. +-12 px in
    one direction and far less in both, the uncovered border for the translation."""
    share = {}
    for cid in SMALL:
        case = BY_ID[cid]
        if case['pattern'] != 'full' or case['n'] != 1:
            continue
        outs, _, _ = M.mirror_of(cid)
        share[(case['kind'], case['bidir'])] = sum(int(hl.sum()) for _, hl in outs.values()) / (len(outs) * case['h'] * case['w'])
    print(share)
    assert share[('smooth', False)] < 0.10 and share[('smooth', True)] < 0.10
    assert 0.05 < share[('iid12', False)] < 0.30 and share[('iid12', True)] < share[('iid12', False)] / 2
    assert abs(share[('const', False)] - (1 - (37 - 1) * (53 - 2) / (37 * 53))) < 1e-9


# ------------------------------------------------------------------------------------------------- host side
def test_option_and_table_rows():
    from unflow_amd.core import inference as I
    plain, rows = I.output_buffers(2, 8, 16, 5), I.output_buffers(2, 8, 16, 5, 3)
    assert rows[:-2] == plain[:-2] and len(rows) == len(plain)              # rows of the existing table keep their order
    assert [r[0] for r in rows[:-2]] == ['flow', 'u16', 'sums', 'counts', 'flow_bw', 'u16_bw', 'occ', 'occ_counts', 'vis',
                                         'track_disp', 'track_alive']
    extra = rows[-2:]
    assert [(r[0], r[2], r[4]) for r in extra] == [('mid', (3, 2, 8, 16, 3), 'interpolate'), ('mid_holes', (3, 2), 'interpolate')]
    assert I.interpolate_option(None) == 0 and I.interpolate_option(False) == 0 and I.interpolate_option(3) == 3
    for bad in (0, 8, -1, True, 1.0, '2'):
        with pytest.raises(ValueError):
            I.interpolate_option(bad)
    files = I.pair_files(7, 'png', backward=True, occlusion=True, mid=2)
    assert [f for f, _ in files] == ['000007_10.png', '000007_01.png', '000007_10_occ.png', '000007_mid1.png', '000007_mid2.png']
    assert files[-2:] == [('000007_mid1.png', ('png', 'mid', 0)), ('000007_mid2.png', ('png', 'mid', 1))]
    assert I.pair_files(7, 'png') == I.pair_files(7, 'png', mid=0)
    assert I.filter_entries(files, [(1, 5, 6)], 4)[-2:] == [('mid', 1, 5, 6), ('mid', 5, 5, 6)]


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from unflow_amd import _lib, build
    build.build()
    L = _lib.lib()
    one = ctypes.c_void_p(16)            # never dereferenced: the arguments are refused before anything is launched
    nul = ctypes.c_void_p(0)

    def call(n=1, B=1, Hmax=4, Wmax=4, bw=nul, ofw=nul, obw=nul, frames=one):
        return L.unflow_sequence_interpolate(frames, one, B, Hmax, Wmax, n, one, bw, ofw, obw, one, one, one, one, nul)
    assert call(n=0) == -5 and call(n=8) == -5 and call(B=0) == -5
    assert call(Hmax=1 << 16, Wmax=1 << 15) == -5
    assert call(bw=one) == -5 and call(bw=one, ofw=one) == -5 and call(ofw=one, obw=one) == -5
    assert call(frames=nul) == -1
    ws = L.unflow_sequence_interpolate_workspace_bytes
    assert ws(3, 2, 40, 64) == 3 * 2 * 40 * 64 * 32 and ws(0, 2, 40, 64) == 0 and ws(8, 2, 40, 64) == 0
