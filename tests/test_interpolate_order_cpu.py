"""CPU: the numpy mirror of unflow_sequence_interpolate_ordered (tests/mid_order_ref.py) proven without a GPU — order 0
is tests/mid_ref.py's definition on every one of its cases; the holes are the unordered definition's at every order; on the occluder
scene the ordered frames are within a derived bound of the rendered truth and two orders of magnitude closer to it than the
averaging ones; every mutant of the mirror is caught by the case list; both colour branches and every value of d are taken; and the
host-side checks of the option and of the entry point."""
import ctypes

import numpy as np
import pytest

import mid_order_ref as R
import mid_ref as M

CASES = R.entry_cases()
BY_ID = dict(CASES)
SMALL = [cid for cid, c in CASES if c['h'] * c['w'] < 10000]
# DESIGN 7.19's table: (n, both directions) -> the hole counts per j
SCENE_HOLES = {(1, False): [64], (1, True): [0], (3, False): [32, 64, 96], (3, True): [0, 0, 0]}
SCENE_MAX_ERR = 12


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]) for i in a)


@pytest.mark.parametrize("cid", [c for c, _ in M.entry_cases()])
def test_order_zero_is_the_unordered_definition(cid):
    case = dict(M.entry_cases())[cid]
    want, want_prev, want_stats = M.mirror_of(cid)
    got, prev, stats = R.replay(case, M.prev_of(case), order=0)
    assert _same(got, want) and np.array_equal(prev, want_prev)
    for i in want_stats:
        assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(stats[i], want_stats[i]))


@pytest.mark.parametrize("cid", SMALL)
def test_the_holes_are_the_unordered_definitions(cid):
    """The hole test is on the conf-less weight sum: the hole sets and the counts are the unordered definition's at every order.
    The weighted sums lie between the conf-less ones and 64 times them, and account for every kept tap."""
    case = BY_ID[cid]
    outs, _, stats = R.mirror_of(cid)
    plain, _, plain_stats = R.replay(case, M.prev_of(case), order=0)
    assert sorted(outs) == sorted(plain) == list(case['valid'])
    for i in outs:
        assert np.array_equal(outs[i][1], plain[i][1])
        for j, ((Sw, kept, hole), (Sw0, _, hole0)) in enumerate(zip(stats[i], plain_stats[i])):
            assert np.array_equal(hole, Sw0 < M.HOLE) and (Sw >= Sw0).all() and (Sw <= 64 * Sw0).all()
            assert int(Sw.sum()) == kept and int(hole.sum()) == outs[i][1][j]


@pytest.mark.parametrize("bidir", [False, True], ids=['fw', 'bidir'])
@pytest.mark.parametrize("n", [1, 3])
def test_the_occluder_scene_comes_out_ordered(n, bidir):
    """A bright square moving over a dark background, exact flows and masks, against the rendered truth.  The bound on the error:
    where two layers collide in a target the winner is there at conf 64 and the loser at conf 1, with direction weights of at most
    1 : 3 against the winner, so the quotient is off the winner's colour by at most 255 * 3 / 67 < 11.5, plus the roundings: 12.
    The averaging definition is off by a sizeable part of the 128 grey levels between the layers on every such pixel."""
    for k in (1, 2, 3, 4):
        sse, worst, holes = R.scene_scores(n, bidir, k)
        sse0, worst0, holes0 = R.scene_scores(n, bidir, 0)
        print("n = %d, %s, k = %d: SSE %d -> %d, max error %d -> %d, holes %s" % (n, 'both' if bidir else 'one', k, sse0, sse, worst0,
                                                                                  worst, holes))
        assert worst <= SCENE_MAX_ERR
        assert sse * 100 < sse0
        assert holes == SCENE_HOLES[(n, bidir)] and holes0 == holes


def _caught(mutant, cid):
    case = BY_ID[cid]
    return not _same(R.mirror_of(cid)[0], R.replay(case, M.prev_of(case), mutant=mutant)[0])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_a_case(mutant):
    caught = [cid for cid in SMALL if _caught(mutant, cid)]
    print(mutant, len(caught), caught[:4])
    assert caught, mutant


def test_both_colour_branches_and_every_d_are_taken():
    """Over the case list at least 100 source pixels blended, 100 unblended (at the floor, and masked), and 100 at every value of
    d, 0..6, so that a GPU test against this mirror cannot pass with one of them dead."""
    tally = {}
    for cid in SMALL:
        case = BY_ID[cid]
        R.replay(case, M.prev_of(case), tally=tally)
    print(tally)
    assert tally['blended'] >= 100 and tally['unblended'] >= 100 and tally['masked'] >= 100
    assert len(tally['d']) == R.FLOOR + 1 and (tally['d'] >= 100).all()
    assert tally['unblended'] == tally['masked'] + tally['d'][R.FLOOR]


def test_a_nan_colour_ends_as_the_definition_says():
    """A NaN in either frame gives e = 765: the pixel is at the floor at every order, keeps its own colour, and a NaN colour is
    quantised to 0 — no NaN reaches an integer conversion."""
    cid = [c for c in SMALL if c.startswith('nan-')][0]
    case = BY_ID[cid]
    assert np.isnan(case['frames'][:, :case['h'], :case['w']]).any() and np.isnan(case['prev']).any()
    tally = {}
    outs = R.replay(case, M.prev_of(case), tally=tally)[0]
    assert sorted(outs) == list(case['valid']) and tally['d'][R.FLOOR] > 0


def test_mirror_is_deterministic_and_leaves_its_inputs_alone():
    cid = 'ragged-n1-u8-fw-iid12-full-k2'
    case = BY_ID[cid]
    before = {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}
    a, pa, _ = R.replay(case, M.prev_of(case))
    b, pb, _ = R.mirror_of(cid)
    assert _same(a, b) and np.array_equal(pa, pb)
    assert all(np.array_equal(v, case[k], equal_nan=v.dtype.kind == 'f') for k, v in before.items())


# ------------------------------------------------------------------------------------------------- host side
def test_the_option_parser():
    from unflow_amd.core import inference as I
    assert I.interpolate_order_option(None) == 0 and I.interpolate_order_option(0) == 0 and I.interpolate_order_option(None, 0) == 0
    assert I.interpolate_order_option(0, 0) == 0
    assert [I.interpolate_order_option(k, 3) for k in (1, 2, 3, 4, np.int64(2))] == [1, 2, 3, 4, 2]
    for bad in (5, -1, True, False, 2.0, '2', (1,)):
        with pytest.raises(ValueError, match="interpolate_order"):
            I.interpolate_order_option(bad, 3)
    with pytest.raises(ValueError, match="interpolate_order.*needs interpolate"):
        I.interpolate_order_option(2, 0)
    # no new rows: the tables are what they were
    assert I.output_buffers(2, 8, 16, 5, 3) == I.output_buffers(2, 8, 16, 5, n_mid=3)
    assert [r[0] for r in I.output_buffers(2, 8, 16, 5, 3)[-2:]] == ['mid', 'mid_holes']


def test_the_command_line_checks_order():
    from unflow_amd import sequence as S
    ap = S.parser()
    assert ap.parse_args(['--ex', 'x', '--frames', 'd']).order is None
    assert ap.parse_args(['--ex', 'x', '--frames', 'd', '--interpolate', '2', '--order', '3']).order == 3
    for argv in (['--interpolate', '1', '--order', '0'], ['--interpolate', '1', '--order', '5'], ['--order', '2']):
        with pytest.raises(SystemExit) as ex:
            S.parse_args(['--ex', 'x', '--frames', 'no-such-folder'] + argv)
        assert ex.value.code == 2


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from unflow_amd import _lib, build
    build.build()
    L = _lib.lib()
    one = ctypes.c_void_p(16)            # never dereferenced: the arguments are refused before anything is launched
    nul = ctypes.c_void_p(0)

    def call(order, n=1, B=1, Hmax=4, Wmax=4, bw=nul, ofw=nul, obw=nul, frames=one):
        return L.unflow_sequence_interpolate_ordered(frames, one, B, Hmax, Wmax, n, one, bw, ofw, obw, one, one, one, one, order, nul)
    assert call(-1) == -5 and call(5) == -5 and call(-1, frames=nul) == -5
    for order in (0, 1, 4):
        assert call(order, n=0) == -5 and call(order, n=8) == -5 and call(order, B=0) == -5
        assert call(order, bw=one) == -5 and call(order, ofw=one, obw=one) == -5
        assert call(order, frames=nul) == -1
    # 2^23 + 1 pixels: refused at order 1, before the NULL checks; at order 0 the shape passes and the NULL check is reached
    assert (1 << 23) + 1 == 3 * 2796203
    assert call(1, Hmax=3, Wmax=2796203, frames=nul) == -5 and call(4, Hmax=2796203, Wmax=3) == -5
    assert call(0, Hmax=3, Wmax=2796203, frames=nul) == -1
    assert call(1, Hmax=2048, Wmax=4096, frames=nul) == -1 and call(1, Hmax=2160, Wmax=3840, frames=nul) == -1


def test_the_symbol_is_declared_exported_and_bound():
    import os
    from unflow_amd import _lib, build
    build.build()
    L = _lib.lib()
    fn = L.unflow_sequence_interpolate_ordered
    assert fn.restype is ctypes.c_int
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'unflow_hip.h')) as f:
        header = f.read()
    assert 'int unflow_sequence_interpolate_ordered(const void* frames, const int* tab,' in header
    decl = header[header.index('int unflow_sequence_interpolate_ordered('):]
    assert 'int order, unflow_stream_t stream);' in decl[:decl.index(';') + 1]
