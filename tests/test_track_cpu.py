"""Tracks along a clip without a GPU: the numpy definition of tests/track_ref.py — its fp32 yardstick against its
fp64 mirror, hand cases, and mutants of the mirror against the comparator the GPU test uses — the table words, the option's
validation, the error messages, the C entry's declaration and argument errors, and the command line's flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import track_ref as T
import warp_parity as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.entry_cases()
BY_ID = dict(CASES)


@pytest.fixture(scope="module")
def lib():
    from unflow_amd import build, _lib
    build.build()
    return _lib.lib()


def _seed(case, state):
    N = case['N']
    return state if case['carry'] else (np.zeros((N, 2), np.float32), np.ones(N, bool))


# ------------------------------------------------------------------------------------------------- 1. yardstick vs mirror
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_yardstick_within_the_floor_of_the_mirror(cid):
    """Step by step along the yardstick's own chain: the fp32 step and the fp64 step from the same fp32 seed agree in every flag,
    and the fp32 displacement is within warp_parity's floor (1e-6 of the tensor's max) of the fp64 one — so the GPU test's bound,
    max(floor, 2 x this distance), is the floor on these cases.  The chain then passes the GPU test's comparator."""
    case = BY_ID[cid]
    state = T.draw_state(case)
    outs, new_state = T.replay(case, state)
    seed = _seed(case, state)
    worst = 0.0
    for i in case['valid']:
        args = (seed[0], seed[1], case['anchors'], case['flow'][i], None if case['occ'] is None else case['occ'][i],
                case['h'], case['w'])
        mir, mir_a = T.step(*args, np.float64, frame_disp=outs[i][0])
        yar, yar_a = T.step(*args, np.float32, frame_disp=outs[i][0])
        assert np.array_equal(mir_a, yar_a) and np.array_equal(yar_a, outs[i][1])
        assert np.array_equal(yar.view(np.int32), outs[i][0].view(np.int32))
        near = np.isfinite(mir) & (np.abs(mir) < T.LIMIT)
        if near.any():
            _, own = WP.bound_of(torch.from_numpy(yar[near].astype(np.float64)), torch.from_numpy(mir[near]))
            worst = max(worst, own)
        seed = outs[i]
    print("%s: the yardstick's distance from the mirror %.3g (floor %.3g)" % (cid, worst, WP.FLOOR))
    assert worst <= WP.FLOOR
    assert T.check_replay(case, state, outs, new_state) <= 0.5 + 1e-9


# ------------------------------------------------------------------------------------------------- 2. hand cases
def _dense_case(B, h, w, flow, occ=None, Hmax=None, Wmax=None, S=1, carry=0):
    """A launch over B valid slots written out by hand (not sequence_tables' patterns): every slot a pair."""
    Hmax, Wmax = Hmax or h, Wmax or w
    f = np.full((B, Hmax, Wmax, 2), np.nan, np.float32)
    f[:, :h, :w] = flow
    o = None
    if occ is not None:
        o = np.ones((B, Hmax, Wmax), np.uint8)
        o[:, :h, :w] = occ
    pts = T.grid_anchors(h, w, S)
    return dict(B=B, Hmax=Hmax, Wmax=Wmax, h=h, w=w, S=S, N=len(pts), anchors=pts, carry=carry, valid=list(range(B)), flow=f,
                occ=o)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_zero_flow_keeps_every_track_where_it_is(dt):
    case = _dense_case(3, 7, 10, 0.0, Hmax=9, Wmax=11)
    outs, (disp, alive) = T.replay(case, None, dt)
    for i in range(3):
        assert (outs[i][0] == 0).all() and outs[i][1].all()
    assert (disp == 0).all() and alive.all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_constant_flow_is_exact_and_tracks_die_at_the_step_they_leave(dt):
    B, h, w = 3, 7, 10
    case = _dense_case(B, h, w, np.asarray((2.0, -1.0), np.float32), Hmax=9, Wmax=11)
    outs, _ = T.replay(case, None, dt)
    x, y = case['anchors'][:, 0], case['anchors'][:, 1]
    died = np.full(case['N'], B + 1)                       # the step (1-based) at which x + 2t, y - t leaves [0, w-1] x [0, h-1]
    for t in range(B, 0, -1):
        out = (x + 2 * t > w - 1) | (y - t < 0)
        died[out] = t
    assert set(died) == {1, 2, 3, B + 1}
    for i in range(B):
        t = i + 1
        disp, alive = outs[i]
        assert np.array_equal(alive, died > t)
        frozen = np.minimum(t, died)                       # a dead track keeps the displacement of the step that took it out
        assert np.array_equal(disp, np.stack([2.0 * frozen, -1.0 * frozen], axis=1).astype(np.float32))


def test_a_track_landing_exactly_on_the_last_column_stays_alive():
    h, w = 4, 6
    flow = np.zeros((1, h, w, 2), np.float32)
    flow[0, :, 2] = (3.0, 0.0)            # x = 2 -> 5 = w - 1 exactly: alive
    flow[0, :, 3] = (2.25, 0.0)           # x = 3 -> 5.25: outside
    flow[0, :, 1] = (3.999, 0.0)          # x = 1 -> 4.999: inside
    flow[0, 1, 0] = (0.0, 2.0)            # y = 1 -> 3 = h - 1 exactly: alive
    flow[0, 2, 0] = (0.0, 1.5)            # y = 2 -> 3.5: outside
    case = _dense_case(1, h, w, flow)
    outs, _ = T.replay(case, None)
    alive = outs[0][1].reshape(h, w)
    assert alive[:, 2].all() and not alive[:, 3].any() and alive[:, 1].all()
    assert alive[1, 0] and not alive[2, 0] and alive[0, 0]
    assert np.array_equal(outs[0][0].reshape(h, w, 2)[0, 3], np.float32((2.25, 0.0)))     # the disp it left with
    # the bound is w - 1, not w: the mutant keeps the track at 5.25 alive
    assert T.replay(case, None, mutant='bound_w')[0][0][1].reshape(h, w)[:, 3].all()


def test_one_occluded_pixel_kills_exactly_the_tracks_with_a_weighted_tap_on_it():
    h, w = 6, 8
    flow = np.zeros((2, h, w, 2), np.float32)
    flow[0, ..., 0] = 0.5                 # slot 0: everything half a pixel to the right
    occ = np.zeros((2, h, w), np.uint8)
    occ[1, 3, 4] = 1                      # slot 1: one occluded pixel
    case = _dense_case(2, h, w, flow, occ)
    outs, _ = T.replay(case, None)
    assert np.array_equal(outs[0][1].reshape(h, w), np.broadcast_to(np.arange(w) < w - 1, (h, w)))    # x = 7 left the frame
    # at slot 1 a track is at (x + 0.5, y): taps x and x + 1 of row y, both weighted; row y + 1 has weight 0
    want = outs[0][1].reshape(h, w).copy()
    want[3, 3] = want[3, 4] = False
    assert np.array_equal(outs[1][1].reshape(h, w), want)
    assert np.array_equal(outs[1][0], outs[0][0])          # zero flow: nobody moved, the occluded ones froze where they were
    # an integer position has one weighted tap: only the track ON the pixel dies
    case = _dense_case(1, h, w, np.zeros((1, h, w, 2), np.float32), occ[1:])
    alive = T.replay(case, None)[0][0][1].reshape(h, w)
    assert not alive[3, 4] and alive.sum() == h * w - 1


# ------------------------------------------------------------------------------------------------- 3. mutants
# the cases every mutant is shown on: a later replay (carry source above 0, a drawn state with dead tracks in it) and a clip's
# first replay, with a blob mask and without, the pitch not the width on all of them
MUTANT_CASES = ('small-smooth-occ-full', 'ragged-S1-smooth-occ-first', 'ragged-S2-smooth-occ-full', 'ragged-S3-far-noocc-full',
                'sparse-65-smooth-occ-full', 'ragged-S1-far-noocc-first')
REJECTED_ON = {            # where each mutant must be caught (a mutant needs an input that shows it: occ, dead tracks, a carry)
    'anchor_sample': ('ragged-S1-smooth-occ-first', 'ragged-S2-smooth-occ-full', 'sparse-65-smooth-occ-full'),
    'pitch_w': MUTANT_CASES,
    'occ_after': ('small-smooth-occ-full', 'ragged-S1-smooth-occ-first', 'ragged-S2-smooth-occ-full'),
    'dead_move': ('small-smooth-occ-full', 'ragged-S2-smooth-occ-full', 'ragged-S3-far-noocc-full', 'sparse-65-smooth-occ-full'),
    'bound_w': ('ragged-S1-smooth-occ-first', 'ragged-S2-smooth-occ-full', 'ragged-S1-far-noocc-first'),
    'reinit': ('small-smooth-occ-full', 'ragged-S2-smooth-occ-full', 'ragged-S3-far-noocc-full', 'sparse-65-smooth-occ-full'),
}


def test_every_mutant_is_named():
    assert sorted(REJECTED_ON) == sorted(T.MUTANTS)


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_comparator_rejects_mutant(mutant):
    """A launch computed by a mutant of the definition (fp32, as a kernel with that mistake would) does not pass check_replay; the
    definition itself does, on the same cases."""
    for cid in REJECTED_ON[mutant]:
        case = BY_ID[cid]
        state = T.draw_state(case)
        assert T.check_replay(case, state, *T.replay(case, state)) <= 0.5 + 1e-9
        outs, new_state = T.replay(case, state, mutant=mutant)
        with pytest.raises(AssertionError):
            T.check_replay(case, state, outs, new_state)


# ------------------------------------------------------------------------------------------------- 4. tables and options
@pytest.mark.parametrize("k,B,carry", [(3, 3, 0), (1, 3, 3), (2, 2, 2), (1, 1, 0)])
def test_sequence_tables_track_words(k, B, carry):
    from unflow_amd.core.inference import sequence_tables
    shape = (90, 151)
    base, valid, nxt = sequence_tables(shape, k, B, carry, True)
    assert base.shape == (16 * B + 4,) and (base[16 * B + 2:] == 0).all()              # free and zero in every table so far
    none = sequence_tables(shape, k, B, carry, True, track=None)
    assert np.array_equal(none[0], base) and none[1:] == (valid, nxt)
    for S, N in ((1, 90 * 151), (3, 30 * 51), (0, 65), (7, 1)):
        tab, v, n = sequence_tables(shape, k, B, carry, True, track=(S, N))
        assert (v, n) == (valid, nxt) and tab.dtype == np.int32
        assert list(np.flatnonzero(tab != base)) == [16 * B + 2, 16 * B + 3][0 if S else 1:]
        assert (tab[16 * B + 2], tab[16 * B + 3]) == (S, N)
    both = sequence_tables(shape, k, B, carry, True, max_flow=20, track=(2, 5))[0]
    assert both[16 * B + 1] == 0x41a00000 and tuple(both[16 * B + 2:]) == (2, 5)
    for bad in ((-1, 5), (1, 0), (1, -4), (1, 2 ** 31)):
        with pytest.raises(ValueError, match="tracks"):
            sequence_tables(shape, k, B, carry, True, track=bad)


def test_track_option_and_grid():
    from unflow_amd.core.inference import Track, track_grid, track_option
    assert track_option(False) is None and track_option(None) is None
    assert track_option(True) == ('dense', 1) and track_option(1) == ('dense', 1) and track_option(np.int64(4)) == ('dense', 4)
    kind, pts = track_option([[3, 4], [0, 0], [-1, 700]])
    assert kind == 'sparse' and pts.dtype == np.int32 and pts.shape == (3, 2) and pts.flags['C_CONTIGUOUS']
    assert track_option(torch.tensor([[1, 2]]))[1].tolist() == [[1, 2]]
    for bad in (0, -2, 'dense', [[1.5, 2.0]], [1, 2], np.zeros((0, 2), np.int32), np.zeros((3, 3), np.int32), [[2 ** 31, 0]], {}):
        with pytest.raises(ValueError, match="track"):
            track_option(bad)
    assert track_grid((37, 53), 1) == (37, 53) and track_grid((37, 53), 2) == (19, 27) and track_grid((37, 53), 3) == (13, 18)
    assert track_grid((7, 10), 10) == (1, 1) and track_grid((7, 10), 11) == (1, 1)
    for S in (1, 2, 3, 5, 64):
        assert len(T.grid_anchors(37, 53, S)) == int(np.prod(track_grid((37, 53), S)))
    assert Track._fields == ('disp', 'alive')


def test_pair_files_track_entry_comes_last_and_is_no_png():
    from unflow_amd.core.inference import filter_entries, pair_files, sequence_visual_files
    pics = sequence_visual_files(5, True)
    for fmt in ('png', 'flo'):
        plain = pair_files(5, fmt, True, True, pics)
        assert pair_files(5, fmt, True, True, pics, track=False) == plain
        plan = pair_files(5, fmt, True, True, pics, track=True)
        assert plan[:-1] == plain and plan[-1] == ('000005_track.flo', ('track', 'track_disp'))
        rows = [(0, 90, 151), (2, 64, 128)]
        assert filter_entries(plan, rows, 3) == filter_entries(plain, rows, 3)


def test_estimator_option_rules_need_no_gpu():
    from unflow_amd.core.inference import FlowEstimator
    mk = lambda **kw: FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), **kw)   # noqa: E731
    for track in (True, 2, [[1, 2]]):
        with pytest.raises(ValueError, match="track .*needs sequence=True"):
            mk(track=track)
        with pytest.raises(ValueError, match="track .*needs sequence=True"):
            mk(bidirectional=True, track=track)
    for seq in (True, 'bidirectional'):
        for bad in (0, -1, 'all', [[0.5, 1.0]], [3, 4]):
            with pytest.raises(ValueError, match="track"):
                mk(sequence=seq, track=bad)


def _bare(**flags):
    """An estimator's flags without its engine: what the guards of the public methods look at."""
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator.__new__(FlowEstimator)
    for k, v in dict(dict(sequence=False, seq_bidir=False, bidirectional=False, visual=False, track=False), **flags).items():
        setattr(est, k, v)
    return est


@pytest.mark.parametrize("method", ['push_tracks', 'track_sequence'])
def test_track_methods_of_other_estimators_raise_and_name_the_option(method):
    frames = [np.zeros((64, 128, 3), np.uint8)] * 3
    with pytest.raises(RuntimeError, match=r"%s: a sequence estimator without tracks.*sequence=True, track=True" % method):
        getattr(_bare(sequence=True), method)(frames)
    with pytest.raises(RuntimeError, match=r"%s: .*sequence='bidirectional', track=True" % method):
        getattr(_bare(sequence=True, seq_bidir=True, bidirectional=True), method)(frames)
    with pytest.raises(RuntimeError, match=r"%s: a pair estimator; build it with FlowEstimator\(\.\.\., sequence=True\)" % method):
        getattr(_bare(), method)(frames)
    with pytest.raises(ValueError, match=r"export_sequence: the tracks need FlowEstimator\(\.\.\., sequence=True, track=True\)"):
        _bare(sequence=True).export_sequence(frames, '/nonexistent', tracks=True)
    with pytest.raises(RuntimeError, match="estimate: a sequence estimator"):        # a tracking estimator is a sequence estimator
        _bare(sequence=True, track=True).estimate(frames, frames)


# ------------------------------------------------------------------------------------------------- 5. the C entry
def test_symbol_is_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "unflow_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+unflow_sequence_track\s*\(([^)]*)\)\s*;", txt)
    assert m, "unflow_sequence_track is not declared in include/unflow_hip.h"
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 13 and args[0] == 'const float* flow_fw' and args[1] == 'const unsigned char* occ_fw'
    assert args[2] == 'const int* tab' and args[-1] == 'unflow_stream_t stream'
    assert hasattr(lib, 'unflow_sequence_track')


def test_null_and_shape_errors_do_not_need_a_gpu(lib):
    n = ctypes.c_void_p(0)
    p = ctypes.c_void_p(256)                              # never dereferenced: every case below returns before a launch
    ok = dict(flow=p, occ=n, tab=p, B=2, Hmax=96, Wmax=160, anchors=n, Ncap=100, disp=p, alive=p, out_disp=p, out_alive=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.unflow_sequence_track(a['flow'], a['occ'], a['tab'], a['B'], a['Hmax'], a['Wmax'], a['anchors'], a['Ncap'],
                                         a['disp'], a['alive'], a['out_disp'], a['out_alive'], n)
    for name in ('flow', 'tab', 'disp', 'alive', 'out_disp', 'out_alive'):
        assert call(**{name: n}) == -1, name
    for name in ('B', 'Ncap', 'Hmax', 'Wmax'):
        assert call(**{name: 0}) == -5 and call(**{name: -3}) == -5, name
    assert call(Hmax=65536, Wmax=32768) == -5             # Hmax * Wmax = 2^31
    assert call(occ=p, anchors=p, B=0) == -5


# ------------------------------------------------------------------------------------------------- 6. command line
def _frames(folder, n=3):
    from unflow_amd.core.input import write_png_rgb8
    folder.mkdir()
    rs = np.random.RandomState(1)
    for i in range(n):
        write_png_rgb8(str(folder / ("%04d.png" % i)), rs.randint(0, 256, size=(64, 128, 3)).astype(np.uint8))
    return str(folder)


def test_cli_track_flags(tmp_path, capsys):
    from unflow_amd import sequence as S
    base = ['--ex', 'x', '--frames', _frames(tmp_path / "clip")]
    d = S.parse_args(base)
    assert d.track is False and d.track_stride is None and d.track_points is None and d.track_option is False
    # every other default is what it was
    assert (d.out, d.flo, d.batch, tuple(d.net_size), d.output_backward, d.occlusion, d.visual, d.max_flow, d.config,
            d.host_decode) == ('../out', False, 4, (384, 1280), False, False, False, None, '../config.ini', False)
    assert S.parse_args(base + ['--track']).track_option is True
    assert S.parse_args(base + ['--track_stride', '4']).track_option == 4
    assert S.parse_args(base + ['--track', '--track_stride', '1']).track_option == 1
    pts = tmp_path / "points.txt"
    pts.write_text("# x y\n3 4\n\n  120   63 \n-1 7\n")
    a = S.parse_args(base + ['--track_points', str(pts), '--occlusion'])
    assert a.track_option.dtype == np.int32 and a.track_option.tolist() == [[3, 4], [120, 63], [-1, 7]] and a.occlusion
    capsys.readouterr()

    def refused(args, *words):
        with pytest.raises(SystemExit) as e:
            S.parse_args(base + args)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
    refused(['--track_stride', '0'], '--track_stride', 'at least 1')
    refused(['--track_stride', '-2'], 'at least 1')
    refused(['--track_points', str(pts), '--track'], 'one or the other')
    refused(['--track_points', str(pts), '--track_stride', '2'], 'one or the other')
    refused(['--track_points', str(tmp_path / "missing.txt")], 'missing.txt', 'not a readable text file')
    for text, words in (("3 4\n5\n", (':2:', 'two integers')), ("3 4.5\n", (':1:', 'two integers')), ("1 2 3\n", (':1:',)),
                        ("# nothing\n", ('no points',)), ("3 4\n%d 0\n" % 2 ** 31, (':2:', 'int32'))):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        refused(['--track_points', str(bad)], 'bad.txt', *words)
    with pytest.raises(SystemExit) as e:
        S.parse_args(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--track' in out and '--track_stride' in out and '--track_points' in out
