"""Sequence inference without a GPU: the engine's row plan (F = B + 1 frame rows, the tower on rows [1, F)), the host packing
of pushes into the frame table, the pair table and the carry source, the flag combinations, and the command line."""
import numpy as np
import pytest

from unflow_amd.core.engine import FlowNetEngine, _Stage

TOWER = ('conv1', 'conv2', 'conv3')
ENC = ('c1', 'cat2', 'c3')


class _Shape:
    """What _Stage reads of its engine for the row plan."""

    def __init__(self, B, one_dir, sequence=None):
        self.B, self.N, self.one_dir = B, 2 * B, one_dir
        if sequence is not None:
            self.sequence = sequence


def _plan(st):
    return [(op.kind, None if op.l is None else op.l.name, op.src, op.dst, op.n, op.r0) for op in st.ops]


@pytest.mark.parametrize("B", [1, 2, 4])
def test_row_plan_of_a_flownet_c(B):
    st = _Stage(_Shape(B, True, True), 'C', 0)
    F = B + 1
    assert st.rows['x0'] == F
    assert st.pairs == [(0, 1, 0)]                           # one block: pair i = (frame row i, frame row i + 1) -> row i
    for name in st.bufs:
        assert st.rows[name] == (F if name in ENC else B), name
    for op in st.ops:
        if op.kind == 'corr':
            assert (op.r0, op.n) == (0, F)                   # reads rows [0, B) against rows [1, F)
        elif op.l.name.split('/')[-1] in TOWER:
            assert (op.r0, op.n) == (1, B), op.l.name        # rows [1, B + 1): row 0 is carried, never computed
        else:
            assert (op.r0, op.n) == (0, B), op.l.name


@pytest.mark.parametrize("B", [1, 3])
def test_row_plan_of_a_flownet_s_changes_x0_alone(B):
    seq, pair = _Stage(_Shape(B, True, True), 'S', 0), _Stage(_Shape(B, True, False), 'S', 0)
    assert seq.rows.pop('x0') == B + 1 and pair.rows.pop('x0') == 2 * B
    assert seq.rows == pair.rows and all(v == B for v in seq.rows.values())
    assert seq.pairs == [(0, 1, 0)] and pair.pairs == [(0, B, 0)]     # the stage input reads the pair's frames from x0
    assert _plan(seq) == _plan(pair) and all(op.r0 == 0 for op in seq.ops)


@pytest.mark.parametrize("kind", ['C', 'S'])
@pytest.mark.parametrize("one_dir", [False, True])
def test_without_the_flag_the_plan_is_the_parents(kind, one_dir):
    """sequence=False (and an engine shape that has never heard of the flag) gives the rows and the op list of today: the
    bidirectional plan on N rows, the one-direction plan with the tower on 2B rows."""
    B = 3
    old, off = _Stage(_Shape(B, one_dir), kind, 0), _Stage(_Shape(B, one_dir, False), kind, 0)
    assert old.rows == off.rows and _plan(old) == _plan(off)
    assert old.pairs == off.pairs == ([(0, B, 0)] if one_dir else None)     # None: the directed batch, one launch over N rows
    assert all(op.r0 == 0 for op in off.ops)
    for name, n in off.rows.items():
        assert n == (2 * B if (not one_dir or name in (ENC if kind == 'C' else ()) or name == 'x0') else B), name
    assert old.bwd_names == off.bwd_names and old.bwd_zero_rows == off.bwd_zero_rows and old.bwd_post_act == off.bwd_post_act


@pytest.mark.parametrize("kw", [dict(supervised=True), dict(inference=True), dict(inference=True, bidirectional=True), {}])
def test_engines_without_the_flag_keep_their_rows(kw):
    a = FlowNetEngine(2, 64, 128, params=dict(flownet='CS'), device='cpu', layout_only=True, seed=None, **kw)
    b = FlowNetEngine(2, 64, 128, params=dict(flownet='CS'), device='cpu', layout_only=True, seed=None, sequence=False, **kw)
    assert not a.sequence and not b.sequence
    for sa, sb in zip(a.stages, b.stages):
        assert sa.rows == sb.rows and _plan(sa) == _plan(sb)
        assert sa.rows['x0'] == 4 and all(op.r0 == 0 for op in sa.ops)


def test_sequence_engine_layout_and_flags():
    p = dict(flownet='CS')
    pair = FlowNetEngine(2, 64, 128, params=p, device='cpu', layout_only=True, seed=None, inference=True)
    seq = FlowNetEngine(2, 64, 128, params=p, device='cpu', layout_only=True, seed=None, inference=True, sequence=True)
    assert seq.sequence and seq.one_dir and seq.F == 3
    assert (seq.n_params, seq.n_weights) == (pair.n_params, pair.n_weights)
    for a, b in zip(pair.layers, seq.layers):               # the flat parameter layout is unchanged
        assert a.name == b.name and a.w.data_ptr() - pair.P.data_ptr() == b.w.data_ptr() - seq.P.data_ptr()
    assert seq.stages[0].rows['c3'] == 3 and seq.stages[1].rows['c3'] == 2     # only the first network has a tower
    # ... but the refinement stage has the same pair blocks: its input takes the frames from x0, which the stages share
    assert seq.stages[0].pairs == seq.stages[1].pairs == [(0, 1, 0)] and pair.stages[0].pairs == pair.stages[1].pairs == [(0, 2, 0)]
    for kw in (dict(inference=True, bidirectional=True), dict(supervised=True), dict(), dict(inference=False)):
        with pytest.raises(ValueError, match="sequence"):
            FlowNetEngine(2, 64, 128, device='cpu', layout_only=True, seed=None, sequence=True, **kw)
    with pytest.raises(ValueError, match="full_res"):
        FlowNetEngine(2, 64, 128, params=dict(flownet='S', full_res=True), device='cpu', layout_only=True, seed=None,
                      inference=True, sequence=True)


def test_estimator_flag_combinations_need_no_gpu():
    from unflow_amd.core.inference import FlowEstimator
    for kw in (dict(bidirectional=True), dict(visual=True), dict(bidirectional=True, visual=True)):
        with pytest.raises(ValueError, match="sequence"):
            FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), sequence=True, **kw)


# ------------------------------------------------------------------------------------------------- host packing
@pytest.mark.parametrize("B", [1, 2, 4])
def test_packing_of_a_clip_stages_every_frame_once_and_every_pair_once(B):
    from unflow_amd.core.inference import sequence_replays
    h, w = 90, 151
    for T in sorted({2, B, B + 1, B + 2, 2 * B + 1} - {1}):
        rows = [None] * (B + 1)                 # the frame of the clip every engine row holds (None: none of this clip)
        staged, pairs, prev_k = [], [], 0
        for r, (n0, k, tab, valid) in enumerate(sequence_replays(T, B, (h, w), u8=True)):
            assert tab.dtype == np.int32 and tab.shape == (16 * B + 4,)
            frame, pair, src = tab[:8 * B].reshape(B, 8), tab[8 * B:16 * B].reshape(B, 8), int(tab[16 * B])
            assert src == prev_k                          # the carry source: the last staged row of the previous replay
            if src:
                rows[0] = rows[src]                       # unflow_sequence_carry
            for i in range(B):                            # unflow_inference_input_frames: slot i -> row i + 1
                if i < k:
                    assert tuple(frame[i]) == (h, w, 0, 0, 0, 1, 0, 0)
                    rows[i + 1] = n0 + i
                    staged.append(n0 + i)
                else:
                    assert frame[i, 0] == 0
                    rows[i + 1] = None
            got = [i for i in range(B) if pair[i, 0] > 0]
            assert got == list(valid)
            if r == 0:
                assert 0 not in got                       # no carried frame yet: one wasted pair slot per clip
            for i in got:
                assert tuple(pair[i]) == (h, w, 0, 0, 0, 1, 0, 0)
                assert rows[i] is not None and rows[i + 1] == rows[i] + 1, (T, B, r, i, rows)
                pairs.append(rows[i])
            # no valid pair is left out: two consecutive rows with consecutive frames are always announced
            for i in range(B):
                if rows[i] is not None and rows[i + 1] is not None:
                    assert i in got
            prev_k = k
        assert staged == list(range(T)), (T, B)           # every frame exactly once, in order
        assert pairs == list(range(T - 1)), (T, B)        # every pair (i, i + 1) in exactly one replay, in order


def test_packing_refuses_what_is_no_clip():
    from unflow_amd.core.inference import sequence_replays, sequence_tables
    with pytest.raises(ValueError, match="two frames"):
        sequence_replays(1, 2)
    with pytest.raises(ValueError):
        sequence_tables((64, 128), 3, 2, 0)               # B + 1 new frames
    with pytest.raises(ValueError):
        sequence_tables((64, 128), 0, 2, 0)
    with pytest.raises(ValueError):
        sequence_tables((64, 128), 1, 2, 3)               # a carry source past the last row
    tab, valid, nxt = sequence_tables((64, 128), 1, 2, 2)  # a short push after a full one
    assert valid == [0] and nxt == 1 and tab[32] == 2 and tab[16:32].reshape(2, 8)[1, 0] == 0


# ------------------------------------------------------------------------------------------------- command line
def _frames(folder, sizes):
    from unflow_amd.core.input import write_png_rgb8
    folder.mkdir()
    rs = np.random.RandomState(1)
    for i, (h, w) in enumerate(sizes):
        write_png_rgb8(str(folder / ("%04d.png" % i)), rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
    return str(folder)


def test_cli_help_lists_the_options(capsys):
    from unflow_amd import sequence as S
    with pytest.raises(SystemExit) as e:
        S.parse_args(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ('--ex', '--frames', '--out', '--flo', '--batch', '--net_size'):
        assert flag in out


def test_cli_refuses_a_folder_that_is_no_clip(tmp_path, capsys):
    from unflow_amd import sequence as S
    one = _frames(tmp_path / "one", [(64, 128)])
    with pytest.raises(SystemExit) as e:
        S.parse_args(['--ex', 'x', '--frames', one])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "at least two" in err and "0000.png" in err
    mixed = _frames(tmp_path / "mixed", [(64, 128), (64, 128), (60, 128)])
    with pytest.raises(SystemExit) as e:
        S.parse_args(['--ex', 'x', '--frames', mixed])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "0002.png" in err and "60x128" in err
    ok = _frames(tmp_path / "ok", [(64, 128)] * 3)
    a = S.parse_args(['--ex', 'x', '--frames', ok, '--flo', '--batch', '2', '--net_size', '64', '128'])
    assert len(a.files) == 3 and a.frame_size == (64, 128) and a.flo and a.batch == 2 and tuple(a.net_size) == (64, 128)
    assert np.array_equal(S.read_frame(a.files[0]).shape, (64, 128, 3)) and S.read_frame(a.files[0]).dtype == np.uint8
