"""Bidirectional sequence inference without a GPU: the engine's row plan — F frame rows in the tower, 2B rows
behind it, the tower's rows of cat2 behind the backward block — the flag rules of engine and estimator, and the command line."""
import pytest

from unflow_amd.core.engine import FlowNetEngine, _Stage

TOWER = ('conv1', 'conv2', 'conv3')
ENC = ('c1', 'cat2', 'c3')


class _Shape:
    """What _Stage reads of its engine for the row plan (tests/test_sequence_cpu.py's, plus seq_bidir)."""

    def __init__(self, B, one_dir, sequence=None, seq_bidir=None):
        self.B, self.N, self.one_dir = B, 2 * B, one_dir
        if sequence is not None:
            self.sequence = sequence
        if seq_bidir is not None:
            self.seq_bidir = seq_bidir


def _plan(st):
    return [(op.kind, None if op.l is None else op.l.name, op.src, op.dst, op.n, op.r0) for op in st.ops]


def _engine(spec, B, **kw):
    return FlowNetEngine(B, 64, 128, params=dict(flownet=spec), device='cpu', layout_only=True, seed=None, inference=True, **kw)


# ------------------------------------------------------------------------------------------------- row plan
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("spec", ['C', 'CS', 'S'])
def test_row_plan(spec, B):
    eng, pair = _engine(spec, B, sequence='bidirectional'), _engine(spec, B, bidirectional=True)
    F = B + 1
    assert eng.sequence is True and eng.bidirectional is True and eng.one_dir is False and eng.seq_bidir is True
    assert eng.F == F
    assert (eng.n_params, eng.n_weights) == (pair.n_params, pair.n_weights)
    for a, b in zip(pair.layers, eng.layers):               # the flat parameter layout is the pair engine's
        assert a.name == b.name and a.w.data_ptr() - pair.P.data_ptr() == b.w.data_ptr() - eng.P.data_ptr()
        assert a.b.data_ptr() - pair.P.data_ptr() == b.b.data_ptr() - eng.P.data_ptr()
    for i, st in enumerate(eng.stages):
        tower = st.is_c
        assert st.seq_bidir and st.rows['x0'] == F
        # two blocks on every stage, refinement stages included (they read the shared x0): the backward pairs (frame i + 1,
        # frame i) at rows [0, B), then the forward pairs at rows [B, 2B)
        assert st.pairs == [(1, 0, 0), (0, 1, B)]
        assert pair.stages[i].pairs is None                  # bidirectional=True: the directed batch
        for name in st.bufs:
            if tower and name == 'cat2':
                # the chosen layout: backward block, then the tower's F rows — 2B rows for the decoder, the last frame behind
                assert st.rows[name] == 2 * B + 1 and st.row0[name] == B
            elif tower and name in ENC:
                assert st.rows[name] == F and st.row0.get(name, 0) == 0, name
            else:
                assert st.rows[name] == 2 * B, (i, name)
        for op in st.ops:
            if op.kind == 'corr':
                assert op.n == F                             # reads all frame rows of c3, both ways round
                continue
            name = op.l.name.split('/')[-1]
            if tower and name in TOWER:
                # B rows from the tower's row 1 of either buffer
                assert op.n == B and op.r0 == 1 + st.row0.get(op.src[0], 0) and op.d0 == 1 + st.row0.get(op.dst[0], 0), name
            else:
                assert (op.n, op.r0, op.d0) == (2 * B, 0, 0), name
        if tower:
            by = {op.l.name.split('/')[-1]: op for op in st.ops if op.kind == 'layer'}
            assert (by['conv2'].r0, by['conv2'].d0) == (1, B + 1) and (by['conv3'].r0, by['conv3'].d0) == (B + 1, 1)


@pytest.mark.parametrize("B", [1, 3])
def test_final_flow_has_both_blocks_and_fw_bw_hides_their_order(B):
    import torch
    eng = _engine('C', B, sequence='bidirectional')
    # (layout_only engines allocate no activations: final_flow's 2B rows are asserted on the GPU; the split is testable here)
    t = torch.arange(2 * B)
    fw, bw = eng.fw_bw(t)
    assert fw.tolist() == list(range(B, 2 * B)) and bw.tolist() == list(range(B))      # backward block first
    fw, bw = _engine('C', B, bidirectional=True).fw_bw(t)
    assert fw.tolist() == list(range(B)) and bw.tolist() == list(range(B, 2 * B))      # the pair engine: forward first


# ------------------------------------------------------------------------------------------------- flag rules
@pytest.mark.parametrize("kind", ['C', 'S'])
@pytest.mark.parametrize("one_dir,seq", [(False, False), (True, False), (True, True)])
def test_other_plans_are_the_parents(kind, one_dir, seq):
    """An engine shape that has never heard of seq_bidir, and one that says False, plan alike: sequence in (False, True) is
    untouched, d0 follows r0."""
    B = 3
    old, off = _Stage(_Shape(B, one_dir, seq), kind, 0), _Stage(_Shape(B, one_dir, seq, False), kind, 0)
    assert not old.seq_bidir and not off.seq_bidir and old.row0 == off.row0 == {}
    assert old.rows == off.rows and _plan(old) == _plan(off)
    assert all(op.d0 == op.r0 for op in off.ops)
    assert old.bwd_names == off.bwd_names and len(old.bwd_names) == len(old.ops)
    for name, n in off.rows.items():
        if seq:
            assert n == (B + 1 if (name in (ENC if kind == 'C' else ()) or name == 'x0') else B), name
        else:
            assert n == (2 * B if (not one_dir or name in (ENC if kind == 'C' else ()) or name == 'x0') else B), name
    for op in off.ops:
        tower = seq and kind == 'C' and op.kind == 'layer' and op.l.name.split('/')[-1] in TOWER
        assert op.r0 == (1 if tower else 0)


@pytest.mark.parametrize("kw", [dict(), dict(bidirectional=True), dict(sequence=True)])
def test_engines_of_the_other_modes_keep_their_rows(kw):
    eng = _engine('CS', 2, **kw)
    assert eng.seq_bidir is False and eng.sequence is bool(kw.get('sequence')) and eng.bidirectional is bool(kw.get('bidirectional'))
    for st in eng.stages:
        assert not st.seq_bidir and all(op.d0 == op.r0 for op in st.ops)
        ref = _Stage(_Shape(2, eng.one_dir, eng.sequence), st.kind, st.index)
        assert st.rows == ref.rows and _plan(st) == _plan(ref)


def test_engine_flag_rules():
    mk = lambda **kw: FlowNetEngine(2, 64, 128, device='cpu', layout_only=True, seed=None, **kw)   # noqa: E731
    for seq in (True, 'bidirectional'):
        for kw in (dict(inference=True, bidirectional=True), dict(supervised=True), dict(), dict(inference=False)):
            with pytest.raises(ValueError, match="sequence"):
                mk(sequence=seq, **kw)
        with pytest.raises(ValueError, match="full_res"):
            FlowNetEngine(2, 64, 128, params=dict(flownet='S', full_res=True), device='cpu', layout_only=True, seed=None,
                          inference=True, sequence=seq)
    with pytest.raises(ValueError, match="'bidirectional'"):   # the message of bidirectional=True names the new spelling
        mk(inference=True, bidirectional=True, sequence=True)
    for bad in ('both', 'Bidirectional', '', 1, 0, None):
        with pytest.raises(ValueError, match="sequence"):
            mk(inference=True, sequence=bad)


def test_estimator_flag_rules_need_no_gpu():
    from unflow_amd.core.inference import FlowEstimator
    mk = lambda **kw: FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), **kw)   # noqa: E731
    for seq in (True, 'bidirectional'):
        for kw in (dict(bidirectional=True), dict(visual=True), dict(bidirectional=True, visual=True)):
            with pytest.raises(ValueError, match="sequence"):
                mk(sequence=seq, **kw)
    with pytest.raises(ValueError, match="sequence='bidirectional'"):
        mk(sequence=True, bidirectional=True)
    for bad in ('both', 1, None):
        with pytest.raises(ValueError, match="sequence"):
            mk(sequence=bad)


# ------------------------------------------------------------------------------------------------- command line
def test_cli_help_lists_the_new_flags(capsys):
    from unflow_amd import sequence as S
    with pytest.raises(SystemExit) as e:
        S.parse_args(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--output_backward' in out and '--occlusion' in out


def test_cli_takes_either_flag_alone(tmp_path):
    import numpy as np
    from unflow_amd import sequence as S
    from unflow_amd.core.input import write_png_rgb8
    rs = np.random.RandomState(1)
    for i in range(3):
        write_png_rgb8(str(tmp_path / ("%04d.png" % i)), rs.randint(0, 256, size=(64, 128, 3)).astype(np.uint8))
    base = ['--ex', 'x', '--frames', str(tmp_path), '--net_size', '64', '128']
    a = S.parse_args(base + ['--occlusion'])                 # without --output_backward: accepted
    assert a.occlusion and not a.output_backward and len(a.files) == 3
    a = S.parse_args(base + ['--output_backward', '--flo'])
    assert a.output_backward and not a.occlusion and a.flo
    a = S.parse_args(base)
    assert not a.output_backward and not a.occlusion
