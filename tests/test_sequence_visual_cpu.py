"""Visual sequence mode without a GPU: the clip-wide max_flow word of sequence_tables, the picture file names, the C entry's
declaration, export and argument errors, and the command line's flags."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from unflow_amd import build, _lib
    build.build()
    return _lib.lib()


def _todays_tables(shape, k, batch, carry, u8):
    """The array sequence_tables gave before the max_flow word existed, written out from the layout (pack_desc's rows)."""
    tab = np.zeros(16 * batch + 4, dtype=np.int32)
    for i in range(batch):
        if i < k:
            tab[8 * i:8 * i + 8] = (shape[0], shape[1], 0, 0, 0, int(u8), 0, 0)
        if i + 1 <= k and (i > 0 or carry > 0):
            tab[8 * batch + 8 * i:8 * batch + 8 * i + 8] = (shape[0], shape[1], 0, 0, 0, int(u8), 0, 0)
    tab[16 * batch] = carry
    return tab


@pytest.mark.parametrize("k,B,carry,u8", [(3, 3, 0, True), (1, 3, 3, False), (2, 2, 2, True), (1, 1, 1, False)])
def test_sequence_tables_max_flow_word(k, B, carry, u8):
    from unflow_amd.core.inference import sequence_tables
    shape = (90, 151)
    base, valid, nxt = sequence_tables(shape, k, B, carry, u8)
    assert base.dtype == np.int32 and base.shape == (16 * B + 4,) and nxt == k
    assert np.array_equal(base, _todays_tables(shape, k, B, carry, u8))       # the default: the array of every existing caller
    none, v2, n2 = sequence_tables(shape, k, B, carry, u8, max_flow=None)
    assert np.array_equal(none, base) and v2 == valid and n2 == nxt
    for given, stored in ((20, 20.0), (20.5, 20.5), (0.25, 1.0), (1, 1.0)):
        tab, v3, n3 = sequence_tables(shape, k, B, carry, u8, max_flow=given)
        assert v3 == valid and n3 == nxt and tab.dtype == np.int32
        differs = np.flatnonzero(tab != base)
        assert list(differs) == [16 * B + 1], (given, differs)
        assert tab[16 * B + 1:16 * B + 2].view(np.float32)[0] == np.float32(stored)
    assert sequence_tables(shape, k, B, carry, u8, max_flow=20)[0][16 * B + 1] == 0x41a00000      # the bits of 20.0f


def test_sequence_visual_files_names_and_order():
    from unflow_amd.core.inference import FlowVisual, SequenceVisual, sequence_visual_files, visual_files
    assert sequence_visual_files(7, False) == [(0, '000007_img.png'), (2, '000007_flow.png'), (1, '000007_diff.png')]
    assert sequence_visual_files(7, True) == [(0, '000007_img.png'), (2, '000007_flow.png'), (1, '000007_diff.png'),
                                              (3, '000007_flow_bw.png'), (4, '000007_diff_noc.png')]
    assert sequence_visual_files(3, False) == visual_files(3, False)          # the one-direction pictures keep export's names
    assert SequenceVisual._fields == FlowVisual._fields + ('flow_bw', 'warp_error_noc')
    assert SequenceVisual._fields[:3] == ('overlay', 'warp_error', 'flow')


_PICTURES = {       # what follows the flow files of a pair: (index into the picture surface, tag), as the docstrings list them
    'none': [],
    'pair': [(0, 'img'), (2, 'flow'), (1, 'diff')],
    'pair_gt': [(0, 'img'), (2, 'flow'), (1, 'diff'), (3, 'err'), (4, 'gt')],
    'sequence': [(0, 'img'), (2, 'flow'), (1, 'diff')],
    'sequence_bidir': [(0, 'img'), (2, 'flow'), (1, 'diff'), (3, 'flow_bw'), (4, 'diff_noc')],
}


@pytest.mark.parametrize("pictures", sorted(_PICTURES))
@pytest.mark.parametrize("occlusion", [False, True])
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("fmt", ['png', 'flo'])
def test_pair_files_names_order_and_filter_entries(fmt, backward, occlusion, pictures):
    """The one file plan of export / export_sequence: the names in the documented order (_10, _01, _10_occ, the pictures), a
    .flo file never from an encode surface, and the PNGs exactly the entries the pool path asks unflow_png_filter for."""
    from unflow_amd.core.inference import filter_entries, pair_files, sequence_visual_files, visual_files
    n, B = 41, 3
    pics = {'none': [], 'pair': visual_files(n, False), 'pair_gt': visual_files(n, True),
            'sequence': sequence_visual_files(n, False), 'sequence_bidir': sequence_visual_files(n, True)}[pictures]
    plan = pair_files(n, fmt, backward, occlusion, pics)
    names = ['000041_10.' + fmt] + (['000041_01.' + fmt] if backward else []) + (['000041_10_occ.png'] if occlusion else [])
    names += ['000041_%s.png' % tag for _, tag in _PICTURES[pictures]]
    assert [name for name, _ in plan] == names
    flows = ['flow'] + (['flow_bw'] if backward else [])
    surfaces = {'u16', 'u16_bw', 'occ', 'vis'}
    for name, src in plan:
        if name.endswith('.flo'):
            assert src[0] == 'flo' and src[1] not in surfaces and src == ('flo', flows.pop(0))
        else:
            assert src[0] == 'png' and src[1] in surfaces and len(src) == 3
    rows = [(0, 90, 151), (2, 64, 128)]                      # a replay whose slot 1 holds no pair
    want = []
    for i, h, w in rows:
        if fmt == 'png':
            want += [('u16', i, h, w)] + ([('u16_bw', i, h, w)] if backward else [])
        want += [('occ', i, h, w)] if occlusion else []
        want += [('vis', k * B + i, h, w) for k, _ in _PICTURES[pictures]]
    assert filter_entries(plan, rows, B) == want
    assert filter_entries(pair_files(0, fmt, backward, occlusion, pics), rows, B) == want      # the pair number names files only


def test_symbol_is_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "unflow_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+unflow_sequence_visual\s*\(([^)]*)\)\s*;", txt)
    assert m, "unflow_sequence_visual is not declared in include/unflow_hip.h"
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 15 and args[0] == 'const void* frames' and args[1] == 'const int* tab' and args[-1] == 'unflow_stream_t stream'
    assert hasattr(lib, 'unflow_sequence_visual')


def test_null_and_shape_errors_do_not_need_a_gpu(lib):
    n = ctypes.c_void_p(0)
    p = ctypes.c_void_p(256)                              # never dereferenced: every case below returns before a launch
    f = lib.unflow_sequence_visual
    ok = dict(frames=p, tab=p, B=2, Hmax=96, Wmax=160, H=64, W=128, fw=p, bw=n, occ=n, shown=p, bits=p, u8=p, f32=n)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['frames'], a['tab'], a['B'], a['Hmax'], a['Wmax'], a['H'], a['W'], a['fw'], a['bw'], a['occ'], a['shown'],
                 a['bits'], a['u8'], a['f32'], n)
    for name in ('frames', 'tab', 'fw', 'shown', 'bits'):
        assert call(**{name: n}) == -1, name
    assert call(u8=n, f32=n) == -1                        # no output at all
    assert call(bw=p) == -1 and call(occ=p) == -1         # the backward flow and the occlusion mask come together
    for name in ('B', 'Hmax', 'Wmax', 'H', 'W'):
        assert call(**{name: 0}) == -5 and call(**{name: -3}) == -5, name
    assert call(Hmax=65536, Wmax=32768) == -5             # Hmax * Wmax = 2^31
    assert call(bw=p, occ=p, B=0) == -5
    # unflow_inference_visual's own answers to the same mistakes
    g = lib.unflow_inference_visual
    assert g(n, p, 2, 96, 160, 64, 128, p, n, n, p, p, p, n, n) == -1
    assert g(p, p, 2, 96, 160, 64, 128, p, p, n, p, p, p, n, n) == -1
    assert g(p, p, 0, 96, 160, 64, 128, p, n, n, p, p, p, n, n) == -5
    assert g(p, p, 2, 65536, 32768, 64, 128, p, n, n, p, p, p, n, n) == -5


def test_estimator_flag_rules_need_no_gpu():
    """The pictures along a clip are spelt visual='sequence'; visual=True with sequence raises as it always did and names it."""
    from unflow_amd.core.inference import FlowEstimator
    mk = lambda **kw: FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), **kw)   # noqa: E731
    for seq in (True, 'bidirectional'):
        with pytest.raises(ValueError, match="visual='sequence'"):
            mk(sequence=seq, visual=True)
    with pytest.raises(ValueError, match="sequence=True"):
        mk(visual='sequence')
    with pytest.raises(ValueError, match="sequence='bidirectional'"):
        mk(sequence=True, bidirectional=True, visual='sequence')
    for bad in ('clip', 'Sequence', 1, None):
        with pytest.raises(ValueError, match="visual"):
            mk(sequence=True, visual=bad)


# ------------------------------------------------------------------------------------------------- command line
def _frames(folder, n=3):
    from unflow_amd.core.input import write_png_rgb8
    folder.mkdir()
    rs = np.random.RandomState(1)
    for i in range(n):
        write_png_rgb8(str(folder / ("%04d.png" % i)), rs.randint(0, 256, size=(64, 128, 3)).astype(np.uint8))
    return str(folder)


def test_cli_visual_flags(tmp_path, capsys):
    from unflow_amd import sequence as S
    clip = _frames(tmp_path / "clip")
    base = ['--ex', 'x', '--frames', clip]
    a = S.parse_args(base + ['--visual', '--max_flow', '20', '--batch', '2', '--net_size', '64', '128'])
    assert a.visual is True and a.max_flow == 20.0 and a.batch == 2 and tuple(a.net_size) == (64, 128)
    assert S.parse_args(base + ['--visual']).max_flow is None
    d = S.parse_args(base)
    assert d.visual is False and d.max_flow is None
    # every other default is what it was
    assert (d.out, d.flo, d.batch, tuple(d.net_size), d.output_backward, d.occlusion, d.config, d.host_decode) == \
        ('../out', False, 4, (384, 1280), False, False, '../config.ini', False)
    assert len(d.files) == 3 and d.frame_size == (64, 128)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        S.parse_args(base + ['--max_flow', '20'])
    assert e.value.code == 2 and '--visual' in capsys.readouterr().err
    for bad in ('0', '-4'):
        with pytest.raises(SystemExit) as e:
            S.parse_args(base + ['--visual', '--max_flow', bad])
        assert e.value.code == 2 and 'positive' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        S.parse_args(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--visual' in out and '--max_flow' in out
