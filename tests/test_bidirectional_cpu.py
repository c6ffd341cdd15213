"""Bidirectional inference, host side: the bidirectional inference engine's layout and row plan, its argument checks, the
evaluate CLI's --output_backward / --occlusion flags, the pooled occlusion scores, the 8-bit PNG writer and the C ABI's
argument checks of the occlusion kernel."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("spec,extra", [('C', {}), ('CSS', {}), ('css', {}), ('S', dict(full_res=True))])
def test_bidirectional_inference_engine_layout_and_rows(spec, extra):
    from unflow_amd.core.engine import FlowNetEngine
    p = dict(flownet=spec, **extra)
    tr = FlowNetEngine(2, 384, 1280, params=p, device='cpu', layout_only=True, seed=None)
    bi = FlowNetEngine(2, 384, 1280, params=p, device='cpu', layout_only=True, seed=None, inference=True, bidirectional=True)
    assert bi.inference and bi.bidirectional and not bi.one_dir and not bi.supervised
    assert (bi.n_params, bi.n_weights) == (tr.n_params, tr.n_weights)
    for a, b in zip(tr.layers, bi.layers):
        assert a.name == b.name and a.cout_p == b.cout_p and a.wshape() == b.wshape()
        assert a.w.data_ptr() - tr.P.data_ptr() == b.w.data_ptr() - bi.P.data_ptr()
        assert a.b.data_ptr() - tr.P.data_ptr() == b.b.data_ptr() - bi.P.data_ptr()
        assert b.dw is None and b.db is None and b.mw is None and b.vb is None
    assert len(tr.layers) == len(bi.layers)
    assert bi.G is None and bi.M is None and bi.V is None
    for st in bi.stages:
        assert not st.trainable
        assert all(n == bi.N for n in st.rows.values()), st.rows
        assert all(op.n == bi.N for op in st.ops)
    tfp = tr.init_params(seed=3)
    bi.load_tf_params(tfp)
    assert torch.equal(bi.P, tr.P)
    out = bi.export_tf_params()
    assert list(out) == list(tfp) and all(torch.equal(out[k], tfp[k]) for k in tfp)


def test_bidirectional_argument_checks_and_no_training():
    from unflow_amd.core.engine import FlowNetEngine
    kw = dict(device='cpu', layout_only=True, seed=None)
    with pytest.raises(ValueError, match="inference"):
        FlowNetEngine(1, 64, 64, bidirectional=True, **kw)
    with pytest.raises(ValueError, match="supervised"):
        FlowNetEngine(1, 64, 64, bidirectional=True, supervised=True, **kw)
    with pytest.raises(ValueError):
        FlowNetEngine(1, 64, 64, bidirectional=True, supervised=True, inference=True, **kw)
    e = FlowNetEngine(1, 64, 64, inference=True, bidirectional=True, **kw)
    for call in (lambda: e.forward_loss(), lambda: e.backward_net(), lambda: e.adam_step(1e-4), lambda: e.fwd_bwd(),
                 lambda: e.train_step(None, None, 1e-4)):
        with pytest.raises(RuntimeError, match="forward-only"):
            call()
    one = FlowNetEngine(1, 64, 64, inference=True, **kw)
    assert one.one_dir and not one.bidirectional


def test_cli_backward_and_occlusion_flags(capsys):
    from unflow_amd import evaluate as E
    a = E.parse_args(['--ex', 'x', '--output_benchmark', '--output_backward', '--output_png'])
    assert a.output_benchmark and a.output_backward and a.output_png and not a.occlusion
    a = E.parse_args(['--ex', 'x', '--occlusion'])
    assert a.occlusion and not a.output_backward
    a = E.parse_args(['--ex', 'x', '--occlusion', '--output_benchmark'])
    assert a.occlusion and a.output_benchmark
    with pytest.raises(SystemExit) as ex:
        E.parse_args(['--ex', 'x', '--output_backward'])
    assert ex.value.code == 2
    assert "--output_backward requires --output_benchmark" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ex:
        E.parse_args(['--ex', 'x', '--output_benchmark', '--output_visual'])
    assert ex.value.code == 2
    assert 'output_visual' in capsys.readouterr().err


def test_occlusion_scores_pooled_and_zero_denominators():
    from unflow_amd.core.inference import OCC_NAMES, occlusion_scores
    s = occlusion_scores([[3, 1, 2], [1, 0, 0], [0, 0, 0]])      # tp 4, fp 1, fn 2
    assert list(s) == list(OCC_NAMES)
    assert s['occ/precision'] == pytest.approx(80.0)
    assert s['occ/recall'] == pytest.approx(400.0 / 6)
    assert s['occ/F1'] == pytest.approx(800.0 / 11)
    assert occlusion_scores([[0, 0, 0]]) == dict.fromkeys(OCC_NAMES, 0.0)
    z = occlusion_scores([[0, 5, 0], [0, 2, 0]])                 # no positives at all: recall's denominator is 0
    assert z == dict.fromkeys(OCC_NAMES, 0.0)
    z = occlusion_scores(np.array([[0, 0, 7]], np.int32))       # no predicted positives: precision's denominator is 0
    assert z['occ/precision'] == 0.0 and z['occ/recall'] == 0.0 and z['occ/F1'] == 0.0


def test_png_gray8_round_trip(tmp_path):
    from unflow_amd.core.input import read_png_image, write_png_gray8
    rs = np.random.RandomState(4)
    a = (rs.rand(37, 53) < 0.3).astype(np.uint8) * np.uint8(255)
    a[0, :5] = [0, 1, 127, 128, 254]
    p = str(tmp_path / "000000_10_occ.png")
    write_png_gray8(p, a)
    back = read_png_image(p)
    assert back.shape == (37, 53, 3)
    assert np.array_equal(back[..., 0], a.astype(np.float32))
    assert np.array_equal(back[..., 1], back[..., 0]) and np.array_equal(back[..., 2], back[..., 0])
    with pytest.raises(ValueError):
        write_png_gray8(p, a.astype(np.uint16))
    with pytest.raises(ValueError):
        write_png_gray8(p, a[..., None])


def test_occlusion_abi_argument_checks():
    """Status codes of unflow_inference_occlusion that answer before any launch (no GPU needed)."""
    from unflow_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)             # never dereferenced: every call below returns before a launch
    n = None
    f = L.unflow_inference_occlusion
    assert f(n, p, p, 1, 8, 8, n, p, p, n, n) == -1                  # UNFLOW_ERR_NULL
    assert f(p, p, p, 1, 8, 8, n, p, n, n, n) == -1
    assert f(p, p, n, 1, 8, 8, n, p, p, n, n) == -1
    assert f(p, p, p, 1, 8, 8, p, p, p, n, n) == -1                  # GT maps but no counts
    assert f(p, p, p, 0, 8, 8, n, p, p, n, n) == -5                  # UNFLOW_ERR_SHAPE
    assert f(p, p, p, 1, 0, 8, n, p, p, n, n) == -5
    assert f(p, p, p, 1, 8, -1, n, p, p, n, n) == -5
    assert f(p, p, p, 1, 65536, 65536, n, p, p, n, n) == -5
