"""Forward-only inference, host side: the KITTI 16-bit encoding and its PNG round trip, .flo / export file names, the
inference engine's parameter layout, the descriptor tables of the batch packer, and the evaluate CLI's flags."""
import os

import numpy as np
import pytest
import torch


def test_flow_to_int16_clamps_truncates_and_sets_valid():
    from unflow_amd.core.input import flow_to_int16
    f = np.array([[[0.0, 0.0], [1.0 / 64 * 0.99, -1.0 / 64 * 0.99], [-600.0, 600.0], [-512.0, 511.984375]],
                  [[2.5, -2.5], [0.3, -0.3], [1e9, -1e9], [-511.99, 512.0]]], dtype=np.float32)
    q = flow_to_int16(f)
    assert q.dtype == np.uint16 and q.shape == (2, 4, 3)
    assert (q[..., 2] == 1).all()
    assert tuple(q[0, 0, :2]) == (32768, 32768)
    assert tuple(q[0, 1, :2]) == (32768, 32767)            # 32768.63 -> 32768, 32767.37 -> 32767: truncation
    assert tuple(q[0, 2, :2]) == (0, 65535)                # clamped at both ends
    assert tuple(q[0, 3, :2]) == (0, 65535)
    assert tuple(q[1, 0, :2]) == (32928, 32608)
    assert tuple(q[1, 1, :2]) == (32787, 32748)            # 19.2 -> 19, -19.2 -> 32748.8 -> 32748
    assert tuple(q[1, 2, :2]) == (65535, 0)
    assert tuple(q[1, 3, :2]) == (0, 65535)
    # torch input and a batch dimension
    assert (flow_to_int16(torch.from_numpy(f)[None]) == q[None]).all()


def test_kitti_png_round_trip(tmp_path):
    from unflow_amd.core.input import flow_to_int16, read_kitti_flow_png, write_kitti_flow_png
    rs = np.random.RandomState(0)
    f = (rs.randn(37, 53, 2) * 40).astype(np.float32)
    q = flow_to_int16(f)
    p = str(tmp_path / "000000_10.png")
    write_kitti_flow_png(p, q)
    flow, mask = read_kitti_flow_png(p)
    assert flow.shape == (37, 53, 2) and mask.shape == (37, 53, 1)
    assert (mask.numpy() == 1).all()
    assert np.array_equal(flow.numpy(), (q[..., :2].astype(np.float32) - 2 ** 15) / 64.0)
    assert np.abs(flow.numpy() - f).max() <= 1.0 / 64 + 1e-6          # truncation: within one quantum
    with pytest.raises(ValueError):
        write_kitti_flow_png(p, q.astype(np.int32))


def test_write_flo_round_trip(tmp_path):
    from unflow_amd.core.input import read_flo, write_flo
    f = np.random.RandomState(1).randn(9, 14, 2).astype(np.float32)
    p = str(tmp_path / ("%06d_10.flo" % 3))
    write_flo(p, f)
    assert os.path.basename(p) == "000003_10.flo"
    g, m = read_flo(p)
    assert np.array_equal(g.numpy(), f) and (m.numpy() == 1).all()
    with open(p, 'rb') as fh:
        head = fh.read(12)
    assert np.frombuffer(head[:4], '<f4')[0] == np.float32(202021.25)
    assert tuple(np.frombuffer(head[4:], '<i4')) == (14, 9)


@pytest.mark.parametrize("spec,extra", [('C', {}), ('CSS', {}), ('css', {}), ('S', dict(full_res=True))])
def test_inference_engine_layout_matches_training_engine(spec, extra):
    from unflow_amd.core.engine import FlowNetEngine
    p = dict(flownet=spec, **extra)
    tr = FlowNetEngine(2, 384, 1280, params=p, device='cpu', layout_only=True, seed=None)
    inf = FlowNetEngine(2, 384, 1280, params=p, device='cpu', layout_only=True, seed=None, inference=True)
    assert inf.inference and inf.one_dir and not tr.inference
    assert (inf.n_params, inf.n_weights) == (tr.n_params, tr.n_weights)
    for a, b in zip(tr.layers, inf.layers):
        assert a.name == b.name and a.cout_p == b.cout_p and a.wshape() == b.wshape()
        assert a.w.data_ptr() - tr.P.data_ptr() == b.w.data_ptr() - inf.P.data_ptr()
        assert a.b.data_ptr() - tr.P.data_ptr() == b.b.data_ptr() - inf.P.data_ptr()
        assert b.dw is None and b.db is None and b.mw is None and b.vb is None
    assert inf.G is None and inf.M is None and inf.V is None
    assert all(not st.trainable for st in inf.stages)
    # the same names and shapes out and in: checkpoints restore unchanged
    tfp = tr.init_params(seed=3)
    inf.load_tf_params(tfp)
    assert torch.equal(inf.P, tr.P)
    out = inf.export_tf_params()
    assert list(out) == list(tfp) and all(torch.equal(out[k], tfp[k]) for k in tfp)


def test_inference_engine_refuses_training_calls():
    from unflow_amd.core.engine import FlowNetEngine
    e = FlowNetEngine(1, 64, 64, device='cpu', layout_only=True, seed=None, inference=True)
    for call in (lambda: e.forward_loss(), lambda: e.backward_net(), lambda: e.adam_step(1e-4), lambda: e.fwd_bwd(),
                 lambda: e.train_step(None, None, 1e-4)):
        with pytest.raises(RuntimeError, match="forward-only"):
            call()
    with pytest.raises(ValueError):
        FlowNetEngine(1, 64, 64, device='cpu', layout_only=True, seed=None, inference=True, supervised=True)


KITTI_SIZES = [(370, 1226), (375, 1242), (376, 1241)]


def _crop_or_pad_origin(h, w, H, W):
    """Where frame pixel (0, 0) lands in resize_image_with_crop_or_pad(frame, H, W), measured with a marker image."""
    from unflow_amd.core.input import resize_image_with_crop_or_pad
    a = np.zeros((h, w, 1), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    a[..., 0] = yy * 10000 + xx + 1
    s = resize_image_with_crop_or_pad(a, H, W)[..., 0]
    nz = np.argwhere(s > 0)
    r, c = nz[0]
    v = int(s[r, c]) - 1
    return int(r) - v // 10000, int(c) - v % 10000


@pytest.mark.parametrize("dims", [(384, 1280), (320, 1216), (360, 1240)])
def test_pack_desc_kitti_layout_origins(dims):
    from unflow_amd.core.inference import pack_desc
    sizes = KITTI_SIZES + [(436, 1024)]
    d = pack_desc(sizes, 4, staged=dims, nmaps=2, u8=True)
    assert d.dtype == np.int32 and d.shape == (4, 8)
    for row, (h, w) in zip(d, sizes):
        assert tuple(row[:2]) == (h, w) and tuple(row[4:]) == (2, 1, 0, 0)
        assert tuple(row[2:4]) == _crop_or_pad_origin(h, w, *dims), (h, w, dims)


def test_pack_desc_raw_frames_and_short_batch():
    from unflow_amd.core.inference import pack_desc
    d = pack_desc(KITTI_SIZES[:2], 4)
    assert [tuple(r) for r in d] == [(370, 1226, 0, 0, 0, 0, 0, 0), (375, 1242, 0, 0, 0, 0, 0, 0), (0,) * 8, (0,) * 8]
    with pytest.raises(ValueError):
        pack_desc(KITTI_SIZES, 2)


def test_example_stream_and_chunks_keep_order_and_short_tail():
    from unflow_amd.core.inference import chunks, example_stream
    bs = []
    for n0, n in ((0, 3), (3, 3), (6, 1)):
        im = np.arange(n0, n0 + n, dtype=np.float32)[:, None, None, None] * np.ones((1, 4, 6, 3), np.float32)
        bs.append((im, im + 1, np.tile(np.array([[4, 6, 3]], np.int32), (n, 1))))
    exs = list(example_stream(bs))
    assert [float(e[0][0, 0, 0]) for e in exs] == list(range(7))
    sizes = [len(c) for c in chunks(exs, 2)]
    assert sizes == [2, 2, 2, 1]
    with pytest.raises(ValueError):
        list(example_stream([(np.zeros((1, 2, 2, 3)),) * 4]))


def test_cli_flags():
    from unflow_amd import evaluate as E
    a = E.parse_args(['--ex', 'x', '--variant', 'test_2015', '--num', '-1', '--output_benchmark', '--output_png',
                      '--batch_size', '8'])
    assert (a.ex, a.dataset, a.variant, a.num, a.output_benchmark, a.output_png, a.batch_size) == \
        ('x', 'kitti', 'test_2015', -1, True, True, 8)
    a = E.parse_args(['--ex', 'y'])
    assert (a.variant, a.num, a.output_benchmark, a.output_png, tuple(a.dims)) == ('train_2012', 10, False, False, (384, 1280))


@pytest.mark.parametrize("argv,msg", [(['--output_visual'], 'output_visual'), (['--output_backward'], 'output_backward'),
                                      (['--dataset', 'sintel'], 'not supported'), (['--dataset', 'chairs'], 'not supported'),
                                      (['--dataset', 'mdb'], 'not supported'), (['--variant', 'val'], 'invalid choice')])
def test_cli_refuses_unsupported(argv, msg, capsys):
    from unflow_amd import evaluate as E
    with pytest.raises(SystemExit) as ex:
        E.parse_args(['--ex', 'x'] + argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


def test_cli_experiment_lookup(tmp_path):
    """eval_gui.py:101-117: the experiment's own config when its logs hold one, the logs folder's checkpoint first, then
    <dirs.checkpoints>/<name>; none: an error."""
    from unflow_amd import evaluate as E
    from unflow_amd.core.input import save_checkpoint
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\ndata = %s\n" % (tmp_path / "log", tmp_path / "ckpt", tmp_path / "data"))
    with pytest.raises(SystemExit, match="checkpoint"):
        E.experiment_paths('ex1', str(cfg))
    ck = tmp_path / "ckpt" / "ex1"
    ck.mkdir(parents=True)
    save_checkpoint(str(ck / "model.ckpt-5"), {'a/weights': torch.zeros(2)})
    with open(ck / "checkpoint", "w") as f:
        f.write('model_checkpoint_path: "model.ckpt-5"\n')
    assert E.experiment_paths('ex1', str(cfg)) == (str(cfg), str(ck))
    logs = tmp_path / "log" / "ex" / "ex1"
    logs.mkdir(parents=True)
    (logs / "config.ini").write_text("[train]\nflownet = C\n")
    assert E.experiment_paths('ex1', str(cfg)) == (str(logs / "config.ini"), str(ck))
    save_checkpoint(str(logs / "model.ckpt-9"), {'a/weights': torch.zeros(2)})
    with open(logs / "checkpoint", "w") as f:
        f.write('model_checkpoint_path: "model.ckpt-9"\n')
    assert E.experiment_paths('ex1', str(cfg)) == (str(logs / "config.ini"), str(logs))


def test_network_files_strict_refuses_a_missing_network(tmp_path):
    from unflow_amd.core.train import network_files
    with pytest.raises(ValueError, match="nothing to restore"):
        network_files(dict(flownet='CS'), 'CS', str(tmp_path), strict=True)
    files, ckpt = network_files(dict(flownet='CS', finetune=['a', 'b']), 'CS', str(tmp_path), strict=True)
    assert files == ['a', 'b'] and ckpt is None
    files, _ = network_files(dict(flownet='CS'), 'CS', str(tmp_path))      # not strict: nothing restored, no error
    assert files == [None, None]
