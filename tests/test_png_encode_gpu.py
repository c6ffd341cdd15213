"""-m gpu: PNG encode on the device (csrc/png_encode.hip, core/png_device.py) — unflow_png_filter against the
numpy reference of png_filter_ref.py byte for byte, a launch over a list of strided surfaces, the filter choice on rows built
for each of the five filters, the sample kinds' values, the round trip through both decoders, skipped entries, and
FlowEstimator.export / export_sequence / the sequence command through the writer pool against the host writers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kitti_fixture
import png_filter_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS, HEIGHTS, KINDS = (1, 2, 3, 63, 64, 65, 257), (1, 2, 5), ('gray8', 'rgb8', 'rgb16')


def _P():
    from unflow_amd.core import png_device as P
    return P


def _L():
    from unflow_amd import _lib as L
    return L


def _scan_of(host, span):
    off, n, h, w, _, _ = span
    return host[off:off + n].reshape(h, n // h)


# ------------------------------------------------------------------------------------------------- 1. kernel vs reference
@pytest.mark.parametrize("kind", KINDS)
def test_filter_kernel_equals_the_reference(kind, dev):
    """Every width x height: scanlines and filter bytes, byte for byte.  A scanline is 1 + w * bpp bytes and the images lie back
    to back, so the rows start at every alignment: the head and tail bytes around the 16-byte stores."""
    P = _P()
    rng = np.random.RandomState(7 + KINDS.index(kind))
    xs = [R.random_image(rng, h, w, kind) for h in HEIGHTS for w in WIDTHS]
    out, spans = P.scanlines_device([torch.from_numpy(x).to(dev) for x in xs])
    host = out.cpu().numpy()
    starts = set()
    for x, span in zip(xs, spans):
        ref, filters, meta = R.reference_scanlines(x)
        got = _scan_of(host, span)
        assert span[2:] == meta
        assert np.array_equal(got[:, 0], filters), (kind, x.shape, got[:, 0].tolist(), filters.tolist())
        assert np.array_equal(got, ref), (kind, x.shape)
        starts |= {(span[0] + y * ref.shape[1]) % 16 for y in range(x.shape[0])}
    assert len(starts) >= 13 and 0 in starts      # a condition on the inputs: the row starts cover the alignments (16, 13, 15 of 16)


# ------------------------------------------------------------------------------------------------- 2. a list of surfaces
def test_one_launch_over_strided_surfaces(dev):
    """Three surfaces of different kinds, three images each of their own (h, w) inside a 9 x 70 allocation filled with 0xAB
    outside the image; the ranges of the table have gaps, and the output buffer keeps its bytes outside them."""
    P, L = _P(), _L()
    B, Hm, Wm = 3, 9, 70
    sizes = [(9, 70), (5, 33), (1, 64)]
    rng = np.random.RandomState(3)
    vis = np.full((B, Hm, Wm, 3), 0xAB, np.uint8)
    occ = np.full((B, Hm, Wm), 0xAB, np.uint8)
    u16 = np.full((B, Hm, Wm, 3), 0xABAB, np.uint16)
    imgs = {}
    for i, (h, w) in enumerate(sizes):
        vis[i, :h, :w] = imgs[0, i] = R.random_image(rng, h, w, 'rgb8')
        occ[i, :h, :w] = m = (rng.rand(h, w) < 0.3).astype(np.uint8)
        imgs[1, i] = m * np.uint8(255)
        u16[i, :h, :w] = imgs[2, i] = R.random_image(rng, h, w, 'rgb16')
    tens = [torch.from_numpy(vis).to(dev), torch.from_numpy(occ).to(dev), torch.from_numpy(u16.view(np.int16)).to(dev)]
    surfaces = [P.PngSurface(tens[0], B, Hm, Wm, 3, L.PNG_U8), P.PngSurface(tens[1], B, Hm, Wm, 1, L.PNG_U8X255),
                P.PngSurface(tens[2], B, Hm, Wm, 3, L.PNG_U16BE)]
    entries = [(s, i, h, w) for i, (h, w) in enumerate(sizes) for s in range(3)]
    rows, spans, total, max_h, max_row = P.plan_scanlines(surfaces, entries, first=5)
    gap = 3
    rows[:, 4] += gap * np.arange(len(entries))               # ranges with gaps between them
    spans = [(sp[0] + gap * k,) + tuple(sp[1:]) for k, sp in enumerate(spans)]
    n_out = total + gap * len(entries) + 11
    out = torch.full((n_out,), 0xCD, dtype=torch.uint8, device=dev)
    P.filter_scanlines(surfaces, torch.from_numpy(rows).to(dev), len(entries), max_h, max_row, out, torch.cuda.current_stream(dev))
    host = out.cpu().numpy()
    covered = np.zeros(n_out, bool)
    for (s, i, h, w), span in zip(entries, spans):
        ref, _, _ = R.reference_scanlines(imgs[s, i])
        assert np.array_equal(_scan_of(host, span), ref), (s, i)       # 0xAB beside or below the image would change the bytes
        covered[span[0]:span[0] + span[1]] = True
    assert (~covered).sum() == 5 + gap * (len(entries) - 1) + (gap + 11) and (host[~covered] == 0xCD).all()


# ------------------------------------------------------------------------------------------------- 3. the filter choice
@pytest.mark.parametrize("kind", ('rgb16', 'rgb8'))
def test_every_row_gets_the_reference_filter(kind, dev):
    P = _P()
    x = R.five_filter_case(kind)                  # asserts that all five filters occur in the reference
    ref, filters, _ = R.reference_scanlines(x)
    out, spans = P.scanlines_device([torch.from_numpy(x).to(dev)])
    got = _scan_of(out.cpu().numpy(), spans[0])
    assert got[:, 0].tolist() == filters.tolist()
    assert filters[0] == 1 and filters[-1] == 0   # a first row where Sub wins: 1, never 4; the all-zero row: 0
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------------- 4. values of the kinds
def test_sample_kinds(dev):
    P, L = _P(), _L()
    mask = torch.tensor([[1]], dtype=torch.uint8, device=dev)
    pat = torch.tensor([[[0x8001 - 65536, 0, 0]]], dtype=torch.int16, device=dev)
    surfaces = [P.PngSurface(mask, 1, 1, 1, 1, L.PNG_U8X255), P.PngSurface(pat, 1, 1, 1, 3, L.PNG_U16BE)]
    rows, spans, total, max_h, max_row = P.plan_scanlines(surfaces, [(0, 0, 1, 1), (1, 0, 1, 1)])
    out = torch.zeros(total, dtype=torch.uint8, device=dev)
    P.filter_scanlines(surfaces, torch.from_numpy(rows).to(dev), 2, max_h, max_row, out, torch.cuda.current_stream(dev))
    host = out.cpu().numpy().tolist()
    assert host == [0, 255] + [0, 0x80, 0x01, 0, 0, 0, 0]      # filter None (a tie with Sub and Up), then the raw bytes
    # encode_png_device's uint8 [h, w] is written as it is; int16 as its uint16 bit pattern
    a = torch.tensor([[1, 200], [0, 255]], dtype=torch.uint8, device=dev)
    back = P.decode_png_device(P.encode_png_device([a, pat]), dev)
    assert np.array_equal(back[0].cpu().numpy()[:, :, 0], a.cpu().numpy())
    assert back[1].cpu().numpy().tolist() == [[[0x8001, 0, 0]]]


# ------------------------------------------------------------------------------------------------- 5. round trip, skipping
def test_round_trip_through_both_decoders(dev):
    from unflow_amd.core.input import decode_png
    P = _P()
    rng = np.random.RandomState(11)
    xs = [R.random_image(rng, 7, 65, 'rgb16'), R.random_image(rng, 5, 3, 'gray8'), R.random_image(rng, 1, 257, 'rgb8'),
          R.five_filter_case('rgb16'), R.random_image(rng, 9, 64, 'rgb16').view(np.int16)]
    datas = P.encode_png_device([torch.from_numpy(x).to(dev) for x in xs], level=1)
    assert all(d[:8] == P.PNG_SIGNATURE and len(P._walk_chunks(d)[1]) == 1 for d in datas)
    for x, d, back in zip(xs, datas, P.decode_png_device(datas, dev)):
        want = x.view(np.uint16) if x.dtype == np.int16 else x
        assert np.array_equal(back.cpu().numpy().reshape(want.shape), want)
        assert np.array_equal(decode_png(d).reshape(want.shape), want)
        h, w, depth, ctype, raw = P.png_scanlines(d)
        assert bytes(raw) == R.reference_scanlines(x)[0].tobytes()
    assert P.encode_png_device([]) == []
    with pytest.raises(ValueError):
        P.encode_png_device([torch.zeros(2, 2, 3, device=dev)])        # float32


def test_an_entry_that_does_not_fit_is_skipped(dev):
    P, L = _P(), _L()
    rng = np.random.RandomState(13)
    xs = [R.random_image(rng, 4, 20, 'rgb8'), R.random_image(rng, 3, 9, 'rgb8'), R.random_image(rng, 2, 31, 'rgb8')]
    big = np.full((3, 4, 31, 3), 0xAB, np.uint8)
    for i, x in enumerate(xs):
        big[i, :x.shape[0], :x.shape[1]] = x
    t = torch.from_numpy(big).to(dev)
    surfaces = [P.PngSurface(t, 3, 4, 31, 3, L.PNG_U8)]
    entries = [(0, i, x.shape[0], x.shape[1]) for i, x in enumerate(xs)]
    rows, spans, total, max_h, max_row = P.plan_scanlines(surfaces, entries)
    full = torch.full((total + 64,), 0xCD, dtype=torch.uint8, device=dev)
    # entry 1 would end 10 bytes behind the buffer; two more entries name an image / a size their surface does not have
    rows = np.concatenate([rows, rows[:1], rows[:1]])
    rows[1, 4] = total - spans[1][1] + 10
    rows[3, 1] = 3
    rows[4, 3] = 32
    P.filter_scanlines(surfaces, torch.from_numpy(rows).to(dev), 5, max_h, max_row, full[:total], torch.cuda.current_stream(dev))
    host = full.cpu().numpy()
    for k in (0, 2):
        assert np.array_equal(_scan_of(host, spans[k]), R.reference_scanlines(xs[k])[0])
    assert (host[spans[1][0]:spans[1][0] + spans[1][1]] == 0xCD).all() and (host[total:] == 0xCD).all()
    # the host refuses what the kernel skips
    for bad in ([(0, 3, 2, 2)], [(0, 0, 5, 2)], [(0, 0, 2, 32)], [(1, 0, 2, 2)]):
        with pytest.raises(ValueError):
            P.plan_scanlines(surfaces, bad)


# ------------------------------------------------------------------------------------------------- 6. the estimator
def _params(est):
    """tests/test_sequence_gpu.py::_params: seed 31."""
    tfp = {k: v.cpu() for k, v in est.engine.init_params(seed=31).items()}
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    est.load_tf_params(tfp)
    return tfp


def _same_files(dir_a, dir_b, names, dev):
    """Every PNG of both directories decodes to the same array, .flo files have the same bytes, and each PNG of dir_b holds
    exactly the reference's (= the kernel's) scanlines of its pixels."""
    P = _P()
    pngs = [n for n in names if n.endswith('.png')]
    da = P.decode_png_device([open(os.path.join(dir_a, n), 'rb').read() for n in pngs], dev)
    datas_b = [open(os.path.join(dir_b, n), 'rb').read() for n in pngs]
    db = P.decode_png_device(datas_b, dev)
    filters = np.zeros(5, np.int64)
    for n, a, b, data in zip(pngs, da, db, datas_b):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), n
        x = b.cpu().numpy()
        ref, f, meta = R.reference_scanlines(x[:, :, 0] if x.shape[2] == 1 else x)
        h, w, depth, ctype, raw = P.png_scanlines(data)
        assert (h, w, depth, ctype) == meta and len(P._walk_chunks(data)[1]) == 1, n
        assert bytes(raw) == ref.tobytes(), n
        filters += np.bincount(f, minlength=5)
    for n in names:
        if n.endswith('.flo'):
            assert open(os.path.join(dir_a, n), 'rb').read() == open(os.path.join(dir_b, n), 'rb').read(), n
    return filters


def test_export_through_the_pool_equals_the_host_writers(dev, tmp_path, monkeypatch):
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.kitti.input import KITTIInput
    monkeypatch.setattr(kitti_fixture, 'SIZES', [(90, 151), (86, 149), (90, 150)])
    kitti_fixture.make_tree(tmp_path / "kitti", n_pairs=3)
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(96, 160), device=dev, bidirectional=True, visual=True)
    _params(est)
    einput = KITTIInput(kitti_fixture.Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(96, 160))
    kw = dict(backward=True, occlusion=True, visual=True)
    host = est.export(einput.input_train_2012(), str(tmp_path / "host"), fmt='png', **kw)
    graph = est.graph
    pool = est.export(einput.input_train_2012(), str(tmp_path / "pool"), fmt='png', workers=2, level=1, **kw)
    assert est.graph is graph and graph is not None                      # the filter launch is outside the graph: no re-capture
    names = [os.path.basename(p) for p in host]
    assert names == [os.path.basename(p) for p in pool] and len(names) == 3 * 8
    assert names[:8] == ['000000_10.png', '000000_01.png', '000000_10_occ.png', '000000_img.png', '000000_flow.png',
                         '000000_diff.png', '000000_err.png', '000000_gt.png']
    assert sorted(os.listdir(str(tmp_path / "pool"))) == sorted(names)
    filters = _same_files(str(tmp_path / "host"), str(tmp_path / "pool"), names, dev)
    assert filters[1:].sum() > 0                                         # the new files do use the filters
    # .flo flows through the same pool, beside the occlusion PNGs; and a device input
    hf = est.export(einput.input_train_2012(), str(tmp_path / "hflo"), fmt='flo', backward=True, occlusion=True)
    pf = est.export(einput.input_train_2012(device=dev), str(tmp_path / "pflo"), fmt='flo', backward=True, occlusion=True, workers=2)
    names = [os.path.basename(p) for p in hf]
    assert names == [os.path.basename(p) for p in pf] and len(names) == 9
    _same_files(str(tmp_path / "hflo"), str(tmp_path / "pflo"), names, dev)
    with pytest.raises(ValueError):
        est.export(einput.input_train_2012(), str(tmp_path / "bad"), workers=2, level=12)


def test_pictures_with_scanlines_and_write_pictures(dev, tmp_path, monkeypatch):
    from unflow_amd import visualize as V
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.kitti.input import KITTIInput
    monkeypatch.setattr(kitti_fixture, 'SIZES', [(90, 151), (86, 149), (90, 150)])
    kitti_fixture.make_tree(tmp_path / "kitti", n_pairs=3)
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(96, 160), device=dev, visual=True)
    _params(est)
    einput = KITTIInput(kitti_fixture.Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(96, 160))
    for d in ("host", "pool"):
        os.makedirs(str(tmp_path / d))
    host = V.write_pictures(est.pictures(einput.input_train_2012()), str(tmp_path / "host"), sheet=True)
    pool = V.write_pictures(est.pictures(einput.input_train_2012(), scanlines=True), str(tmp_path / "pool"), sheet=True,
                            workers=2, level=6)
    names = [os.path.basename(p) for p in host]
    assert names == [os.path.basename(p) for p in pool] and len(names) == 3 * 5 + 1
    _same_files(str(tmp_path / "host"), str(tmp_path / "pool"), [n for n in names if not n.startswith('page_')], dev)
    page = [n for n in names if n.startswith('page_')][0]                # the contact sheet is the host's either way
    assert open(str(tmp_path / "host" / page), 'rb').read() == open(str(tmp_path / "pool" / page), 'rb').read()


def test_export_sequence_through_the_pool_and_the_cli(dev, tmp_path):
    from test_sequence_gpu import clip
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import decode_png, write_png_rgb8
    from unflow_amd.core.train import Trainer
    H, W, h, w = 64, 128, 90, 151
    frames = clip(5, h, w, 50, u8=True)
    tr = Trainer(1, H, W, dict(flownet='C', pyramid_loss=True, border_mask=True, ternary_weight=1.0, smooth_2nd_weight=3.0,
                               learning_rate=1e-4, save_interval=1, display_interval=1), device=dev, seed=3, augment=False)
    tfp = tr.engine.export_tf_params()
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    tr.engine.load_tf_params(tfp)
    ckpt_dir = str(tmp_path / "ckpts" / "clipnet")
    os.makedirs(ckpt_dir)
    tr.save(ckpt_dir, 7)
    del tr
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(h, w), device=dev, sequence=True)
    names = ['%06d_10.png' % i for i in range(4)]
    host = est.export_sequence(frames, str(tmp_path / "host"), fmt='png')
    graph = est.graph
    pool = est.export_sequence(iter(frames), str(tmp_path / "pool"), fmt='png', workers=2)
    assert est.graph is graph and graph is not None
    assert [os.path.basename(p) for p in host] == names == [os.path.basename(p) for p in pool]
    _same_files(str(tmp_path / "host"), str(tmp_path / "pool"), names, dev)
    a, b = (decode_png(open(p[0], 'rb').read()) for p in (host, pool))   # and through the host decoder
    assert np.array_equal(a, b) and a.shape == (h, w, 3) and a.dtype == np.uint16
    fh = est.export_sequence(frames, str(tmp_path / "hflo"), fmt='flo')
    fp = est.export_sequence(frames, str(tmp_path / "pflo"), fmt='flo', workers=2)
    _same_files(str(tmp_path / "hflo"), str(tmp_path / "pflo"), [os.path.basename(p) for p in fh], dev)
    assert [os.path.basename(p) for p in fp] == ['%06d_10.flo' % i for i in range(4)]
    # the command line, as child processes: the device path and the host writers give the same pixels as the library
    fdir = tmp_path / "frames"
    fdir.mkdir()
    for i, f in enumerate(frames):
        write_png_rgb8(str(fdir / ("f%03d.png" % i)), f)
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp_path / "log", tmp_path / "ckpts"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for out, flags in (("cli_pool", ['--workers', '2']), ("cli_host", ['--host_encode'])):
        r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', str(fdir), '--out',
                            str(tmp_path / out), '--batch', '2', '--net_size', str(H), str(W), '--config', str(cfg)] + flags,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(str(tmp_path / out / "clipnet"))) == names
    _same_files(str(tmp_path / "cli_host" / "clipnet"), str(tmp_path / "cli_pool" / "clipnet"), names, dev)
    _same_files(str(tmp_path / "host"), str(tmp_path / "cli_pool" / "clipnet"), names, dev)
    for n in names:                                                       # --host_encode: the parent commit's files, byte for byte
        assert open(str(tmp_path / "host" / n), 'rb').read() == open(str(tmp_path / "cli_host" / "clipnet" / n), 'rb').read()
