"""Flow visualisation, host side: known answers of the fp64 mirror (tests/visual_ref.py) that the GPU tests compare the kernels
with, the C ABI's argument checks of the visual entry points, the visualize CLI's flags, file names and contact sheets, and the
8-bit RGB PNG writer."""
import ctypes

import numpy as np
import pytest

import visual_ref as R


def _color_bytes(u, v, **kw):
    return tuple(int(c) for c in R.to_bytes(R.flow_to_color(np.array([[u, v]], np.float32), **kw))[0])


def test_mirror_colour_wheel_known_answers():
    assert _color_bytes(1, 0, max_flow=8) == (255, 0, 0)              # hue 0, s = 1
    assert _color_bytes(-1, 0, max_flow=8) == (0, 255, 255)           # hue 0.5: cyan
    assert _color_bytes(0, 1, max_flow=8) == (0, 255, 255)            # the reference's u == 0 rule: +pi, not pi / 2
    assert _color_bytes(0, -1, max_flow=8) == (0, 255, 255)           # -pi: the same hue
    assert _color_bytes(0, 0, max_flow=8) == (255, 255, 255)          # white, whatever the hue
    assert _color_bytes(0.5, 0, max_flow=8) == (255, 128, 128)        # s = 0.5
    assert _color_bytes(1, 0, max_flow=0.25) == (255, 0, 0)           # max(max_flow, 1)
    assert _color_bytes(-1, -1, max_flow=1) == (0, 64, 255)           # atan(1) - pi = -3 pi / 4: hue 5 / 8, d = 3.75, g = 0.25
    assert _color_bytes(1, 0, max_flow=8, mask=np.zeros(1)) == (0, 0, 0)
    # max_flow from the field: max |flow * mask| over both channels
    f = np.array([[0.25, 0], [0, 0], [100, 0], [-4, 0]], np.float32)
    img = R.to_bytes(R.flow_to_color(f, mask=np.array([1, 1, 0, 1], np.float32)))
    assert [tuple(p) for p in img] == [(255, 128, 128), (255, 255, 255), (0, 0, 0), (0, 255, 255)]    # max_flow 4: s = 0.25 * 8 / 4
    assert (R.to_bytes(R.flow_to_color(np.zeros((4, 5, 2), np.float32))) == 255).all()       # an all-zero field: white


def test_mirror_angle_table():
    a = R.ref_angle([1, -1, -1, 0, 0, 0, 1], [1, 0, -1, 2, -2, 0, -1])
    assert np.allclose(a, [np.pi / 4, np.pi, -3 * np.pi / 4, np.pi, -np.pi, 0.0, -np.pi / 4])


def _err_bytes(gt, d, mask_occ=1.0, mask_noc=1.0, **kw):
    gt = np.array([gt], np.float32)
    pred = gt + np.array([d], np.float32)
    return tuple(int(c) for c in R.to_bytes(R.flow_error_image(pred, gt, np.array([mask_occ]), np.array([mask_noc]), **kw))[0])


def test_mirror_error_image_known_answers():
    assert _err_bytes((10, 0), (2.25, 0)) == (224, 243, 248)          # min(0.75, 4.5) -> [0.5, 1)
    assert _err_bytes((100, 0), (2.25, 0)) == (171, 217, 233)         # min(0.75, 0.45) -> [0.25, 0.5): |gt| > 60
    # halved where not in noc: the exact round-half-up of the fp32 image value fp32(c / 255) * 0.5.  fp32(243 / 255) lies above
    # 243 / 255 (its half times 255 is 121.5000004), so the odd level rounds up
    assert _err_bytes((10, 0), (2.25, 0), mask_noc=0.0) == (112, 122, 124)
    assert _err_bytes((100, 0), (2.25, 0), mask_noc=0.0) == (86, 109, 117)     # 85.5000025, 108.5000011, 116.5000007
    assert _err_bytes((10, 0), (2.25, 0), mask_occ=0.0) == (0, 0, 0)
    assert _err_bytes((10, 0), (2.25, 0), mask_occ=0.0, mask_noc=0.0) == (0, 0, 0)
    assert _err_bytes((0, 0), (1.5, 0)) == (224, 243, 248)            # |gt| = 0: diff / 3 = 0.5
    assert _err_bytes((0, 0), (0, 0)) == (49, 54, 149)                # diff = 0: bin 0
    assert _err_bytes((7, -3), (0, 0)) == (49, 54, 149)
    # one probe inside each of the ten bins, through the absolute term (|gt| small enough that 20 diff / |gt| is larger)
    for lo, hi, r, g, b in R.COLORMAP:
        e = lo * 1.5 if lo > 0 else 0.03
        assert lo <= e < hi
        assert _err_bytes((1, 0), (0, 3 * e)) == (r, g, b), (lo, hi)
    # log_colors=False: min(diff, 5) / 5, red where occluded
    assert _err_bytes((10, 0), (2.5, 0), log_colors=False) == (128, 128, 128)
    assert _err_bytes((10, 0), (9, 0), mask_noc=0.0, log_colors=False) == (255, 0, 0)
    assert _err_bytes((10, 0), (9, 0), mask_occ=0.0, log_colors=False) == (0, 0, 0)


def test_mirror_edge_band_and_bytes():
    e = np.array([0.0625, 0.0625 * (1 + 5e-5), 0.0625 * (1 + 2e-4), 0.3, 16 * (1 - 9e-5), 15.9])
    assert list(R.edge_band(e)) == [True, True, False, False, True, False]
    assert list(R.to_bytes([-0.1, 0.0, 0.5 / 255, 0.49 / 255, 1.0, 1.7, 224 / 255])) == [0, 0, 1, 0, 255, 255, 224]


def test_mirror_resize_and_warp():
    rs = np.random.RandomState(0)
    a = rs.rand(6, 9, 3) * 255
    assert np.array_equal(R.resize_tf1(a, 6, 9), a)
    up = R.resize_tf1(a, 12, 18)
    assert np.allclose(up[::2, ::2], a) and np.allclose(up[1, 0], 0.5 * (a[0, 0] + a[1, 0]))
    assert np.allclose(up[-1], up[-2])                                 # the last source row is clamped
    fl = np.zeros((6, 9, 2), np.float32)
    assert np.array_equal(R.image_warp(a, fl), a)
    fl[..., 0] = 1.0
    w = R.image_warp(a, fl)
    assert np.array_equal(w[:, :-1], a[:, 1:]) and np.array_equal(w[:, -1], a[:, -1])
    fl[..., 0], fl[..., 1] = -3000.5, 0.25
    w = R.image_warp(a, fl)
    assert np.allclose(w[2], 0.75 * a[2, 0] + 0.25 * a[3, 0])


def test_visual_abi_argument_checks():
    """Status codes of the visual entry points that answer before any launch (no GPU needed)."""
    from unflow_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)             # never dereferenced: every call below returns before a launch
    n = None
    mf = ctypes.byref(ctypes.c_float(8.0))
    f = L.unflow_flow_to_color
    assert f(n, n, mf, 1, 8, 8, p, p, n, n) == -1                    # UNFLOW_ERR_NULL: no flow
    assert f(p, n, mf, 1, 8, 8, n, n, n, n) == -1                    # no output at all
    assert f(p, n, n, 1, 8, 8, p, n, n, n) == -1                     # max_flow to be reduced, but no scratch word
    assert f(p, p, mf, 0, 8, 8, p, p, n, n) == -5                    # UNFLOW_ERR_SHAPE
    assert f(p, p, n, 1, 8, -2, p, n, p, n) == -5
    f = L.unflow_flow_error_image
    assert f(n, p, p, p, 1, 1, 8, 8, p, p, n) == -1
    assert f(p, n, p, n, 1, 1, 8, 8, p, p, n) == -1
    assert f(p, p, n, n, 1, 1, 8, 8, p, p, n) == -1                  # mask_occ is required
    assert f(p, p, p, n, 1, 1, 8, 8, n, n, n) == -1
    assert f(p, p, p, n, 0, 1, 0, 8, p, n, n) == -5
    assert f(p, p, p, p, 1, 0, 8, 8, n, p, n) == -5
    f = L.unflow_inference_visual
    ok = dict(frames=p, desc=p, flow=p, gt_flow=n, gt_mask=n, shown=p, max_bits=p, out_u8=p, out_f32=n)

    def call(B=1, Hmax=8, Wmax=8, H=8, W=8, **kw):
        a = dict(ok, **kw)
        return f(a['frames'], a['desc'], B, Hmax, Wmax, H, W, a['flow'], a['gt_flow'], a['gt_mask'], a['shown'], a['max_bits'],
                 a['out_u8'], a['out_f32'], n)
    for k in ('frames', 'desc', 'flow', 'shown', 'max_bits', 'out_u8'):
        assert call(**{k: n}) == -1, k
    assert call(out_u8=n, out_f32=p, B=0) == -5                       # fp32 alone is an output
    assert call(gt_flow=p) == -1 and call(gt_mask=p) == -1            # the ground truth comes as a pair
    assert call(B=0) == -5 and call(Hmax=0) == -5 and call(W=-1) == -5 and call(H=0) == -5
    assert call(Hmax=65536, Wmax=65536) == -5
    assert call(gt_flow=p, gt_mask=p, B=-1) == -5


def test_visualize_cli_flags(capsys):
    from unflow_amd import visualize as V
    a = V.parse_args(['--ex', 'x'])
    assert (a.variant, a.num, a.num_vis, a.batch_size, a.sheet, tuple(a.dims)) == ('train_2012', 10, 100, 4, False, (384, 1280))
    a = V.parse_args(['--ex', 'x', '--variant', 'test_2015', '--num', '-1', '--num_vis', '8', '--batch_size', '2', '--sheet'])
    assert (a.variant, a.num, a.num_vis, a.batch_size, a.sheet) == ('test_2015', -1, 8, 2, True)
    for argv, msg in ((['--dataset', 'sintel'], 'not supported'), (['--dataset', 'chairs'], 'not supported'),
                      (['--dataset', 'mdb'], 'not supported'), (['--variant', 'val'], 'invalid choice'),
                      (['--batch_size', '0'], 'batch_size'), (['--num_vis', '-1'], 'num_vis')):
        with pytest.raises(SystemExit) as ex:
            V.parse_args(['--ex', 'x'] + argv)
        assert ex.value.code == 2
        assert msg in capsys.readouterr().err
    with pytest.raises(SystemExit):
        V.parse_args([])                                               # --ex is required


def test_visual_file_names():
    from unflow_amd.core.inference import VISUAL_IMAGES, FlowVisual, visual_files
    assert VISUAL_IMAGES[:3] == FlowVisual._fields == ('overlay', 'warp_error', 'flow')
    assert visual_files(7, False) == [(0, '000007_img.png'), (2, '000007_flow.png'), (1, '000007_diff.png')]
    assert visual_files(123456, True) == [(0, '123456_img.png'), (2, '123456_flow.png'), (1, '123456_diff.png'),
                                          (3, '123456_err.png'), (4, '123456_gt.png')]


def test_contact_sheet_on_unequal_sizes():
    from unflow_amd.visualize import contact_sheet
    rs = np.random.RandomState(1)
    a, b, c = (rs.randint(1, 256, size=s + (3,)).astype(np.uint8) for s in ((5, 9), (7, 4), (6, 6)))
    s = contact_sheet([[a, b, c], [c, a]])
    assert s.shape == (14, 27, 3) and s.dtype == np.uint8
    assert np.array_equal(s[:5, :9], a) and np.array_equal(s[:7, 9:13], b) and np.array_equal(s[:6, 18:24], c)
    assert np.array_equal(s[7:13, :6], c) and np.array_equal(s[7:12, 9:18], a)
    assert int((s != 0).all(2).sum()) == 2 * 45 + 28 + 2 * 36          # everything else is black
    with pytest.raises(ValueError):
        contact_sheet([])
    with pytest.raises(ValueError):
        contact_sheet([[a.astype(np.float32)]])


def test_write_pictures_files_and_sheets(tmp_path):
    from unflow_amd.core.input import decode_png
    from unflow_amd.visualize import SHEET_COLUMNS, contact_sheet, write_pictures
    rs = np.random.RandomState(2)

    def example(h, w, gt):
        names = ('overlay', 'warp_error', 'flow') + (('error', 'gt') if gt else ())
        return {k: rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for k in names}
    exs = [example(5, 8, True), example(6, 7, True), example(4, 9, True), example(5, 5, True), example(6, 6, True),
           example(3, 3, True)]
    paths = write_pictures(iter(exs), str(tmp_path), sheet=True, num_vis=5)
    names = [p.rsplit('/', 1)[-1] for p in paths]
    per = lambda n: [n + t for t in ('_img.png', '_flow.png', '_diff.png', '_err.png', '_gt.png')]   # noqa: E731
    assert names == per('000000') + per('000001') + per('000002') + per('000003') + ['page_000.png'] + per('000004') + \
        per('000005') + ['page_001.png']
    dec = lambda p: decode_png(open(p, 'rb').read())                  # noqa: E731
    assert np.array_equal(dec(paths[0]), exs[0]['overlay']) and np.array_equal(dec(paths[1]), exs[0]['flow'])
    assert np.array_equal(dec(paths[2]), exs[0]['warp_error']) and np.array_equal(dec(paths[3]), exs[0]['error'])
    assert np.array_equal(dec(paths[4]), exs[0]['gt'])
    assert np.array_equal(dec(paths[20]), contact_sheet([[e[c] for c in SHEET_COLUMNS[True]] for e in exs[:4]]))
    assert np.array_equal(dec(paths[-1]), contact_sheet([[exs[4][c] for c in SHEET_COLUMNS[True]]]))       # num_vis = 5
    # a test split: three pictures per example, three columns; no sheet unless asked for
    plain = [example(4, 4, False), example(2, 6, False)]
    out2 = tmp_path / "t"
    out2.mkdir()
    p2 = write_pictures(iter(plain), str(out2))
    assert [p.rsplit('/', 1)[-1] for p in p2] == ['000000_img.png', '000000_flow.png', '000000_diff.png', '000001_img.png',
                                                  '000001_flow.png', '000001_diff.png']


def test_png_rgb8_round_trip(tmp_path):
    from unflow_amd.core.input import decode_png, read_png_image, write_png_rgb8
    rs = np.random.RandomState(4)
    a = rs.randint(0, 256, size=(37, 53, 3)).astype(np.uint8)
    a[0, :5, 0] = [0, 1, 127, 128, 255]
    p = str(tmp_path / "000000_flow.png")
    write_png_rgb8(p, a)
    with open(p, 'rb') as f:
        back = decode_png(f.read())
    assert back.dtype == np.uint8 and np.array_equal(back, a)
    assert np.array_equal(read_png_image(p), a.astype(np.float32))
    for bad in (a.astype(np.uint16), a[..., 0], a[..., :2]):
        with pytest.raises(ValueError):
            write_png_rgb8(p, bad)


def test_flow_util_refuses_host_tensors():
    """The visualisers are HIP kernels: a CPU tensor is an error, not a fall-back."""
    import torch
    from unflow_amd.core import flow_util
    with pytest.raises(ValueError, match="device tensor"):
        flow_util.flow_to_color(torch.zeros(1, 4, 4, 2))
    with pytest.raises(ValueError, match="device tensor"):
        flow_util.flow_error_image(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 2), torch.ones(1, 4, 4, 1))
