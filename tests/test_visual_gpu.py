"""-m gpu: flow visualisation — the kernels of csrc/visual.hip against the fp64 mirror (tests/visual_ref.py) on the same float32
inputs, overlay / brightness error against the chained library launches, the error image outside a band around the bin edges,
graph against eager, and FlowEstimator(visual=True)'s export and the visualize CLI end to end on a KITTI-format tree.

Bounds (derived, not measured): the continuous images (colour wheel, overlay, brightness error) lie in [0, 1] and are a dozen
fp32 operations plus atanf behind their inputs, about ten ulp of 1.0 = 1.2e-6; asserted within 1e-5 absolute.  A byte can differ
from the mirror's only where the value sits on a half level: at most one level.  The error image is piecewise constant: bytes
equal wherever the fp64 error is farther than a relative 1e-4 from every bin edge, and that band may exclude at most 0.1 % of the
mask_occ pixels."""
import os

import numpy as np
import pytest
import torch

import visual_ref as R
from kitti_fixture import Data, make_tree

pytestmark = pytest.mark.gpu

KITTI_SIZES = [(370, 1226), (375, 1242), (376, 1241)]
FLOAT_TOL = 1e-5
BAND = 1e-4
BAND_SHARE = 1e-3


def _lib():
    from unflow_amd import _lib as L
    return L


def _close(got, ref, what):
    """Float image within FLOAT_TOL of the mirror; prints the measured maximum."""
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    print("%s: max |kernel - fp64 mirror| = %.3g" % (what, err))
    assert err <= FLOAT_TOL, (what, err)
    return err


def _bytes_within_one(got, ref_img, what):
    d = np.abs(got.astype(np.int16) - R.to_bytes(ref_img).astype(np.int16))
    print("%s: bytes differing from the mirror's: %d of %d (max %d level)" % (what, int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1, (what, int(d.max()))


def _field(rs, h, w, scale=1.0):
    """A flow field with exact zeros, u == 0 columns, all four quadrants and a block of vectors of thousands of pixels."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f = np.stack([12.0 * np.sin(xx / 31.0) + 3.0 * np.cos(yy / 17.0), 9.0 * np.cos(xx / 23.0 + 1.0) - 4.0 * np.sin(yy / 29.0)], 2)
    f = (f * scale + rs.randn(h, w, 2) * 0.3).astype(np.float32)
    f[:, 5] = 0.0                                        # exact zero vectors
    f[:, 11::40, 0] = 0.0                                # u == 0, v != 0: the +-pi rule
    f[7::30, :, 1] = 0.0                                 # v == 0: hue 0 or 0.5
    f[3, :8] = [[1, 0], [-1, 0], [0, 1], [0, -1], [0.5, 0], [-2, -2], [2, -2], [0, 0]]
    f[h // 2:h // 2 + 6, w // 3:w // 3 + 50] = rs.randn(6, 50, 2).astype(np.float32) * 4000.0
    return f


def test_flow_to_color_vs_mirror(dev):
    from unflow_amd.core import flow_util
    rs = np.random.RandomState(3)
    B, H, W = 3, 97, 203
    flow = np.stack([_field(rs, H, W), _field(rs, H, W, 0.2), np.zeros((H, W, 2), np.float32)])
    mask = (rs.rand(B, H, W, 1) < 0.6).astype(np.float32)
    mask[0, H // 2:H // 2 + 6] = 0.0                     # the far-out block is masked: max_flow comes from the rest
    fd, md = torch.from_numpy(flow).to(dev), torch.from_numpy(mask).to(dev)
    for what, kw, rkw in (("no mask", {}, {}), ("masked", dict(mask=md), dict(mask=mask)),
                          ("max_flow 8", dict(max_flow=8.0), dict(max_flow=8.0)),
                          ("masked, max_flow 0.5", dict(mask=md, max_flow=0.5), dict(mask=mask, max_flow=0.5))):
        ref = R.flow_to_color(flow, **rkw)
        got = flow_util.flow_to_color(fd, **kw)
        got8 = flow_util.flow_to_color(fd, uint8=True, **kw)
        torch.cuda.synchronize()
        assert got.shape == (B, H, W, 3) and got.dtype == torch.float32 and got8.dtype == torch.uint8
        g = got.cpu().numpy()
        _close(g, ref, "flow_to_color (%s)" % what)
        _bytes_within_one(got8.cpu().numpy(), ref, "flow_to_color (%s)" % what)
        assert np.array_equal(got8.cpu().numpy(), R.to_bytes(g))          # the byte is the exact rounding of the fp32 value
        again = flow_util.flow_to_color(fd, **kw)
        assert torch.equal(got, again)
    # known answers, as bytes
    probe = torch.tensor([[[[1, 0], [-1, 0], [0, 1], [0, 0], [0.5, 0]]]], dtype=torch.float32, device=dev)
    b8 = flow_util.flow_to_color(probe, max_flow=8.0, uint8=True)[0, 0].cpu().numpy()
    assert [tuple(int(c) for c in p) for p in b8] == [(255, 0, 0), (0, 255, 255), (0, 255, 255), (255, 255, 255), (255, 128, 128)]
    # an all-zero batch: white
    z = flow_util.flow_to_color(torch.zeros(1, 9, 13, 2, device=dev), uint8=True)
    assert (z == 255).all()


def _kitti_like_error_case(rs, h, w):
    """kitti_fixture-style ground truth and a prediction whose error is log-uniform in [0.01, 80] px in a random direction."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    gt = np.round(np.stack([3.0 + 2.0 * np.sin(xx / 97.0) + 40.0 * xx / w, -1.0 + 1.5 * np.cos(yy / 53.0)], 2) * 64.0) / 64.0
    gt = gt.astype(np.float32)
    mag = np.exp(rs.uniform(np.log(0.01), np.log(80.0), size=(h, w)))
    ang = rs.uniform(0, 2 * np.pi, size=(h, w))
    pred = (gt + np.stack([mag * np.cos(ang), mag * np.sin(ang)], 2)).astype(np.float32)
    m_occ = (rs.rand(h, w, 1) < 0.35).astype(np.float32)
    m_noc = m_occ * (rs.rand(h, w, 1) < 0.8).astype(np.float32)
    pred[0, :4] = gt[0, :4]                               # diff == 0
    gt[1, :4] = 0.0                                       # |gt| == 0
    m_occ[:2, :4] = 1.0
    m_noc[:2, :4] = 1.0
    return pred, gt, m_occ, m_noc


def _check_error_bytes(got8, pred, gt, m_occ, m_noc, what):
    """Bytes equal to the mirror's outside the band around the bin edges; the band's share of the mask_occ pixels is asserted."""
    ref8 = R.to_bytes(R.flow_error_image(pred, gt, m_occ, m_noc))
    error, _ = R.kitti_error(pred, gt)
    band = R.edge_band(error, BAND)
    valid = m_occ.reshape(error.shape) != 0
    share = float((band & valid).sum()) / max(1, int(valid.sum()))
    bad = (got8 != ref8).any(-1)
    print("%s: %.4f %% of the mask_occ pixels in the edge band; %d pixels differ inside it, %d outside"
          % (what, 100 * share, int((bad & band).sum()), int((bad & ~band).sum())))
    assert share <= BAND_SHARE, (what, share)
    assert not (bad & ~band).any(), (what, int((bad & ~band).sum()))
    return error, valid


def test_flow_error_image_vs_mirror(dev):
    from unflow_amd.core import flow_util
    rs = np.random.RandomState(5)
    h, w = 376, 1241
    pred, gt, m_occ, m_noc = _kitti_like_error_case(rs, h, w)
    t = lambda a: torch.from_numpy(a[None]).to(dev)       # noqa: E731
    got8 = flow_util.flow_error_image(t(pred), t(gt), t(m_occ), t(m_noc), uint8=True)[0].cpu().numpy()
    gotf = flow_util.flow_error_image(t(pred), t(gt), t(m_occ), t(m_noc))[0].cpu().numpy()
    error, valid = _check_error_bytes(got8, pred, gt, m_occ, m_noc, "flow_error_image")
    assert np.array_equal(got8, R.to_bytes(gotf))
    # all ten bins are populated among the evaluated pixels, 5 - 33 % each
    edges = [0.0] + R.EDGES + [1e9]
    shares = [float(((error >= lo) & (error < hi) & valid).sum()) / valid.sum() for lo, hi in zip(edges[:-1], edges[1:])]
    assert min(shares) > 0.05 and max(shares) < 0.33, shares
    # the colours themselves, the halving and the mask
    colors = {tuple(int(c) for c in p) for p in got8[(m_noc[..., 0] != 0)]}
    assert colors == {(r, g, b) for _, _, r, g, b in R.COLORMAP}
    assert (got8[m_occ[..., 0] == 0] == 0).all()
    assert tuple(got8[0, 0]) == (49, 54, 149) and tuple(got8[1, 0]) in {(r, g, b) for _, _, r, g, b in R.COLORMAP}
    # mask_noc absent = ones
    got1 = flow_util.flow_error_image(t(pred), t(gt), t(m_occ), uint8=True)[0].cpu().numpy()
    _check_error_bytes(got1, pred, gt, m_occ, np.ones_like(m_occ), "flow_error_image (no mask_noc)")
    # log_colors=False is continuous: min(diff, 5) / 5, a few fp32 operations
    lin = flow_util.flow_error_image(t(pred), t(gt), t(m_occ), t(m_noc), log_colors=False)[0].cpu().numpy()
    ref = R.flow_error_image(pred, gt, m_occ, m_noc, log_colors=False)
    _close(lin, ref, "flow_error_image (log_colors=False)")
    lin8 = flow_util.flow_error_image(t(pred), t(gt), t(m_occ), t(m_noc), log_colors=False, uint8=True)[0].cpu().numpy()
    _bytes_within_one(lin8, ref, "flow_error_image (log_colors=False)")
    # known answers
    g2 = torch.tensor([[[[10, 0], [100, 0], [10, 0], [10, 0]]]], dtype=torch.float32, device=dev)
    p2 = g2 + torch.tensor([2.25, 0], device=dev)
    mo = torch.tensor([1, 1, 1, 0], dtype=torch.float32, device=dev).view(1, 1, 4, 1)
    mn = torch.tensor([1, 1, 0, 1], dtype=torch.float32, device=dev).view(1, 1, 4, 1)
    k8 = flow_util.flow_error_image(p2, g2, mo, mn, uint8=True)[0, 0].cpu().numpy()
    assert [tuple(int(c) for c in p) for p in k8] == [(224, 243, 248), (171, 217, 233), (112, 122, 124), (0, 0, 0)]


# ------------------------------------------------------------------------------------------------------ the desc-driven form
def _frame_of(staged, h, w):
    from unflow_amd.core.input import resize_image_with_crop_or_pad
    return resize_image_with_crop_or_pad(staged, h, w)


def _run_visual(frames, desc, flow, gt_flow, gt_mask, B, Hm, Wm, H, W, dev, with_f32=True):
    L = _lib()
    u8 = torch.full((5, B, Hm, Wm, 3), 7, dtype=torch.uint8, device=dev)
    f32 = torch.full((5, B, Hm, Wm, 3), -3.0, device=dev) if with_f32 else None
    shown = torch.zeros(2, B, Hm, Wm, 4, device=dev)
    bits = torch.zeros(3 * B, dtype=torch.int32, device=dev)             # maxima and tickets: zero before, zero after
    L.check(L.lib().unflow_inference_visual(L.ptr(frames), L.ptr(desc), B, Hm, Wm, H, W, L.ptr(flow), L.ptr(gt_flow), L.ptr(gt_mask),
                                            L.ptr(shown), L.ptr(bits), L.ptr(u8), L.ptr(f32), L.stream()), "inference_visual")
    torch.cuda.synchronize()
    assert (bits == 0).all()
    return u8.cpu().numpy(), None if f32 is None else f32.cpu().numpy(), shown.cpu().numpy()


def _chained(fr1, fr2, flow, H, W, dev):
    """overlay and brightness error through the library's own launches: unflow_resize_bilinear_tf1 twice per frame, then
    unflow_image_warp_fwd; the elementwise tail in numpy float32 (one correctly rounded operation at a time)."""
    L = _lib()
    h, w = fr1.shape[:2]
    shown = []
    for fr in (fr1, fr2):
        a = torch.from_numpy(np.ascontiguousarray(fr, np.float32)[None]).to(dev)
        net, back = torch.zeros(1, H, W, 3, device=dev), torch.zeros(1, h, w, 3, device=dev)
        L.check(L.lib().unflow_resize_bilinear_tf1(L.ptr(a), L.ptr(net), 1, h, w, 3, H, W, L.cf(1.0), L.stream()), "resize")
        L.check(L.lib().unflow_resize_bilinear_tf1(L.ptr(net), L.ptr(back), 1, H, W, 3, h, w, L.cf(1.0), L.stream()), "resize")
        shown.append(back)
    fl = torch.from_numpy(np.ascontiguousarray(flow)[None]).to(dev)
    warped = torch.zeros(1, h, w, 3, device=dev)
    L.check(L.lib().unflow_image_warp_fwd(L.ptr(shown[1]), 3, L.ptr(fl), L.cf(1.0), L.ptr(warped), None, 0, 1, h, w, 3, L.stream()),
            "image_warp")
    torch.cuda.synchronize()
    im1, im2, wp = shown[0][0].cpu().numpy(), shown[1][0].cpu().numpy(), warped[0].cpu().numpy()
    half, c255 = np.float32(0.5), np.float32(255.0)
    return (im1 * half + im2 * half) / c255, np.abs(im1 - wp) / c255


@pytest.mark.parametrize("u8", [True, False], ids=['uint8', 'fp32'])
def test_inference_visual_kernel_vs_mirror_and_chained_launches(u8, dev):
    from unflow_amd.core.inference import pack_desc
    from unflow_amd.core.input import resize_image_with_crop_or_pad
    H, W = 384, 1280
    Hs, Ws = 384, 1280                                   # the KITTIInput layout: frames padded / cropped into it
    Hm, Wm = 448, 1280
    sizes = KITTI_SIZES + [(97, 203), (0, 0), (400, 1280)]                # (400, 1280): taller than the layout, cropped into it
    B = len(sizes)
    rs = np.random.RandomState(9 + int(u8))
    dt = np.uint8 if u8 else np.float32
    frames = np.zeros((2, B, Hm, Wm, 3), dt)
    flow = rs.randn(B, Hm, Wm, 2).astype(np.float32)     # junk outside the frames: must not be read into the pictures
    gt_flow = np.zeros((2, B, Hm, Wm, 2), np.float32)
    gt_mask = np.zeros((2, B, Hm, Wm), np.float32)
    raw, gts = [], []
    for b, (h, w) in enumerate(sizes):
        if h == 0:
            raw.append(None)
            gts.append(None)
            continue
        small = rs.randint(0, 256, size=(h // 4 + 2, w // 4 + 2, 3))
        a = np.kron(small, np.ones((4, 4, 1)))[:h, :w] if u8 else rs.rand(h, w, 3) * 255.0
        a = a.astype(dt)
        c = np.roll(a, (1, -3), (0, 1))
        frames[0, b, :Hs, :Ws] = resize_image_with_crop_or_pad(a, Hs, Ws)
        frames[1, b, :Hs, :Ws] = resize_image_with_crop_or_pad(c, Hs, Ws)
        # what the kernel sees of the frame: the staged layout cropped / padded back (a cropped frame's lost rows read zero)
        raw.append((_frame_of(frames[0, b, :Hs, :Ws], h, w).astype(np.float32), _frame_of(frames[1, b, :Hs, :Ws], h, w).astype(np.float32)))
        flow[b, :h, :w] = _field(rs, h, w) if b != 2 else 0.0            # sample 2: an all-zero flow (a white picture)
        pred, g, mo, mn = _kitti_like_error_case(rs, h, w)
        if b != 2:
            g = (flow[b, :h, :w] - (pred - g)).astype(np.float32)        # the same error distribution around this flow
        gt_flow[0, b, :Hs, :Ws] = resize_image_with_crop_or_pad(g, Hs, Ws)
        gt_mask[0, b, :Hs, :Ws] = resize_image_with_crop_or_pad(mo, Hs, Ws)[..., 0]
        gt_mask[1, b, :Hs, :Ws] = resize_image_with_crop_or_pad(mn, Hs, Ws)[..., 0]
        gts.append(tuple(_frame_of(x, h, w) for x in (gt_flow[0, b, :Hs, :Ws], gt_mask[0, b, :Hs, :Ws, None], gt_mask[1, b, :Hs, :Ws, None])))
    desc_np = pack_desc(sizes, B, staged=(Hs, Ws), nmaps=2, u8=u8)
    to = lambda a: torch.from_numpy(a).to(dev)            # noqa: E731
    fd, dd, fl, gf, gm = to(frames), to(desc_np), to(flow), to(gt_flow), to(gt_mask)
    out8, outf, _ = _run_visual(fd, dd, fl, gf, gm, B, Hm, Wm, H, W, dev)
    again8, againf, _ = _run_visual(fd, dd, fl, gf, gm, B, Hm, Wm, H, W, dev)
    assert np.array_equal(out8, again8) and np.array_equal(outf, againf)
    only8, _, _ = _run_visual(fd, dd, fl, gf, gm, B, Hm, Wm, H, W, dev, with_f32=False)
    assert np.array_equal(only8, out8)
    for b, (h, w) in enumerate(sizes):
        if h == 0:
            assert (out8[:, b] == 7).all() and (outf[:, b] == -3.0).all()
            continue
        hh = min(h, Hm)                                   # a frame taller than its row would be cut, never written past it
        assert (out8[:, b, hh:] == 7).all() and (out8[:, b, :hh, w:] == 7).all()      # nothing outside the frame
        assert (outf[:, b, hh:] == -3.0).all() and (outf[:, b, :hh, w:] == -3.0).all()
        f = flow[b, :h, :w]
        tag = "%s %dx%d" % ('uint8' if u8 else 'fp32', h, w)
        assert np.array_equal(out8[:, b, :h, :w], R.to_bytes(outf[:, b, :h, :w])), tag
        # overlay, brightness error: bit-identical to the chained launches, and close to the fp64 mirror
        c_over, c_diff = _chained(raw[b][0], raw[b][1], f, H, W, dev)
        assert np.array_equal(outf[0, b, :h, :w], c_over), (tag, float(np.abs(outf[0, b, :h, :w] - c_over).max()))
        assert np.array_equal(outf[1, b, :h, :w], c_diff), (tag, float(np.abs(outf[1, b, :h, :w] - c_diff).max()))
        r_over, r_diff = R.overlay_and_diff(raw[b][0], raw[b][1], f, H, W)
        _close(outf[0, b, :h, :w], r_over, "overlay " + tag)
        _close(outf[1, b, :h, :w], r_diff, "brightness error " + tag)
        _bytes_within_one(out8[0, b, :h, :w], r_over, "overlay " + tag)
        _bytes_within_one(out8[1, b, :h, :w], r_diff, "brightness error " + tag)
        # flow colours, max_flow of this sample alone
        r_col = R.flow_to_color(f)
        _close(outf[2, b, :h, :w], r_col, "flow colours " + tag)
        _bytes_within_one(out8[2, b, :h, :w], r_col, "flow colours " + tag)
        if b == 2:
            assert (out8[2, b, :h, :w] == 255).all()
        # ground truth: the error image and the ground truth's colours
        g, mo, mn = gts[b]
        _check_error_bytes(out8[3, b, :h, :w], f, g, mo, mn, "error image " + tag)
        r_gt = R.flow_to_color(g, mask=mo)
        _close(outf[4, b, :h, :w], r_gt, "gt colours " + tag)
        _bytes_within_one(out8[4, b, :h, :w], r_gt, "gt colours " + tag)
    # one ground-truth map: mask_noc = ones; none: the last two images are not written
    d1 = to(pack_desc(sizes, B, staged=(Hs, Ws), nmaps=1, u8=u8))
    one8, _, _ = _run_visual(fd, d1, fl, gf, gm, B, Hm, Wm, H, W, dev, with_f32=False)
    h, w = sizes[0]
    _check_error_bytes(one8[3, 0, :h, :w], flow[0, :h, :w], gts[0][0], gts[0][1], np.ones_like(gts[0][1]), "error image, one map")
    assert np.array_equal(one8[[0, 1, 2, 4]], out8[[0, 1, 2, 4]])
    d0 = to(pack_desc(sizes, B, staged=(Hs, Ws), nmaps=0, u8=u8))
    for args in ((d0, gf, gm), (dd, None, None)):
        no8, _, _ = _run_visual(fd, args[0], fl, args[1], args[2], B, Hm, Wm, H, W, dev, with_f32=False)
        assert np.array_equal(no8[:3], out8[:3]) and (no8[3:] == 7).all()


def test_inference_visual_raw_frames_at_the_origin(dev):
    """estimate()'s layout: raw frames at the origin of their rows (desc y0 = x0 = 0), a network smaller than the frames."""
    from unflow_amd.core.inference import pack_desc
    H, W = 128, 192
    Hm, Wm = 160, 256
    sizes = [(150, 250), (97, 203), (160, 256)]
    B = len(sizes)
    rs = np.random.RandomState(21)
    frames = np.zeros((2, B, Hm, Wm, 3), np.float32)
    flow = np.zeros((B, Hm, Wm, 2), np.float32)
    for b, (h, w) in enumerate(sizes):
        frames[0, b, :h, :w] = rs.rand(h, w, 3) * 255.0
        frames[1, b, :h, :w] = rs.rand(h, w, 3) * 255.0
        flow[b, :h, :w] = _field(rs, h, w)
    to = lambda a: torch.from_numpy(a).to(dev)            # noqa: E731
    out8, outf, _ = _run_visual(to(frames), to(pack_desc(sizes, B)), to(flow), None, None, B, Hm, Wm, H, W, dev)
    for b, (h, w) in enumerate(sizes):
        c_over, c_diff = _chained(frames[0, b, :h, :w], frames[1, b, :h, :w], flow[b, :h, :w], H, W, dev)
        assert np.array_equal(outf[0, b, :h, :w], c_over) and np.array_equal(outf[1, b, :h, :w], c_diff)
        r_over, r_diff = R.overlay_and_diff(frames[0, b, :h, :w], frames[1, b, :h, :w], flow[b, :h, :w], H, W)
        _close(outf[0, b, :h, :w], r_over, "overlay %dx%d" % (h, w))
        _close(outf[1, b, :h, :w], r_diff, "brightness error %dx%d" % (h, w))
        assert (out8[:3, b, h:] == 7).all() and (out8[:3, b, :h, w:] == 7).all() and (out8[3:] == 7).all()


# ------------------------------------------------------------------------------------------------------ the estimator
def _batches(rs, sizes_list, Hs, Ws, nmaps=2):
    from unflow_amd.core.input import resize_image_with_crop_or_pad
    out = []
    for sizes in sizes_list:
        cols = [[] for _ in range(3 + 2 * nmaps)]
        for h, w in sizes:
            a = rs.randint(0, 256, size=(h, w, 3)).astype(np.float32)
            b = np.roll(a, (1, -2), (0, 1))
            vals = [resize_image_with_crop_or_pad(a, Hs, Ws), resize_image_with_crop_or_pad(b, Hs, Ws), np.array([h, w, 3], np.int32)]
            for k in range(nmaps):
                vals.append(resize_image_with_crop_or_pad((rs.randn(h, w, 2) * 3).astype(np.float32), Hs, Ws))
                vals.append(resize_image_with_crop_or_pad((rs.rand(h, w, 1) < 0.5 + 0.2 * k).astype(np.float32), Hs, Ws))
            for c, v in zip(cols, vals):
                c.append(v)
        out.append(tuple(np.stack(c) for c in cols))
    return out


def _same_pictures(a, b, keys=None):
    """Two lists of picture dicts are equal (on `keys`: the images both must hold); reports where they are not."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if keys is None:
            assert list(x) == list(y)
        for k in keys or x:
            diff = (x[k] != y[k]).any(-1)
            assert not diff.any(), "example %d, %s: %d pixels differ, first at %s" % (i, k, int(diff.sum()), np.argwhere(diff)[0])


def test_estimator_visual_graph_vs_eager_mixed_sizes_short_last_batch(dev):
    from unflow_amd.core.inference import VISUAL_IMAGES, FlowEstimator
    params = dict(flownet='C')
    B, Hs, Ws = 3, 384, 1280
    rs = np.random.RandomState(11)
    batches = _batches(rs, [KITTI_SIZES, [KITTI_SIZES[2], KITTI_SIZES[0], KITTI_SIZES[1]], [KITTI_SIZES[1], KITTI_SIZES[2]]], Hs, Ws)
    ests = [FlowEstimator(params, B, device=dev, use_graph=g, visual=True) for g in (True, False)]
    plain = FlowEstimator(params, B, device=dev)
    tfp = ests[0].engine.init_params(seed=4)
    for e in ests + [plain]:
        e.load_tf_params(tfp)
    assert plain.vis is None and plain.vis_shown is None and not plain.visual
    for e in ests:
        e.vis.fill_(7)                                   # nothing is written outside the frames (checked below)
    pics = [list(e.pictures(iter(batches))) for e in ests]
    assert len(pics[0]) == 8 and all(list(p) == list(VISUAL_IMAGES) for p in pics[0])
    sizes = [s for grp in (KITTI_SIZES, [KITTI_SIZES[2], KITTI_SIZES[0], KITTI_SIZES[1]], [KITTI_SIZES[1], KITTI_SIZES[2]]) for s in grp]
    assert [p['flow'].shape for p in pics[0]] == [s + (3,) for s in sizes]
    _same_pictures(pics[0], pics[1])                     # graph replay against eager launches
    assert ests[0].graph is not None and ests[1].graph is None
    g0 = ests[0].graph
    _same_pictures(pics[0], list(ests[0].pictures(iter(batches))))       # and a second pass of replays
    assert ests[0].graph is g0
    for e in ests:
        v = e.vis.cpu().numpy()
        hmax, wmax = max(s[0] for s in KITTI_SIZES), max(s[1] for s in KITTI_SIZES)
        assert (v[:, :, hmax:] == 7).all() and (v[:, :, :, wmax:] == 7).all()
    # test-split input (no ground truth): three pictures
    nogt = [b[:3] for b in batches]
    p3 = list(ests[0].pictures(iter(nogt)))
    assert all(list(p) == list(VISUAL_IMAGES[:3]) for p in p3)
    _same_pictures(p3, pics[0], keys=VISUAL_IMAGES[:3])
    # raw pairs through visualize: float32 and uint8 frames, the pictures of the KITTIInput layout
    f1 = [b[0][i] for b in batches for i in range(len(b[0]))][:5]
    f2 = [b[1][i] for b in batches for i in range(len(b[1]))][:5]
    vis = [e.visualize(f1, f2) for e in ests]
    vis8 = ests[0].visualize([a.astype(np.uint8) for a in f1], [a.astype(np.uint8) for a in f2])
    assert ests[0].graph is g0
    for a, b, c in zip(vis[0], vis[1], vis8):
        assert a._fields == ('overlay', 'warp_error', 'flow')
        for x, y, z in zip(a, b, c):
            assert x.dtype == np.uint8 and x.shape == (Hs, Ws, 3)
            assert np.array_equal(x, y) and np.array_equal(x, z)
    # visual=True changes nothing else: flows and scores bit-equal to the plain estimator
    fl_v, fl_p = ests[0].estimate(f1, f2), plain.estimate(f1, f2)
    assert all(np.array_equal(a, b) for a, b in zip(fl_v, fl_p))
    res_v, res_p = ests[0].evaluate(iter(batches)), plain.evaluate(iter(batches))
    assert res_v['per_example'] == res_p['per_example'] and res_v['names'] == res_p['names']
    assert ests[0].graph is g0
    with pytest.raises(RuntimeError, match="visual=True"):
        plain.visualize(f1[:1], f2[:1])
    with pytest.raises(RuntimeError, match="visual=True"):
        next(plain.pictures(iter(batches)))
    # the estimator's pictures against the mirror, fed the flow read back from the GPU
    H, W = 384, 1280
    for i in (0, 3):
        f = fl_v[i]
        r_over, r_diff = R.overlay_and_diff(f1[i], f2[i], f, H, W)
        _bytes_within_one(vis[0][i].overlay, r_over, "estimator overlay %d" % i)
        _bytes_within_one(vis[0][i].warp_error, r_diff, "estimator brightness error %d" % i)
        _bytes_within_one(vis[0][i].flow, R.flow_to_color(f), "estimator flow colours %d" % i)


def test_bidirectional_visual_estimator(dev):
    """visual=True on a bidirectional estimator: the pictures follow the occlusion kernel in the same graph, and are those of
    the one-direction estimator wherever the forward flow is bit-equal."""
    from unflow_amd.core.inference import FlowEstimator
    params = dict(flownet='C')
    rs = np.random.RandomState(13)
    f1 = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in KITTI_SIZES]
    f2 = [np.roll(a, (1, -2), (0, 1)) for a in f1]
    bi = FlowEstimator(params, 2, device=dev, bidirectional=True, visual=True)
    tfp = bi.engine.init_params(seed=8)
    bi.load_tf_params(tfp)
    ref = FlowEstimator(params, 2, device=dev, bidirectional=True)
    ref.load_tf_params(tfp)
    got, want = bi.estimate_bidirectional(f1, f2), ref.estimate_bidirectional(f1, f2)
    for a, b in zip(got, want):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    vis = bi.visualize(f1, f2)
    for v, r, a, b in zip(vis, got, f1, f2):
        _bytes_within_one(v.flow, R.flow_to_color(r.flow_fw), "bidirectional flow colours")
        r_over, r_diff = R.overlay_and_diff(a, b, r.flow_fw, 384, 1280)
        _bytes_within_one(v.warp_error, r_diff, "bidirectional brightness error")
        _bytes_within_one(v.overlay, r_over, "bidirectional overlay")


def test_end_to_end_kitti_export_visual_and_cli(dev, tmp_path):
    from unflow_amd import visualize as V
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import decode_png, save_checkpoint
    from unflow_amd.kitti.input import KITTIInput
    written = make_tree(tmp_path / "kitti", n_pairs=5)
    params = dict(flownet='C')
    est = FlowEstimator(params, 2, device=dev, visual=True)
    tfp = est.engine.init_params(seed=3)
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    est.load_tf_params(tfp)
    einput = KITTIInput(Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(384, 1280))
    dec = lambda p: decode_png(open(p, 'rb').read())      # noqa: E731
    vis = est.visualize([ex[0] for ex in written], [ex[1] for ex in written])
    pics = list(est.pictures(einput.input_train_2012()))
    flows = est.estimate([ex[0] for ex in written], [ex[1] for ex in written])
    out = str(tmp_path / "out")
    paths = est.export(einput.input_train_2012(), out, fmt='png', visual=True)
    tags = ('%06d_10.png', '%06d_img.png', '%06d_flow.png', '%06d_diff.png', '%06d_err.png', '%06d_gt.png')
    assert [os.path.basename(p) for p in paths] == [n % i for i in range(5) for n in tags]
    for i, (v, pc, ex) in enumerate(zip(vis, pics, written)):
        p = paths[6 * i:6 * i + 6]
        assert np.array_equal(dec(p[1]), v.overlay) and np.array_equal(dec(p[2]), v.flow) and np.array_equal(dec(p[3]), v.warp_error)
        assert np.array_equal(dec(p[4]), pc['error']) and np.array_equal(dec(p[5]), pc['gt'])
        assert all(np.array_equal(pc[k], getattr(v, k)) for k in v._fields)
        # the ground-truth pictures against the mirror: the flow read back from the GPU, the maps as written
        _check_error_bytes(pc['error'], flows[i], ex[2], ex[3], ex[5], "exported error image %d" % i)
        _bytes_within_one(pc['gt'], R.flow_to_color(ex[2], mask=ex[3]), "exported gt colours %d" % i)
    # without visual=True the files are what they were
    ppaths = est.export(einput.input_train_2012(), str(tmp_path / "plain"), fmt='png', num=2)
    assert [os.path.basename(p) for p in ppaths] == ['000000_10.png', '000001_10.png']
    one = FlowEstimator(params, 2, device=dev)
    with pytest.raises(ValueError, match="visual=True"):
        one.export(einput.input_train_2012(), str(tmp_path / "x"), visual=True)
    # the CLI: an experiment folder with its config and checkpoint
    ck = tmp_path / "ckpt" / "ex1"
    ck.mkdir(parents=True)
    save_checkpoint(str(ck / "model.ckpt-7"), tfp, 7)
    with open(ck / "checkpoint", "w") as f:
        f.write('model_checkpoint_path: "model.ckpt-7"\n')
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\ndata = %s\n\n[train]\nflownet = C\n"
                   % (tmp_path / "log", tmp_path / "ckpt", tmp_path / "kitti"))
    root = str(tmp_path / "cli")
    assert V.main(['--ex', 'ex1', '--config', str(cfg), '--out', root, '--num', '-1', '--batch_size', '2', '--sheet',
                   '--num_vis', '5']) == 0
    names = sorted(os.listdir(os.path.join(root, 'ex1')))
    want = sorted(['config.ini', 'page_000.png', 'page_001.png'] + [n % i for i in range(5) for n in tags[1:]])
    assert names == want
    for i, pc in enumerate(pics):
        for k, tag in (('overlay', 'img'), ('flow', 'flow'), ('warp_error', 'diff'), ('error', 'err'), ('gt', 'gt')):
            assert np.array_equal(dec(os.path.join(root, 'ex1', '%06d_%s.png' % (i, tag))), pc[k]), (i, k)
    sheet = dec(os.path.join(root, 'ex1', 'page_000.png'))
    assert np.array_equal(sheet, V.contact_sheet([[pc[c] for c in V.SHEET_COLUMNS[True]] for pc in pics[:4]]))
    assert sheet.shape == (4 * 376, 5 * 1242, 3)
    sheet1 = dec(os.path.join(root, 'ex1', 'page_001.png'))
    assert np.array_equal(sheet1, V.contact_sheet([[pics[4][c] for c in V.SHEET_COLUMNS[True]]]))
