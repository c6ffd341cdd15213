"""-m gpu: visual sequence mode — unflow_sequence_visual against unflow_inference_visual on the same pairs, bit for bit; the
clip-wide max_flow; the two pictures of bidirectional mode; FlowEstimator(..., sequence=..., visual='sequence') against the pair
kernel fed its own flows, graph against eager, short pushes, reset; export through the three file paths and the command line.

Bounds: everything here is an equality (bytes, or fp32 bit patterns) except the backward flow's colours against the fp64 mirror,
which keep tests/test_visual_gpu.py's derived constants: 1e-5 on the continuous image, bytes at most one level off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import visual_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_TOL = 1e-5                                          # tests/test_visual_gpu.py
B3, HM, WM, H, W = 3, 96, 160, 64, 128


def _lib():
    from unflow_amd import _lib as L
    return L


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flow(rs, zero=False):
    """A staged flow [HM][WM][2]: junk everywhere (what lies outside the frame must not be read), exact zeros and u == 0 inside."""
    f = (rs.randn(HM, WM, 2) * 6.0).astype(np.float32)
    f[:, 5] = 0.0
    f[:, 11::40, 0] = 0.0
    f[7::30, :, 1] = 0.0
    f[40:44, 60:90] = rs.randn(4, 30, 2).astype(np.float32) * 300.0
    if zero:
        f[:] = 0.0
    return f


def _clip_frames(rs, T, h, w, u8):
    fr = []
    for _ in range(T):
        a = rs.randint(0, 256, size=(h, w, 3)).astype(np.float32)
        if not u8:
            a += rs.rand(h, w, 3).astype(np.float32) * 0.5
        fr.append(a.astype(np.uint8 if u8 else np.float32))
    return fr


class _Seq:
    """The buffers of unflow_sequence_visual, kept from launch to launch as an estimator keeps them."""

    def __init__(self, dev, u8, bidir=False):
        self.dev, self.u8, self.bidir = dev, u8, bidir
        self.shown = torch.full((B3 + 1, HM, WM, 4), -5.0, device=dev)
        self.bits = torch.zeros(3 * B3, dtype=torch.int32, device=dev)

    def launch(self, new_frames, h, w, carry, flow, flow_bw=None, occ=None, max_flow=None):
        from unflow_amd.core.inference import sequence_tables
        L = _lib()
        k = len(new_frames)
        staged = np.full((B3, HM, WM, 3), 9, np.uint8 if self.u8 else np.float32)      # unused slots: bytes that must not be read
        for i, a in enumerate(new_frames):
            staged[i, :h, :w] = a
        tab, valid, _ = sequence_tables((h, w), k, B3, carry, self.u8, max_flow)
        to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)   # noqa: E731
        out8 = torch.full((5, B3, HM, WM, 3), 7, dtype=torch.uint8, device=self.dev)
        outf = torch.full((5, B3, HM, WM, 3), -3.0, device=self.dev)
        fr, tb, fl, fb, oc = to(staged), to(tab), to(flow), to(flow_bw), to(occ)
        L.check(L.lib().unflow_sequence_visual(L.ptr(fr), L.ptr(tb), B3, HM, WM, H, W, L.ptr(fl), L.ptr(fb), L.ptr(oc),
                                               L.ptr(self.shown), L.ptr(self.bits), L.ptr(out8), L.ptr(outf), L.stream()),
                "sequence_visual")
        torch.cuda.synchronize()
        assert (self.bits == 0).all()                     # the slots and the tickets clean themselves
        return out8.cpu().numpy(), outf.cpu().numpy(), self.shown.cpu().numpy(), tab, valid


def _pair_kernel(firsts, seconds, h, w, u8, flow, desc, dev):
    """unflow_inference_visual on pairs staged [2][B]: slot i = (firsts[i], seconds[i]) or None; desc: the [B][8] table."""
    L = _lib()
    staged = np.zeros((2, B3, HM, WM, 3), np.uint8 if u8 else np.float32)
    for i in range(B3):
        if firsts[i] is not None:
            staged[0, i, :h, :w] = firsts[i]
            staged[1, i, :h, :w] = seconds[i]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    out8 = torch.full((5, B3, HM, WM, 3), 7, dtype=torch.uint8, device=dev)
    outf = torch.full((5, B3, HM, WM, 3), -3.0, device=dev)
    shown = torch.zeros(2, B3, HM, WM, 4, device=dev)
    bits = torch.zeros(3 * B3, dtype=torch.int32, device=dev)
    fr, dd, fl = to(staged), to(desc), to(flow)
    L.check(L.lib().unflow_inference_visual(L.ptr(fr), L.ptr(dd), B3, HM, WM, H, W, L.ptr(fl), None, None, L.ptr(shown), L.ptr(bits),
                                            L.ptr(out8), L.ptr(outf), L.stream()), "inference_visual")
    torch.cuda.synchronize()
    assert (bits == 0).all()
    return out8.cpu().numpy(), outf.cpu().numpy(), shown.cpu().numpy()


def _check_launch(got, ref, valid, h, w, images=3):
    """Valid pairs: images [0, images) equal the reference's, bytes and fp32 bits; everything else keeps its sentinel."""
    out8, outf = got[0], got[1]
    r8, rf = ref[0], ref[1]
    for i in range(B3):
        if i not in valid:
            assert (out8[:, i] == 7).all() and (outf[:, i] == -3.0).all(), i
            continue
        assert (out8[:, i, h:] == 7).all() and (out8[:, i, :h, w:] == 7).all(), i
        assert (outf[:, i, h:] == -3.0).all() and (outf[:, i, :h, w:] == -3.0).all(), i
        assert (out8[images:, i] == 7).all() and (outf[images:, i] == -3.0).all(), i
        for k in range(3):
            assert np.array_equal(out8[k, i, :h, :w], r8[k, i, :h, :w]), (i, k)
            assert np.array_equal(_bits(outf[k, i, :h, :w]), _bits(rf[k, i, :h, :w])), (i, k)
        assert np.array_equal(out8[:images, i, :h, :w], R.to_bytes(outf[:images, i, :h, :w])), i


# ------------------------------------------------------------------------------------------------- 1. against the pair kernel
@pytest.mark.parametrize("h,w", [(90, 151), (64, 128)], ids=['90x151', 'net-size'])
@pytest.mark.parametrize("u8", [True, False], ids=['uint8', 'fp32'])
def test_kernel_equals_the_pair_kernel_bit_for_bit(u8, h, w, dev):
    rs = np.random.RandomState(17 + int(u8))
    f = _clip_frames(rs, 4, h, w, u8)
    flow1 = np.stack([_flow(rs), _flow(rs), _flow(rs, zero=True)])
    flow2 = np.stack([_flow(rs), _flow(rs), _flow(rs)])
    seq = _Seq(dev, u8)
    # launch one: three new frames, nothing carried -> pairs (f0, f1), (f1, f2) in slots 1, 2; slot 0 has no first frame
    g1 = seq.launch(f[:3], h, w, 0, flow1)
    tab1, valid1 = g1[3], g1[4]
    assert valid1 == [1, 2]
    r1 = _pair_kernel([None, f[0], f[1]], [None, f[1], f[2]], h, w, u8, flow1, tab1[8 * B3:16 * B3].reshape(B3, 8), dev)
    _check_launch(g1, r1, valid1, h, w)
    assert (g1[0][2, 2, :h, :w] == 255).all()             # the all-zero flow: a white picture
    sh1 = g1[2]
    assert (sh1[0] == -5.0).all()                         # carry source 0: row 0 is not written
    for j in range(3):                                    # frame slot j -> row j + 1, the pair kernel's shown frames
        assert (sh1[j + 1, h:] == -5.0).all() and (sh1[j + 1, :h, w:] == -5.0).all()
    assert np.array_equal(_bits(sh1[2, :h, :w]), _bits(r1[2][1, 1, :h, :w])) and np.array_equal(_bits(sh1[2, :h, :w]), _bits(r1[2][0, 2, :h, :w]))
    assert np.array_equal(_bits(sh1[1, :h, :w]), _bits(r1[2][0, 1, :h, :w])) and np.array_equal(_bits(sh1[3, :h, :w]), _bits(r1[2][1, 2, :h, :w]))
    if (h, w) == (H, W) and u8:                           # both resizes are the identity
        assert np.array_equal(sh1[1, :h, :w, :3], f[0].astype(np.float32))
    # launch two, a short batch: one new frame, row 3 carried -> pair (f2, f3) in slot 0
    g2 = seq.launch(f[3:], h, w, 3, flow2)
    tab2, valid2 = g2[3], g2[4]
    assert valid2 == [0]
    r2 = _pair_kernel([f[2], None, None], [f[3], None, None], h, w, u8, flow2, tab2[8 * B3:16 * B3].reshape(B3, 8), dev)
    _check_launch(g2, r2, valid2, h, w)
    sh2 = g2[2]
    assert np.array_equal(_bits(sh2[0]), _bits(sh1[3]))   # the carried row, whole
    assert np.array_equal(_bits(sh2[2:]), _bits(sh1[2:]))  # rows beyond k + 1: untouched
    assert np.array_equal(_bits(sh2[1, :h, :w]), _bits(r2[2][1, 0, :h, :w]))
    assert (sh2[1, h:] == -5.0).all() and (sh2[1, :h, w:] == -5.0).all()
    # the same launch again on the same buffers: the same output
    g3 = seq.launch(f[3:], h, w, 3, flow2)
    assert np.array_equal(g3[0], g2[0]) and np.array_equal(_bits(g3[1]), _bits(g2[1])) and np.array_equal(_bits(g3[2]), _bits(g2[2]))


# ------------------------------------------------------------------------------------------------- 2. the clip's maximum
def test_clip_max_flow_colours_every_pair_alike(dev):
    from unflow_amd.core import flow_util
    h, w, u8 = 90, 151, True
    rs = np.random.RandomState(23)
    f = _clip_frames(rs, 3, h, w, u8)
    flow = np.stack([_flow(rs), _flow(rs), _flow(rs)])
    for given, used in ((20.0, 20.0), (0.25, 1.0)):
        seq = _Seq(dev, u8)
        out8, outf, _, tab, valid = seq.launch(f, h, w, 0, flow, max_flow=given)     # bits == 0 asserted inside: no maxima formed
        assert valid == [1, 2] and tab[16 * B3 + 1:16 * B3 + 2].view(np.float32)[0] == np.float32(used)
        for i in valid:
            win = torch.from_numpy(np.ascontiguousarray(flow[i, :h, :w])[None]).to(dev)
            want8 = flow_util.flow_to_color(win, max_flow=used, uint8=True)[0].cpu().numpy()
            wantf = flow_util.flow_to_color(win, max_flow=used)[0].cpu().numpy()
            assert np.array_equal(out8[2, i, :h, :w], want8), (given, i)
            assert np.array_equal(_bits(outf[2, i, :h, :w]), _bits(wantf)), (given, i)
        # the other pictures do not depend on it
        ref = _Seq(dev, u8).launch(f, h, w, 0, flow)
        assert np.array_equal(out8[:2], ref[0][:2]) and not np.array_equal(out8[2], ref[0][2])


# ------------------------------------------------------------------------------------------------- 3. both directions
def test_backward_colours_and_non_occluded_error(dev):
    from unflow_amd.core import flow_util
    h, w, u8 = 90, 151, False
    rs = np.random.RandomState(29)
    f = _clip_frames(rs, 3, h, w, u8)
    flow = np.stack([_flow(rs), _flow(rs), _flow(rs)])
    bw = np.stack([_flow(rs), _flow(rs), _flow(rs)]) * np.float32(0.5)
    occ = (rs.rand(B3, HM, WM) < 0.3).astype(np.uint8)
    out8, outf, _, tab, valid = _Seq(dev, u8, True).launch(f, h, w, 0, flow, bw, occ)
    one = _Seq(dev, u8).launch(f, h, w, 0, flow)
    assert valid == [1, 2]
    assert np.array_equal(out8[:3], one[0][:3]) and np.array_equal(_bits(outf[:3]), _bits(one[1][:3]))
    assert (out8[:, 0] == 7).all() and (outf[:, 0] == -3.0).all()
    for i in valid:
        assert (out8[:, i, h:] == 7).all() and (out8[:, i, :h, w:] == 7).all()
        assert (outf[:, i, h:] == -3.0).all() and (outf[:, i, :h, w:] == -3.0).all()
        win = torch.from_numpy(np.ascontiguousarray(bw[i, :h, :w])[None]).to(dev)
        want8 = flow_util.flow_to_color(win, uint8=True)[0].cpu().numpy()             # the pair's own maximum
        wantf = flow_util.flow_to_color(win)[0].cpu().numpy()
        assert np.array_equal(out8[3, i, :h, :w], want8), i
        assert np.array_equal(_bits(outf[3, i, :h, :w]), _bits(wantf)), i
        mirror = R.flow_to_color(bw[i, :h, :w])
        err = float(np.abs(outf[3, i, :h, :w].astype(np.float64) - mirror).max())
        d = np.abs(out8[3, i, :h, :w].astype(np.int16) - R.to_bytes(mirror).astype(np.int16))
        print("backward colours, pair slot %d: max |kernel - fp64 mirror| = %.3g, bytes off by at most %d" % (i, err, int(d.max())))
        assert err <= FLOAT_TOL and d.max() <= 1, (i, err, int(d.max()))
        o = occ[i, :h, :w, None] != 0
        assert o.any() and not o.all()
        assert np.array_equal(out8[4, i, :h, :w], np.where(o, np.uint8(0), out8[1, i, :h, :w])), i
        assert np.array_equal(_bits(outf[4, i, :h, :w]), _bits(np.where(o, np.float32(0.0), outf[1, i, :h, :w]))), i
    # a clip-wide maximum colours the backward flow as well
    o20 = _Seq(dev, u8, True).launch(f, h, w, 0, flow, bw, occ, max_flow=20.0)[0]
    win = torch.from_numpy(np.ascontiguousarray(bw[1, :h, :w])[None]).to(dev)
    assert np.array_equal(o20[3, 1, :h, :w], flow_util.flow_to_color(win, max_flow=20.0, uint8=True)[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------- 4. the estimator
FH, FW = 90, 151
_TFP = {}


def clip(T, h, w, seed):
    """tests/test_sequence_gpu.py's uint8 clip: every frame is the one before shifted, attenuated, plus noise."""
    g = torch.Generator().manual_seed(seed)
    fr = [torch.rand(h, w, 3, generator=g) * 255]
    for _ in range(T - 1):
        fr.append(torch.roll(fr[-1], shifts=(2, -3), dims=(0, 1)) * 0.9 + torch.rand(h, w, 3, generator=g) * 25)
    return [np.clip(np.rint(f.numpy()), 0, 255).astype(np.uint8) for f in fr]


def _estimator(dev, B, **kw):
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=(FH, FW), device=dev, **kw)
    if not _TFP:
        tfp = est.engine.init_params(seed=31)
        _TFP.update({k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v).cpu() for k, v in tfp.items()})
    est.load_tf_params(_TFP)
    return est


def _pair_pictures(first, second, flow, dev):
    """unflow_inference_visual on one pair with the given frame-size flow: the three pictures as bytes."""
    from unflow_amd.core.inference import pack_desc
    L = _lib()
    h, w = first.shape[:2]
    staged = np.zeros((2, 1, FH, FW, 3), np.uint8)
    staged[0, 0, :h, :w], staged[1, 0, :h, :w] = first, second
    fl = np.zeros((1, FH, FW, 2), np.float32)
    fl[0, :h, :w] = flow
    to = lambda a: torch.from_numpy(a).to(dev)            # noqa: E731
    fr, dd, fd = to(staged), to(pack_desc([(h, w)], 1, u8=True)), to(fl)
    out8 = torch.zeros(5, 1, FH, FW, 3, dtype=torch.uint8, device=dev)
    shown = torch.zeros(2, 1, FH, FW, 4, device=dev)
    bits = torch.zeros(3, dtype=torch.int32, device=dev)
    L.check(L.lib().unflow_inference_visual(L.ptr(fr), L.ptr(dd), 1, FH, FW, H, W, L.ptr(fd), None, None, L.ptr(shown), L.ptr(bits),
                                            L.ptr(out8), None, L.stream()), "inference_visual")
    torch.cuda.synchronize()
    return [out8[k, 0, :h, :w].cpu().numpy() for k in range(3)]


def _same(a, b):
    assert len(a) == len(b)
    for n, (x, y) in enumerate(zip(a, b)):
        assert type(x) is type(y) and len(x) == len(y)
        for name, p, q in zip(x._fields, x, y):
            assert p.dtype == np.uint8 and p.shape == (FH, FW, 3) and np.array_equal(p, q), (n, name)


def test_estimator_pictures_equal_the_pair_kernel_on_its_own_flows(dev):
    from unflow_amd.core.inference import FlowVisual
    T = 5
    frames = clip(T, FH, FW, 33)
    est = _estimator(dev, 2, sequence=True, visual='sequence')
    assert est.vis.shape == (5, 2, FH, FW, 3) and est.vis_shown.numel() == 3 * FH * FW * 4 and est.vis_max.numel() == 6
    flows = est.estimate_sequence(frames)                 # replays of 2, 2, 1 frames: a carry after a full and after a short batch
    vis = est.visualize_sequence(frames)
    assert len(vis) == T - 1 and all(type(v) is FlowVisual for v in vis)
    assert max(float(np.abs(f).max()) for f in flows) > 0.05
    for n, v in enumerate(vis):
        want = _pair_pictures(frames[n], frames[n + 1], flows[n], dev)
        for name, got, ref in zip(v._fields, v, want):
            assert got.dtype == np.uint8 and np.array_equal(got, ref), (n, name, int((got != ref).sum()))
    g = est.graph
    _same(vis, est.visualize_sequence(iter(frames)))      # reset() inside: the same clip, the same pictures
    est.reset()
    _same(vis[:1], est.push_visual(frames[:2]))
    assert est.graph is g and g is not None
    eager = _estimator(dev, 2, sequence=True, visual='sequence', use_graph=False)
    _same(vis, eager.visualize_sequence(frames))
    assert eager.graph is None
    # the flows are those of the estimator without pictures, and push / estimate_sequence return what they did
    plain = _estimator(dev, 2, sequence=True)
    assert plain.vis is None and plain.vis_shown is None and plain.vis_max is None
    pf = plain.estimate_sequence(frames)
    assert len(pf) == len(flows) and all(np.array_equal(a, b) for a, b in zip(pf, flows))
    # the clip's max_flow: set by the first push, fixed until reset()
    est.reset()
    assert est.push_visual(frames[:1], max_flow=20) == []
    one = est.push_visual(frames[1:2], max_flow=20.0) + est.push_visual(frames[2:3])
    with pytest.raises(ValueError, match="max_flow"):
        est.push_visual(frames[3:4], max_flow=10)
    whole = est.visualize_sequence(frames, max_flow=20)
    _same(one, whole[:2])
    assert not np.array_equal(whole[0].flow, vis[0].flow) and np.array_equal(whole[0].warp_error, vis[0].warp_error)
    est.reset()
    est.push_visual(frames[:2])
    with pytest.raises(ValueError, match="max_flow"):
        est.push_visual(frames[2:3], max_flow=20)
    # the guards name the constructor flag
    with pytest.raises(RuntimeError, match="visual='sequence'"):
        plain.push_visual(frames[:2])
    with pytest.raises(RuntimeError, match="visual='sequence'"):
        plain.visualize_sequence(frames)
    with pytest.raises(ValueError, match="visual='sequence'"):
        plain.export_sequence(frames, "unused", visual=True)
    # visual=True stays the pair estimator's flag: with sequence it raises as before and names the spelling; and the reverse
    for seq in (True, 'bidirectional'):
        with pytest.raises(ValueError, match="visual='sequence'"):
            _estimator(dev, 2, sequence=seq, visual=True)
    with pytest.raises(ValueError, match="sequence=True"):
        _estimator(dev, 2, visual='sequence')
    with pytest.raises(ValueError, match="visual"):
        _estimator(dev, 2, sequence=True, visual='clip')
    with pytest.raises(RuntimeError, match="sequence"):
        est.visualize(frames[:1], frames[1:2])


def test_estimator_short_pushes_equal_the_whole_clip(dev):
    frames = clip(8, FH, FW, 34)
    est = _estimator(dev, 3, sequence=True, visual='sequence')
    whole = est.visualize_sequence(frames)
    assert len(whole) == 7
    est.reset()
    got, n0 = [], 0
    for k, want in ((2, 1), (3, 3), (1, 1), (2, 2)):
        out = est.push_visual(frames[n0:n0 + k])
        assert len(out) == want
        got += out
        n0 += k
    _same(got, whole)
    pair = _estimator(dev, 3, visual=True)
    with pytest.raises(RuntimeError, match="sequence=True"):
        pair.push_visual(frames[:2])
    with pytest.raises(RuntimeError, match="sequence=True"):
        pair.visualize_sequence(frames)


def test_bidirectional_estimator_pictures(dev):
    from unflow_amd.core import flow_util
    from unflow_amd.core.inference import SequenceVisual
    T = 5
    frames = clip(T, FH, FW, 33)
    bi = _estimator(dev, 2, sequence='bidirectional', visual='sequence')
    both = bi.estimate_sequence_bidirectional(frames)
    vis = bi.visualize_sequence(frames)
    assert len(vis) == T - 1 and all(type(v) is SequenceVisual for v in vis)
    assert SequenceVisual._fields == ('overlay', 'warp_error', 'flow', 'flow_bw', 'warp_error_noc')
    some_occ = False
    for n, (v, r) in enumerate(zip(vis, both)):
        want = _pair_pictures(frames[n], frames[n + 1], r.flow_fw, dev)
        for name, got, ref in zip(v._fields[:3], v[:3], want):
            assert np.array_equal(got, ref), (n, name)
        fb = torch.from_numpy(np.ascontiguousarray(r.flow_bw)[None]).to(dev)
        assert np.array_equal(v.flow_bw, flow_util.flow_to_color(fb, uint8=True)[0].cpu().numpy()), n
        assert np.array_equal(v.warp_error_noc, np.where(r.occ_fw[..., None], np.uint8(0), v.warp_error)), n
        some_occ = some_occ or bool(r.occ_fw.any())
    print("bidirectional pictures: occluded pixels in the clip: %s" % some_occ)
    _same(vis, bi.visualize_sequence(frames))
    flows = bi.estimate_sequence(frames)                  # the one-direction methods return what they did
    assert all(np.array_equal(a, b.flow_fw) for a, b in zip(flows, both))


# ------------------------------------------------------------------------------------------------- 5. files and the command
def test_export_sequence_visual_and_cli(dev, tmp_path):
    from unflow_amd.core.inference import FlowEstimator, sequence_visual_files
    from unflow_amd.core.input import decode_png, save_checkpoint, write_png_rgb8
    T = 5
    frames = clip(T, FH, FW, 50)
    fdir = tmp_path / "frames"
    fdir.mkdir()
    for i, f in enumerate(frames):
        write_png_rgb8(str(fdir / ("f%03d.png" % i)), f)
    bi = _estimator(dev, 2, sequence='bidirectional', visual='sequence')
    ck = tmp_path / "ckpts" / "clipnet"
    ck.mkdir(parents=True)
    save_checkpoint(str(ck / "model.ckpt-7"), _TFP, 7)
    with open(ck / "checkpoint", "w") as f:
        f.write('model_checkpoint_path: "model.ckpt-7"\n')
    dec = lambda p: decode_png(open(p, 'rb').read())      # noqa: E731
    names = lambda paths: [os.path.basename(p) for p in paths]   # noqa: E731
    vis = bi.visualize_sequence(frames, max_flow=20)
    kw = dict(fmt='png', backward=True, occlusion=True, visual=True, max_flow=20)
    host = bi.export_sequence(frames, str(tmp_path / "host"), **kw)
    per_pair = ['%06d_10.png', '%06d_01.png', '%06d_10_occ.png', '%06d_img.png', '%06d_flow.png', '%06d_diff.png', '%06d_flow_bw.png',
                '%06d_diff_noc.png']
    assert names(host) == [n % i for i in range(T - 1) for n in per_pair]
    assert [n for _, n in sequence_visual_files(2, True)] == [n % 2 for n in per_pair[3:]]
    for i, v in enumerate(vis):
        p = host[8 * i + 3:8 * i + 8]
        for path, img in zip(p, (v.overlay, v.flow, v.warp_error, v.flow_bw, v.warp_error_noc)):
            assert np.array_equal(dec(path), img), path
    pool = bi.export_sequence(frames, str(tmp_path / "pool"), workers=2, **kw)
    devz = bi.export_sequence(frames, str(tmp_path / "devz"), workers=2, deflate='device', **kw)
    assert names(pool) == names(host) and names(devz) == names(host)
    for a, b, c in zip(host, pool, devz):
        x = dec(a)
        assert np.array_equal(x, dec(b)) and np.array_equal(x, dec(c)), os.path.basename(a)
    # the flow files are those of an export without the pictures, byte for byte
    plain = bi.export_sequence(frames, str(tmp_path / "plain"), fmt='png', backward=True, occlusion=True)
    assert names(plain) == [n % i for i in range(T - 1) for n in per_pair[:3]]
    for p in plain:
        with open(p, 'rb') as fa, open(os.path.join(str(tmp_path / "host"), os.path.basename(p)), 'rb') as fb:
            assert fa.read() == fb.read(), p
    with pytest.raises(ValueError, match="visual=True"):
        bi.export_sequence(frames, str(tmp_path / "x"), max_flow=20)
    # the command line, as a child process: one direction, the pictures beside the flow files
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp_path / "log", tmp_path / "ckpts"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', str(fdir), '--out',
                        str(tmp_path / "cli"), '--visual', '--max_flow', '20', '--batch', '2', '--net_size', str(H), str(W),
                        '--config', str(cfg)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cli_dir = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(cli_dir)) == sorted(n % i for i in range(T - 1) for n in (per_pair[:1] + per_pair[3:6]))
    one = FlowEstimator.from_checkpoint(str(ck), dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence=True, visual='sequence')
    ref = one.export_sequence(frames, str(tmp_path / "one"), fmt='png', visual=True, max_flow=20)
    assert sorted(names(ref)) == sorted(os.listdir(cli_dir))
    for p in ref:
        assert np.array_equal(dec(p), dec(os.path.join(cli_dir, os.path.basename(p)))), p
