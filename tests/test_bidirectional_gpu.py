"""-m gpu: bidirectional inference — the bidirectional inference engine against the fp64 oracle and its memory, the occlusion
kernel against losses.occlusion's chained ops and numpy counts, the backward output against the chained resize, graph against
eager, and FlowEstimator's bidirectional evaluate / export end to end on a KITTI-format tree."""
import os

import numpy as np
import pytest
import torch

from kitti_fixture import Data, make_tree
from parity_util import images

pytestmark = pytest.mark.gpu

CHANNEL_MEAN = [104.920005, 110.1753, 114.785955]
KITTI_SIZES = [(370, 1226), (375, 1242), (376, 1241)]
# = test_inference_gpu.ORACLE_CASES
ORACLE_CASES = [('C', 2, 128, 192, {}), ('S', 2, 128, 192, {}), ('CSS', 1, 64, 128, {}), ('css', 1, 128, 192, {}),
                ('S', 1, 64, 128, dict(full_res=True)), ('C', 1, 384, 1280, {}), ('C', 8, 384, 1280, {})]


def _lib():
    from unflow_amd import _lib as L
    return L


@pytest.mark.parametrize("spec,B,H,W,extra", ORACLE_CASES,
                         ids=['C', 'S', 'CSS', 'css', 'S-full_res', 'C-kitti-B1', 'C-kitti-B8'])
def test_bidirectional_engine_flows_vs_fp64_oracle(spec, B, H, W, extra, dev):
    from unflow_amd.core.engine import FlowNetEngine, conv_math_mode, flow_error_avg
    from oracle import model_ref as M
    params = dict(flownet=spec, **extra)
    eng = FlowNetEngine(B, H, W, params=params, device=dev, seed=None, inference=True, bidirectional=True)
    tfp = eng.init_params(seed=31)
    if len(spec) > 1:
        tfp = {k: (v * 0.3 if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v) for k, v in tfp.items()}
        eng.load_tf_params(tfp)
    im1, im2 = images(B, H, W, 32)
    eng.set_input(im1, im2)
    eng.forward_net()
    fw, bw = eng.final_flows()
    torch.cuda.synchronize()
    assert fw.shape == (B, H, W, 2) and bw.shape == (B, H, W, 2)
    mean = torch.tensor(CHANNEL_MEAN) / 255.0
    tf64 = {k: v.double() for k, v in tfp.items()}
    full_res = bool(extra.get('full_res'))
    ref_fw, ref_bw = M.flownet(tf64, (im1 / 255.0 - mean).double(), (im2 / 255.0 - mean).double(), spec, backward_flow=True,
                               full_resolution=full_res)
    bound = 5e-2 if conv_math_mode() == 'f16' else 1e-3
    for got, ref in ((fw, ref_fw[-1][0]), (bw, ref_bw[-1][0])):
        ref_final = ref * 20 if full_res else M.resize_bilinear_tf1(ref, H, W) * 20
        epe = flow_error_avg(got, ref_final.float().to(dev)).item()
        assert epe < bound, (spec, epe)
    fl, bl = eng.flows()
    assert all(f.shape[0] == B for f in fl) and all(f.shape[0] == B for f in bl)


def test_bidirectional_engine_memory(dev):
    """No G / M / V / Gd, and less device memory than the default (training) engine of the same shape."""
    from unflow_amd.core.engine import FlowNetEngine
    B, H, W = 4, 384, 1280

    def built(**kw):
        import gc
        gc.collect()
        torch.cuda.synchronize()
        a = torch.cuda.memory_allocated(dev)
        e = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=None, **kw)
        torch.cuda.synchronize()
        return e, torch.cuda.memory_allocated(dev) - a
    bi, m_bi = built(inference=True, bidirectional=True)
    assert bi.G is None and bi.M is None and bi.V is None and bi.im01 is None
    assert all(not st.Gd and not st.trainable for st in bi.stages)
    assert bi.final_flow.shape[0] == 2 * B
    del bi
    tr, m_tr = built()
    print("engine memory: bidirectional inference %.1f MB, training %.1f MB" % (m_bi / 1e6, m_tr / 1e6))
    assert m_bi < m_tr, (m_bi, m_tr)


def _smooth_pair(rs, Hm, Wm):
    """A forward field and a backward field that mostly cancels it (a mix of occluded and visible pixels), displacements of
    tens of pixels (many taps clamp at the frame edges) and a block of far-out vectors."""
    yy, xx = np.mgrid[0:Hm, 0:Wm].astype(np.float32)
    u = 30.0 * np.sin(xx / 50.0) + 10.0
    v = 8.0 * np.cos(yy / 40.0) - 3.0
    base = np.stack([u, v], 2)
    fw = base + rs.randn(Hm, Wm, 2).astype(np.float32) * 0.4
    bw = -base + rs.randn(Hm, Wm, 2).astype(np.float32) * 0.4
    occ = rs.rand(Hm, Wm) < 0.2
    fw[occ] += rs.randn(int(occ.sum()), 2).astype(np.float32) * 25.0
    fw[10:40, 100:300] = rs.randn(30, 200, 2).astype(np.float32) * 5000.0
    bw[50:60, :] = rs.randn(10, Wm, 2).astype(np.float32) * 3000.0
    return fw.astype(np.float32), bw.astype(np.float32)


def _run_occlusion(fw, bw, desc, B, Hm, Wm, gt_mask):
    L = _lib()
    occ = torch.full((2, B, Hm, Wm), 7, dtype=torch.uint8, device=fw.device)
    counts = torch.full((B, 3), 99, dtype=torch.int32, device=fw.device)
    L.check(L.lib().unflow_inference_occlusion(L.ptr(fw), L.ptr(bw), L.ptr(desc), B, Hm, Wm, L.ptr(gt_mask), L.ptr(occ[0]),
                                               L.ptr(occ[1]), L.ptr(counts), L.stream()), "inference_occlusion")
    torch.cuda.synchronize()
    return occ.cpu().numpy(), counts.cpu().numpy()


def _np_counts(o_fw, m_occ, m_noc):
    ev = m_occ == 1
    gocc = ev & (m_noc == 0)
    return [int((o_fw & gocc).sum()), int((o_fw & ev & ~gocc).sum()), int((~o_fw & gocc).sum())]


def _frame_gt(gt_mask, b, desc_row, Hm, Wm):
    """Both GT maps of sample b at its frame pixels (zero outside the staging buffer), as the kernel reads them."""
    h, w, y0, x0 = (int(v) for v in desc_row[:4])
    r, c = np.arange(h)[:, None] + y0, np.arange(w)[None, :] + x0
    ok = (r >= 0) & (r < Hm) & (c >= 0) & (c < Wm)
    rc, cc = np.clip(r, 0, Hm - 1), np.clip(c, 0, Wm - 1)
    return [np.where(ok, gt_mask[k, b][rc, cc], 0.0) for k in range(2)]


def test_occlusion_kernel_vs_chained_ops_and_counts(dev):
    from unflow_amd.core import losses
    from unflow_amd.core.inference import pack_desc
    Hs, Ws = 384, 1280                       # the KITTIInput layout: frames padded into it, GT at the frames' origins
    Hm, Wm = 448, 1280
    sizes = KITTI_SIZES + [(97, 203), (0, 0), (384, 1280)]
    B = len(sizes)
    rs = np.random.RandomState(7)
    fw = np.zeros((B, Hm, Wm, 2), np.float32)
    bw = np.zeros((B, Hm, Wm, 2), np.float32)
    for b in range(B):
        fw[b], bw[b] = _smooth_pair(rs, Hm, Wm)
    gt = np.zeros((2, B, Hm, Wm), np.float32)
    gt[0] = (rs.rand(B, Hm, Wm) < 0.6).astype(np.float32)                         # mask_occ
    gt[1] = gt[0] * (rs.rand(B, Hm, Wm) < 0.7).astype(np.float32)                 # mask_noc within it
    desc_np = pack_desc(sizes, B, staged=(Hs, Ws), nmaps=2)
    fwd, bwd = torch.from_numpy(fw).to(dev), torch.from_numpy(bw).to(dev)
    desc, gtd = torch.from_numpy(desc_np).to(dev), torch.from_numpy(gt).to(dev)
    occ, counts = _run_occlusion(fwd, bwd, desc, B, Hm, Wm, gtd)
    occ2, counts2 = _run_occlusion(fwd, bwd, desc, B, Hm, Wm, gtd)
    assert np.array_equal(occ, occ2) and np.array_equal(counts, counts2)
    n_clamped, frac = 0, []
    for b, (h, w) in enumerate(sizes):
        if h == 0:
            assert (occ[:, b] == 7).all() and (counts[b] == 0).all()
            continue
        ref_fw, ref_bw = losses.occlusion(fwd[b:b + 1, :h, :w].contiguous(), bwd[b:b + 1, :h, :w].contiguous())
        torch.cuda.synchronize()
        r_fw = ref_fw[0, ..., 0].cpu().numpy().astype(np.uint8)
        r_bw = ref_bw[0, ..., 0].cpu().numpy().astype(np.uint8)
        assert np.array_equal(occ[0, b, :h, :w], r_fw), (sizes[b], int((occ[0, b, :h, :w] != r_fw).sum()))
        assert np.array_equal(occ[1, b, :h, :w], r_bw), (sizes[b], int((occ[1, b, :h, :w] != r_bw).sum()))
        assert (occ[:, b, h:] == 7).all() and (occ[:, b, :h, w:] == 7).all()      # nothing outside the frame
        frac.append(r_fw.mean())
        yy, xx = np.mgrid[0:h, 0:w]
        tx, ty = xx + np.floor(fw[b, :h, :w, 0]), yy + np.floor(fw[b, :h, :w, 1])
        n_clamped += int(((tx < 0) | (tx + 1 >= w) | (ty < 0) | (ty + 1 >= h)).sum())
        m_occ, m_noc = _frame_gt(gt, b, desc_np[b], Hm, Wm)
        assert list(counts[b]) == _np_counts(occ[0, b, :h, :w].astype(bool), m_occ, m_noc), sizes[b]
    assert 0.05 < min(frac) and max(frac) < 0.95, frac        # both outcomes are exercised
    assert n_clamped > 10000, n_clamped
    # no ground truth staged (nmaps = 0): the same masks, zero counts
    desc0 = torch.from_numpy(pack_desc(sizes, B, staged=(Hs, Ws), nmaps=0)).to(dev)
    occ0, counts0 = _run_occlusion(fwd, bwd, desc0, B, Hm, Wm, gtd)
    assert np.array_equal(occ0, occ) and (counts0 == 0).all()


def test_backward_output_vs_chained_resize(dev):
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import flow_to_int16
    L = _lib()
    H, W = 384, 1280
    est = FlowEstimator(dict(flownet='C'), 3, device=dev, bidirectional=True)
    est.engine.init_params(seed=6)
    est._params_changed()
    rs = np.random.RandomState(2)
    f1 = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in KITTI_SIZES]
    f2 = [np.roll(a, (1, -2), (0, 1)) for a in f1]
    got = est.estimate_bidirectional(f1, f2)
    fw, bw = est.engine.final_flows()
    torch.cuda.synchronize()
    out_fw, out_bw = est.out_flow.cpu(), est.out_flow_bw.cpu()
    u16_bw = est.out_u16_bw.cpu().numpy().view(np.uint16)
    for i, (h, w) in enumerate(KITTI_SIZES):
        for mid, out, ret in ((fw[i:i + 1], out_fw, got[i].flow_fw), (bw[i:i + 1], out_bw, got[i].flow_bw)):
            r = torch.zeros(1, h, w, 2, device=dev)
            L.check(L.lib().unflow_resize_bilinear_tf1(L.ptr(mid.contiguous()), L.ptr(r), 1, H, W, 2, h, w, L.cf(1.0),
                                                       L.stream()), "resize")
            torch.cuda.synchronize()
            r = r.cpu()
            ref = torch.stack([r[..., 0] * np.float32(w / W), r[..., 1] * np.float32(h / H)], 3)[0]
            assert torch.equal(out[i, :h, :w], ref), (i, (out[i, :h, :w] - ref).abs().max().item())
            assert np.array_equal(ret, ref.numpy())
        assert np.array_equal(u16_bw[i, :h, :w], flow_to_int16(got[i].flow_bw))
        assert got[i].occ_fw.dtype == np.bool_ and got[i].occ_fw.shape == (h, w) and got[i].occ_bw.shape == (h, w)


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


def test_bidirectional_graph_vs_eager_mixed_sizes_short_last_batch(dev):
    from unflow_amd.core.inference import FlowEstimator
    params = dict(flownet='C')
    B, Hs, Ws = 3, 384, 1280
    rs = np.random.RandomState(11)
    batches = _batches(rs, [KITTI_SIZES, [KITTI_SIZES[2], KITTI_SIZES[0], KITTI_SIZES[1]], [KITTI_SIZES[1], KITTI_SIZES[2]]],
                       Hs, Ws)
    ests = [FlowEstimator(params, B, device=dev, use_graph=g, bidirectional=True) for g in (True, False)]
    tfp = ests[0].engine.init_params(seed=4)
    for e in ests:
        e.load_tf_params(tfp)
    res = [e.evaluate(iter(batches)) for e in ests]
    assert res[0]['num_examples'] == 8 and len(res[0]['occ_counts']) == 8
    assert res[0]['per_example'] == res[1]['per_example'] and res[0]['occ_counts'] == res[1]['occ_counts']
    assert all(res[0][k] == res[1][k] for k in ('occ/precision', 'occ/recall', 'occ/F1'))
    assert ests[0].graph is not None and ests[1].graph is None
    g0 = ests[0].graph
    f1 = [b[0][i] for b in batches for i in range(len(b[0]))][:5]
    f2 = [b[1][i] for b in batches for i in range(len(b[1]))][:5]
    outs = [e.estimate_bidirectional(f1, f2) for e in ests]
    assert ests[0].graph is g0                           # no re-capture
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    # uint8 frames: the same result; the forward flow is estimate()'s of the same estimator
    u8 = ests[0].estimate_bidirectional([a.astype(np.uint8) for a in f1], [a.astype(np.uint8) for a in f2])
    for a, b in zip(outs[0], u8):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    fl = ests[0].estimate(f1, f2)
    assert ests[0].graph is g0
    for a, f in zip(outs[0], fl):
        assert np.array_equal(a.flow_fw, f)
    occ_frac = np.mean([a.occ_fw.mean() for a in outs[0]])
    print("occluded fraction (random weights): %.3f" % occ_frac)


def test_end_to_end_kitti_evaluate_export_bidirectional(dev, tmp_path):
    from unflow_amd.core.inference import FlowEstimator, occlusion_scores
    from unflow_amd.core.input import flow_to_int16, read_flo, read_kitti_flow_png, read_png_image
    from unflow_amd.kitti.input import KITTIInput
    written = make_tree(tmp_path / "kitti", n_pairs=5)
    params = dict(flownet='C')
    est = FlowEstimator(params, 2, device=dev, bidirectional=True)
    tfp = est.engine.init_params(seed=3)
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    est.load_tf_params(tfp)
    one = FlowEstimator(params, 2, device=dev)
    one.load_tf_params(tfp)
    einput = KITTIInput(Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(384, 1280))
    res = est.evaluate(einput.input_train_2012())
    ref = one.evaluate(einput.input_train_2012())
    occ_keys = {'occ/precision', 'occ/recall', 'occ/F1', 'occ_counts'}
    assert set(res) == set(ref) | occ_keys and not occ_keys & set(ref)
    assert res['names'] == ref['names'] and res['num_examples'] == ref['num_examples'] == 5
    for a, b in zip(res['per_example'], ref['per_example']):
        assert abs(a[0] - b[0]) < 1e-3 and abs(a[2] - b[2]) < 1e-3, (a, b)
    bi = est.estimate_bidirectional([ex[0] for ex in written], [ex[1] for ex in written])
    cnt = [_np_counts(r.occ_fw, ex[3][..., 0], ex[5][..., 0]) for r, ex in zip(bi, written)]
    assert res['occ_counts'] == cnt
    sc = occlusion_scores(cnt)
    assert all(res[k] == sc[k] for k in sc)
    print("occlusion scores (random weights):", {k: round(v, 2) for k, v in sc.items()})
    # export: _10, _01 and _10_occ per example; the files decode to what estimate_bidirectional returns
    out = str(tmp_path / "out")
    paths = est.export(einput.input_train_2012(), out, fmt='png', backward=True, occlusion=True)
    assert [os.path.basename(p) for p in paths] == [n % i for i in range(5) for n in ('%06d_10.png', '%06d_01.png', '%06d_10_occ.png')]
    for i, r in enumerate(bi):
        for p, f in ((paths[3 * i], r.flow_fw), (paths[3 * i + 1], r.flow_bw)):
            back, mask = read_kitti_flow_png(p)
            q = flow_to_int16(f)[..., :2]
            assert np.array_equal(back.numpy(), (q.astype(np.float32) - 2 ** 15) / 64.0)
            assert (mask.numpy() == 1).all()
        img = read_png_image(paths[3 * i + 2])
        assert np.array_equal(img[..., 0], r.occ_fw.astype(np.float32) * 255)
    fpaths = est.export(einput.input_train_2012(), str(tmp_path / "flo"), fmt='flo', backward=True)
    assert [os.path.basename(p) for p in fpaths] == [n % i for i in range(5) for n in ('%06d_10.flo', '%06d_01.flo')]
    for i, r in enumerate(bi):
        assert np.array_equal(read_flo(fpaths[2 * i])[0].numpy(), r.flow_fw)
        assert np.array_equal(read_flo(fpaths[2 * i + 1])[0].numpy(), r.flow_bw)
    # a one-direction estimator: no backward flow, no occlusion
    with pytest.raises(RuntimeError, match="bidirectional"):
        one.estimate_bidirectional([written[0][0]], [written[0][1]])
    for kw in (dict(backward=True), dict(occlusion=True)):
        with pytest.raises(ValueError, match="bidirectional"):
            one.export(einput.input_train_2012(), str(tmp_path / "x"), **kw)
