"""-m gpu: forward-only inference — the input kernel against resize_input + unflow_prepare_image_pair, the output kernel against
the chained resizes, the KITTI encoding and fp64 metric sums, the inference engine against the fp64 oracle, its memory, graph
against eager, and FlowEstimator end to end on a KITTI-format tree (evaluate, export, checkpoint restore)."""
import os

import numpy as np
import pytest
import torch

from kitti_fixture import Data, make_tree
from parity_util import images

pytestmark = pytest.mark.gpu

CHANNEL_MEAN = [104.920005, 110.1753, 114.785955]
KITTI_SIZES = [(370, 1226), (375, 1242), (376, 1241)]


def _lib():
    from unflow_amd import _lib as L
    return L


def _run_input(frames, desc, B, Hm, Wm, H, W, pl=None):
    L = _lib()
    x0 = torch.full((2 * B, H, W, 4), 7.0, device=frames.device)
    mean = (L.ctypes.c_float * 3)(*CHANNEL_MEAN)
    L.check(L.lib().unflow_inference_input(L.ptr(frames), L.ptr(desc), B, Hm, Wm, H, W, L.ptr(x0), mean, L.planes_of(pl),
                                           L.stream()), "inference_input")
    torch.cuda.synchronize()
    return x0


def _prepared(im1, im2, H, W, dev):
    """resize_input's values through unflow_prepare_image_pair: the reference chain of the network input."""
    L = _lib()
    B = im1.shape[0]
    x0 = torch.zeros(2 * B, H, W, 4, device=dev)
    mean = (L.ctypes.c_float * 3)(*CHANNEL_MEAN)
    L.check(L.lib().unflow_prepare_image_pair(L.ptr(im1.contiguous()), L.ptr(im2.contiguous()), L.cl(B * H * W), L.ptr(x0),
                                              L.ptr(None), mean, None, L.stream()), "prepare")
    torch.cuda.synchronize()
    return x0


@pytest.mark.parametrize("u8", [False, True], ids=['fp32', 'uint8'])
def test_input_kernel_vs_resize_input_and_prepare(u8, dev):
    from unflow_amd.core.input import resize_image_with_crop_or_pad, resize_input
    from unflow_amd.core.inference import pack_desc
    from unflow_amd.core import layers as Lay
    H, W = 384, 1280
    Hs, Ws = 384, 1280                         # KITTIInput dims: frames cropped / padded to them
    sizes = KITTI_SIZES + [(436, 1024), (0, 0)]
    B = len(sizes)
    rs = np.random.RandomState(5)
    dt = np.uint8 if u8 else np.float32
    staged = np.zeros((2, B, Hs, Ws, 3), dt)
    refs = [[], []]
    for i, (h, w) in enumerate(sizes):
        for k in range(2):
            if h == 0:
                refs[k].append(torch.zeros(1, H, W, 3))
                continue
            fr = rs.randint(0, 256, size=(h, w, 3)).astype(np.float32)
            if not u8:
                fr += rs.rand(h, w, 3).astype(np.float32) * 0.5
            st = resize_image_with_crop_or_pad(fr, Hs, Ws)
            staged[k, i] = st.astype(dt)
            refs[k].append(resize_input(torch.from_numpy(st.astype(dt).astype(np.float32)).unsqueeze(0), h, w, H, W))
    desc = torch.from_numpy(pack_desc(sizes, B, staged=(Hs, Ws), u8=u8)).to(dev)
    frames = torch.from_numpy(staged).to(dev)
    pl = torch.zeros(3, 2 * B, H, W, 4, dtype=torch.int16, device=dev)
    got = _run_input(frames, desc, B, Hs, Ws, H, W, pl)
    ref = _prepared(torch.cat(refs[0]).to(dev), torch.cat(refs[1]).to(dev), H, W, dev)
    for i, (h, w) in enumerate(sizes):
        for k in range(2):
            r = k * B + i
            if h == 0:
                assert (got[r] == 0).all()
                continue
            err = (got[r] - ref[r]).abs().max().item()
            assert err <= 1e-6, (sizes[i], k, err)
    planes = torch.zeros_like(pl)
    Lay.planes_from_f32(got, planes, C=4)
    torch.cuda.synchronize()
    assert torch.equal(planes, pl)


def _run_output(flow, H, W, desc, B, Hm, Wm, gt=None, mask=None, scale=20.0):
    L = _lib()
    dev = flow.device
    out = torch.zeros(B, Hm, Wm, 2, device=dev)
    u16 = torch.zeros(B, Hm, Wm, 3, dtype=torch.int16, device=dev)
    nb = L.lib().unflow_inference_output_blocks(Hm, Wm)
    partial = torch.zeros(B * nb * 6, dtype=torch.float64, device=dev)
    ticket = torch.zeros(B, dtype=torch.int32, device=dev)
    sums = torch.zeros(B, 2, 2, dtype=torch.float64, device=dev)
    counts = torch.zeros(B, 2, dtype=torch.int32, device=dev)
    L.check(L.lib().unflow_inference_output(L.ptr(flow), flow.shape[1], flow.shape[2], L.cf(scale), H, W, L.ptr(desc), B, Hm, Wm,
                                            L.ptr(out), L.ptr(u16), L.ptr(gt), L.ptr(mask), L.ptr(partial), L.ptr(ticket),
                                            L.ptr(sums), L.ptr(counts), L.stream()), "inference_output")
    torch.cuda.synchronize()
    assert (ticket == 0).all()
    return out, u16, sums, counts


def _chained(flow, H, W, h, w, dev, scale=20.0):
    L = _lib()
    mid = torch.zeros(1, H, W, 2, device=dev)
    f = flow.contiguous()
    if f.shape[1] == H:
        L.check(L.lib().unflow_scale(L.ptr(f), L.cf(scale), L.ptr(mid), L.cl(f.numel()), L.stream()), "scale")
    else:
        L.check(L.lib().unflow_resize_bilinear_tf1(L.ptr(f), L.ptr(mid), 1, f.shape[1], f.shape[2], 2, H, W, L.cf(scale),
                                                   L.stream()), "resize")
    out = torch.zeros(1, h, w, 2, device=dev)
    L.check(L.lib().unflow_resize_bilinear_tf1(L.ptr(mid), L.ptr(out), 1, H, W, 2, h, w, L.cf(1.0), L.stream()), "resize")
    torch.cuda.synchronize()
    out = out.cpu()
    return torch.stack([out[..., 0] * np.float32(w / W), out[..., 1] * np.float32(h / H)], 3)[0], mid.cpu()


@pytest.mark.parametrize("full_res", [False, True], ids=['flow2', 'flow0'])
def test_output_kernel_bit_identical_to_chain_u16_and_metrics(full_res, dev):
    from unflow_amd.core.input import flow_to_int16, resize_output_flow, resize_image_with_crop_or_pad
    from unflow_amd.core.inference import pack_desc
    H, W = 384, 1280
    fh, fw = (H, W) if full_res else (H // 4, W // 4)
    Hs, Ws = 384, 1280                  # the KITTIInput layout, at the top left of staging rows of the largest frame
    Hm, Wm = 448, 1280
    sizes = KITTI_SIZES + [(436, 1024), (0, 0)]
    B = len(sizes)
    g = torch.Generator().manual_seed(9)
    flow = (torch.randn(B, fh, fw, 2, generator=g) * 0.4).to(dev)
    desc = torch.from_numpy(pack_desc(sizes, B, staged=(Hs, Ws), nmaps=2)).to(dev)
    rs = np.random.RandomState(3)
    gt = np.zeros((2, B, Hm, Wm, 2), np.float32)
    mk = np.zeros((2, B, Hm, Wm), np.float32)
    frame_gt = {}
    for i, (h, w) in enumerate(sizes):
        if h == 0:
            continue
        for k in range(2):
            f = (rs.randn(h, w, 2) * 6).astype(np.float32)
            m = (rs.rand(h, w) < 0.4 - 0.1 * k).astype(np.float32)
            gt[k, i, :Hs, :Ws] = resize_image_with_crop_or_pad(f, Hs, Ws)
            mk[k, i, :Hs, :Ws] = resize_image_with_crop_or_pad(m[..., None], Hs, Ws)[..., 0]
            # what resize_output_crop gives back at the frame's size
            frame_gt[i, k] = (resize_image_with_crop_or_pad(gt[k, i, :Hs, :Ws], h, w),
                              resize_image_with_crop_or_pad(mk[k, i, :Hs, :Ws][..., None], h, w)[..., 0])
    gtd, mkd = torch.from_numpy(gt).to(dev), torch.from_numpy(mk).to(dev)
    out, u16, sums, counts = _run_output(flow, H, W, desc, B, Hm, Wm, gtd, mkd)
    out2, u16b, sums2, counts2 = _run_output(flow, H, W, desc, B, Hm, Wm, gtd, mkd)
    assert torch.equal(out, out2) and torch.equal(u16, u16b) and torch.equal(sums, sums2) and torch.equal(counts, counts2)
    out, u16, sums, counts = out.cpu(), u16.cpu().numpy().view(np.uint16), sums.cpu().numpy(), counts.cpu().numpy()
    for i, (h, w) in enumerate(sizes):
        if h == 0:
            assert (sums[i] == 0).all() and (counts[i] == 0).all()
            continue
        ref, mid = _chained(flow[i:i + 1], H, W, h, w, dev)
        got = out[i, :h, :w]
        assert torch.equal(got, ref), (sizes[i], (got - ref).abs().max().item())
        # against the torch chain of Trainer.eval (resize_output_flow of final_flows())
        tref = resize_output_flow(mid, h, w)[0]
        assert (got - tref).abs().max().item() < 1e-4
        assert np.array_equal(u16[i, :h, :w], flow_to_int16(got.numpy()))
        f = got.numpy().astype(np.float64)
        for k in range(2):
            gk, mk_ = frame_gt[i, k]
            gk, mk_ = gk.astype(np.float64), mk_.astype(np.float64)
            d = np.sqrt(((gk - f) ** 2).sum(-1)) * mk_
            thr = np.maximum(np.sqrt((gk ** 2).sum(-1)) * 0.05, 3.0)
            assert abs(sums[i, k, 0] - d.sum()) <= 1e-6 * d.sum(), (i, k)
            assert sums[i, k, 1] == mk_.sum()
            near = np.abs(d - thr) < 1e-4
            n_ref = int((d >= thr).sum())
            assert abs(int(counts[i, k]) - n_ref) <= int(near.sum()), (i, k, counts[i, k], n_ref)


ORACLE_CASES = [('C', 2, 128, 192, {}), ('S', 2, 128, 192, {}), ('CSS', 1, 64, 128, {}), ('css', 1, 128, 192, {}),
                ('S', 1, 64, 128, dict(full_res=True)), ('C', 1, 384, 1280, {}), ('C', 8, 384, 1280, {})]


@pytest.mark.parametrize("spec,B,H,W,extra", ORACLE_CASES,
                         ids=['C', 'S', 'CSS', 'css', 'S-full_res', 'C-kitti-B1', 'C-kitti-B8'])
def test_inference_engine_flows_vs_fp64_oracle(spec, B, H, W, extra, dev):
    from unflow_amd.core.engine import FlowNetEngine, conv_math_mode, flow_error_avg
    from oracle import model_ref as M
    params = dict(flownet=spec, **extra)
    eng = FlowNetEngine(B, H, W, params=params, device=dev, seed=None, inference=True)
    tfp = eng.init_params(seed=31)
    if len(spec) > 1:
        tfp = {k: (v * 0.3 if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v) for k, v in tfp.items()}
        eng.load_tf_params(tfp)
    im1, im2 = images(B, H, W, 32)
    eng.set_input(im1, im2)
    eng.forward_net()
    fw, bw = eng.final_flows()
    torch.cuda.synchronize()
    assert bw is None and fw.shape == (B, H, W, 2)
    mean = torch.tensor(CHANNEL_MEAN) / 255.0
    tf64 = {k: v.double() for k, v in tfp.items()}
    ref = M.flownet(tf64, (im1 / 255.0 - mean).double(), (im2 / 255.0 - mean).double(), spec, backward_flow=False,
                    full_resolution=bool(extra.get('full_res')))
    last = ref[-1][0]
    if extra.get('full_res'):
        ref_final = last * 20
    else:
        ref_final = M.resize_bilinear_tf1(last, H, W) * 20
    bound = 5e-2 if conv_math_mode() == 'f16' else 1e-3
    epe = flow_error_avg(fw, ref_final.float().to(dev)).item()
    assert epe < bound, (spec, epe)
    fl, _ = eng.flows()
    assert all(f.shape[0] == B for f in fl)


def test_inference_engine_memory(dev):
    """No G / M / V / Gd, and at least the derived byte count below the supervised engine: 3 flat fp32 buffers of n_params,
    the activation gradients of the trained network (one fp32 tensor + planes per buffer) and the weight-plane layout the
    forward pass does not read."""
    from unflow_amd.core.engine import FlowNetEngine, round8
    B, H, W = 4, 384, 1280

    def built(**kw):
        import gc
        gc.collect()              # tensors of earlier tests freed now, not in the middle of the measurement
        torch.cuda.synchronize()
        a = torch.cuda.memory_allocated(dev)
        e = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=None, **kw)
        torch.cuda.synchronize()
        return e, torch.cuda.memory_allocated(dev) - a
    inf, m_inf = built(inference=True)
    sup, m_sup = built(supervised=True)
    assert inf.G is None and inf.M is None and inf.V is None
    assert all(not st.Gd for st in inf.stages) and all(st.Gd for st in sup.stages[-1:])
    derived = 3 * 4 * sup.n_params
    st = sup.stages[-1]
    derived += sum(pt.t.numel() * 4 + (0 if pt.pl is None else pt.pl.numel() * 2) for pt in st.Gd.values())
    if sup.n_planes:
        P = sup.n_planes
        for l in sup.layers:
            if l.uses_planes():
                taps, R, Cc = l.wplane_view()
                derived += 2 * P * (taps * R * round8(Cc) if l.kind == 'conv' else taps * Cc * round8(R))
    print("engine memory: inference %.1f MB, supervised %.1f MB, derived saving %.1f MB" % (m_inf / 1e6, m_sup / 1e6, derived / 1e6))
    assert m_sup - m_inf >= derived, (m_sup, m_inf, derived)


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
                vals.append(resize_image_with_crop_or_pad((rs.rand(h, w, 1) < 0.5).astype(np.float32), Hs, Ws))
            for c, v in zip(cols, vals):
                c.append(v)
        out.append(tuple(np.stack(c) for c in cols))
    return out


def test_graph_vs_eager_mixed_sizes_short_last_batch(dev):
    from unflow_amd.core.inference import FlowEstimator
    params = dict(flownet='C')
    B, Hs, Ws = 3, 384, 1280
    rs = np.random.RandomState(11)
    batches = _batches(rs, [KITTI_SIZES, [KITTI_SIZES[2], KITTI_SIZES[0], KITTI_SIZES[1]], [KITTI_SIZES[1], KITTI_SIZES[2]]],
                       Hs, Ws)
    ests = [FlowEstimator(params, B, device=dev, use_graph=g) for g in (True, False)]
    tfp = ests[0].engine.init_params(seed=4)
    ests[1].load_tf_params(tfp)
    ests[0].load_tf_params(tfp)
    res = [e.evaluate(iter(batches)) for e in ests]
    assert res[0]['num_examples'] == 8
    assert res[0]['per_example'] == res[1]['per_example']
    assert ests[0].graph is not None and ests[1].graph is None
    g0 = ests[0].graph
    f1 = [e.estimate([b[0][i] for b in batches for i in range(len(b[0]))][:5], [b[1][i] for b in batches for i in range(len(b[1]))][:5])
          for e in ests]
    assert ests[0].graph is g0                           # no re-capture
    for a, b in zip(*f1):
        assert np.array_equal(a, b)


def test_estimate_uint8_equals_float_and_raw_sizes(dev):
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(128, 192), max_frame=(160, 256), device=dev)
    est.engine.init_params(seed=6)
    est._params_changed()
    rs = np.random.RandomState(2)
    sizes = [(120, 200), (160, 256), (100, 150)]
    f1 = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in sizes]
    f2 = [np.roll(a, (1, 2), (0, 1)) for a in f1]
    a = est.estimate(f1, f2)
    b = est.estimate([x.astype(np.float32) for x in f1], [x.astype(np.float32) for x in f2])
    assert [x.shape for x in a] == [s + (2,) for s in sizes]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        est.estimate([np.zeros((200, 300, 3), np.uint8)], [np.zeros((200, 300, 3), np.uint8)])


def _oracle_eval(tf_params, params, example):
    """One example through the reference's evaluation chain with the oracle's pieces (tests/test_eval_gpu.py::_oracle_eval):
    AEE / outliers of both maps and the frame-size flow."""
    from oracle import model_ref as M
    im1, im2, flow_occ, mask_occ, flow_noc, mask_noc = [torch.from_numpy(np.ascontiguousarray(a)) for a in example]
    h, w = im1.shape[:2]
    a = M.resize_bilinear_tf1(im1.unsqueeze(0), 384, 1280)
    b = M.resize_bilinear_tf1(im2.unsqueeze(0), 384, 1280)
    with torch.no_grad():
        loss, ffw, _, _ = M.unsupervised_loss(tf_params, a, b, params, return_flow=True)
    f = M.resize_bilinear_tf1(ffw, h, w)
    f = torch.stack([f[..., 0] * (w / 1280.0), f[..., 1] * (h / 384.0)], 3)
    vals = []
    for gt, mask in ((flow_occ, mask_occ), (flow_noc, mask_noc)):
        gt, mask = gt.unsqueeze(0), mask.unsqueeze(0)
        d = ((gt - f) ** 2).sum(3, keepdim=True).sqrt() * mask
        thr = torch.clamp(((gt ** 2).sum(3, keepdim=True)).sqrt() * 0.05, min=3.0)
        vals += [(d.sum() / mask.sum()).item(), ((d >= thr).float().sum() / mask.sum()).item() * 100]
    return vals, f


def test_end_to_end_checkpoint_evaluate_export(dev, tmp_path):
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import read_kitti_flow_png
    from unflow_amd.core.train import Trainer
    from unflow_amd.kitti.input import KITTIInput
    written = make_tree(tmp_path / "kitti", n_pairs=5)
    params = dict(flownet='C', pyramid_loss=True, border_mask=True, ternary_weight=1.0, smooth_2nd_weight=3.0,
                  learning_rate=1e-4, save_interval=1, display_interval=1)
    tr = Trainer(1, 128, 192, params, device=dev, seed=3, augment=False)
    tfp = tr.engine.export_tf_params()
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    tr.engine.load_tf_params(tfp)
    ckpt_dir = str(tmp_path / "ckpt")
    tr.save(ckpt_dir, 7)
    einput = KITTIInput(Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(384, 1280))
    est = FlowEstimator.from_checkpoint(ckpt_dir, params, 2, device=dev)
    assert est.global_step == 7
    res = est.evaluate(einput.input_train_2012())
    assert res['num_examples'] == 5 and 'loss' not in res
    ref_rows = [_oracle_eval({k: v.cpu() for k, v in tfp.items()}, params, ex)[0] for ex in written]
    for got, ref in zip(res['per_example'], ref_rows):
        assert abs(got[0] - ref[0]) < 1e-3 and abs(got[2] - ref[2]) < 1e-3, (got, ref)
        assert abs(got[1] - ref[1]) < 0.05 and abs(got[3] - ref[3]) < 0.05, (got, ref)
    t_rows = tr.eval(lambda: KITTIInput(Data(tmp_path / "kitti"), batch_size=1, normalize=False,
                                        dims=(384, 1280)).input_train_2012(), ckpt_dir)['per_example']
    for got, ref in zip(res['per_example'], t_rows):
        assert abs(got[0] - ref[0]) < 1e-3 and abs(got[2] - ref[2]) < 1e-3, (got, ref)
        assert abs(got[1] - ref[1]) < 0.05 and abs(got[3] - ref[3]) < 0.05, (got, ref)
    for k, i in (('AEE/occluded', 0), ('outliers/occluded', 1), ('AEE/non-occluded', 2), ('outliers/non-occluded', 3)):
        assert abs(res[k] - np.mean([r[i] for r in res['per_example']])) < 1e-9
    # export: the files in example order, the kernel's flow quantised to 1/64
    out = str(tmp_path / "out")
    paths = est.export(einput.input_train_2012(), out, fmt='png')
    assert [os.path.basename(p) for p in paths] == ['%06d_10.png' % i for i in range(5)]
    flows = est.estimate([ex[0] for ex in written], [ex[1] for ex in written])
    for p, f in zip(paths, flows):
        back, mask = read_kitti_flow_png(p)
        q = np.clip(np.float32(f) * np.float32(64) + np.float32(32768), 0, 65535).astype(np.uint16)
        assert np.array_equal(back.numpy(), (q.astype(np.float32) - 2 ** 15) / 64.0)
        assert (mask.numpy() == 1).all()
    fpaths = est.export(einput.input_train_2012(), str(tmp_path / "flo"), fmt='flo')
    assert [os.path.basename(p) for p in fpaths] == ['%06d_10.flo' % i for i in range(5)]


def test_stacked_checkpoint_restores_frozen_networks_through_finetune(dev, tmp_path):
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import save_params_npz
    from unflow_amd.core.train import Trainer
    params = dict(flownet='CS', learning_rate=1e-4)
    tr = Trainer(1, 64, 128, params, device=dev, seed=5, augment=False)
    full = tr.engine.export_tf_params()
    c_file = str(tmp_path / "c.npz")
    save_params_npz(c_file, {k: v for k, v in full.items() if k.startswith('flownet_c')})
    ckpt_dir = str(tmp_path / "ckpt")
    tr.save(ckpt_dir, 3)                  # holds the last network only (the Saver's scope without train_all)
    with pytest.raises(ValueError, match="nothing to restore"):
        FlowEstimator.from_checkpoint(ckpt_dir, params, 1, net_size=(64, 128), device=dev)
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(params, finetune=[c_file]), 1, net_size=(64, 128), device=dev)
    got = est.engine.export_tf_params()
    assert all(torch.equal(got[k], full[k]) for k in full)
