"""GPU: unflow_supervised_geo_augment (csrc/augment_flow.hip) against the fp64 reference of tests/geo_augment_ref.py (comparator
and bounds proven by tests/test_geo_augment_cpu.py), against the kernels it fuses, and everything built on it: the engine's
geometric set_input, the trainer (eager = graph replay), the Sintel / Chairs device iterators and python -m unflow_amd.finetune."""
import os
import threading

import numpy as np
import pytest
import torch

import flo_fixture as F
import geo_augment_ref as R
from parity_util import images

pytestmark = pytest.mark.gpu
CHANNEL_MEAN = [104.920005, 110.1753, 114.785955]


def _run_kernel(dev, a, mode, draws=None):
    """The kernel on a case's inputs -> dict of host numpy outputs + the device im01 / x0."""
    from unflow_amd.core import augment as A
    from unflow_amd.core.engine import CHANNEL_MEAN as MEAN
    t = lambda k: torch.from_numpy(np.ascontiguousarray(a[k])).to(dev)
    B, H, W, _ = a['im1'].shape
    nan = float('nan')
    im01 = torch.full((2 * B, H, W, 3), nan, device=dev)
    x0 = torch.full((2 * B, H, W, 4), nan, device=dev)
    flow = torch.full((B, H, W, 2), nan, device=dev)
    mask = torch.full((B, H, W, 1), nan, device=dev)
    draws = A.identity_photometric(B) if draws is None else draws
    A.supervised_geo_augment(t('im1'), t('im2'), t('flow'), None if a.get('mask') is None else t('mask'), torch.from_numpy(a['mats']),
                             draws, im01, x0, flow, mask, gt_sampling=('bilinear', 'nearest')[mode], mean=MEAN)
    torch.cuda.synchronize()
    return dict(im01=im01.cpu().numpy(), x0=x0.cpu().numpy(), flow=flow.cpu().numpy(), mask=mask.cpu().numpy(), im01_dev=im01,
                x0_dev=x0, draws=draws)


def _prepare01(im1, im2):
    """unflow_prepare_image_pair's [0,1] images [2B,H,W,3] of two device batches in [0,255]."""
    from unflow_amd import _lib
    B, H, W, _ = im1.shape
    x0, im01 = torch.zeros(2 * B, H, W, 4, device=im1.device), torch.zeros(2 * B, H, W, 3, device=im1.device)
    mean = (_lib.ctypes.c_float * 3)(*CHANNEL_MEAN)
    _lib.check(_lib.lib().unflow_prepare_image_pair(_lib.ptr(im1), _lib.ptr(im2), _lib.cl(B * H * W), _lib.ptr(x0), _lib.ptr(im01), mean,
                                                    None, _lib.stream(im1.device)), "prepare_image_pair")
    return im01


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape,kind", R.CASES)
def test_kernel_vs_reference(shape, kind, mode, dev):
    from unflow_amd.core import augment as A
    from unflow_amd.core.engine import CHANNEL_MEAN as MEAN
    a, r = R.case_inputs(shape, kind), R.reference(shape, kind, mode)
    draws = R.photometric_draws(shape[0], 40 + shape[1]) if kind != 'identity' else None
    o = _run_kernel(dev, a, mode, draws)
    ferr, ierr = r.flow_err(o['flow']), r.image_err(o['im01'])
    print("case %s %s mode %d: flow err %.3e px (tol %.3e, yardstick %.3e), image err %.3e (tol %.3e), mask mismatches %d"
          % (shape, kind, mode, ferr, r.flow_tol, r.yard_flow_err, ierr, r.im_tol, r.mask_mismatches(o['mask'])))
    for k in ('im01', 'x0', 'flow', 'mask'):
        assert np.isfinite(o[k]).all(), k                 # the 1e10 / NaN under the holes reach no output
    assert r.mask_mismatches(o['mask']) == 0
    assert set(np.unique(o['mask'])) <= {0.0, 1.0}
    inval = o['mask'][..., 0] == 0
    assert F.same_bits(o['flow'][inval], np.zeros_like(o['flow'][inval]))        # +0 by selection
    assert ferr <= r.flow_tol
    assert ierr <= r.im_tol
    # x0: the photometric kernel on the kernel's own im01, bit for bit (pad channel zero)
    want = torch.full_like(o['x0_dev'], float('nan'))
    A.photometric(o['im01_dev'], o['draws'], out=want, mean=MEAN)
    torch.cuda.synchronize()
    assert torch.equal(want.view(torch.int32), o['x0_dev'].view(torch.int32))
    assert (o['x0'][..., 3] == 0).all()


def test_null_mask_and_unaligned_rows(dev):
    """mask_gt = NULL means all ones; ld_out = 3 and an odd float offset of the flow take the scalar store / load paths and
    give the same values."""
    from unflow_amd.core import augment as A
    shape, kind = (3, 37, 47), 'full'
    a = dict(R.case_inputs(shape, kind))
    ones = dict(a, mask=np.ones_like(a['mask']), flow=np.nan_to_num(a['flow'], nan=1.0, posinf=1.0, neginf=1.0))
    base = _run_kernel(dev, ones, 0)
    null = _run_kernel(dev, dict(ones, mask=None), 0)
    for k in ('im01', 'x0', 'flow', 'mask'):
        assert F.same_bits(base[k], null[k]), k
    B, H, W = shape
    t = lambda k: torch.from_numpy(np.ascontiguousarray(ones[k])).to(dev)
    store = torch.zeros(B * H * W * 2 + 1, device=dev)
    store[1:] = t('flow').reshape(-1)
    flow_in = store[1:].view(B, H, W, 2)                 # 4-byte aligned only
    out_store = torch.zeros(B * H * W * 2 + 1, device=dev)
    flow_out = out_store[1:].view(B, H, W, 2)
    im01, x3, mask = torch.zeros(2 * B, H, W, 3, device=dev), torch.zeros(2 * B, H, W, 3, device=dev), torch.zeros(B, H, W, 1, device=dev)
    assert flow_in.data_ptr() % 8 == 4
    A.supervised_geo_augment(t('im1'), t('im2'), flow_in, t('mask'), torch.from_numpy(ones['mats']), A.identity_photometric(B), im01,
                             x3, flow_out, mask, mean=CHANNEL_MEAN)
    torch.cuda.synchronize()
    assert F.same_bits(flow_out.cpu().numpy(), base['flow']) and F.same_bits(mask.cpu().numpy(), base['mask'])
    assert F.same_bits(im01.cpu().numpy(), base['im01']) and F.same_bits(x3.cpu().numpy(), base['x0'][..., :3])


@pytest.mark.parametrize("shape", [(4, 19, 45), (2, 333, 795)])
def test_im1_rows_vs_transformer(shape, dev):
    """Rows [0, B) of im01 against the existing path: transformer(prepare_image_pair's [0,1] image, theta_global).  Only the
    coordinate rounding differs (the pixel map against the normalised grid), so the image bound of the reference holds; pixels
    whose coordinate is within the margin of an integer are left out as there."""
    from unflow_amd.core import augment as A
    B, H, W = shape
    g = torch.Generator().manual_seed(77 + H)
    tg = A.draw_affine(B, horizontal_flipping=True, generator=g, **R.FULL_RANGES)
    tl = A.draw_affine(B, generator=g, **R.FULL_RANGES)
    im1, im2 = R.smooth_images(B, H, W, 5)
    flow, mask = R.noisy_gt(B, H, W, 5, holes=False)
    a = dict(im1=im1, im2=im2, flow=flow, mask=mask, mats=A.affine_pixel_maps(tg, tl, H, W).numpy())
    r = R.Reference(a, 0)
    assert r.shares['im1'] <= R.CAP
    o = _run_kernel(dev, a, 0)
    want = A.transformer(_prepare01(torch.from_numpy(im1).to(dev), torch.from_numpy(im2).to(dev))[:B], tg).cpu().numpy()
    d = np.abs(o['im01'][:B].astype(np.float64) - want).max(-1)[~r.ex_im1].max()
    print("im1 rows vs transformer %s: %.3e (tol %.3e)" % (shape, d, r.im_tol))
    assert d <= r.im_tol
    assert r.image_err(o['im01']) <= r.im_tol


def test_integer_translation(dev):
    """M1 = M2 = a shift by whole pixels: the images are the shifted inputs exactly, the flow is the shifted flow up to the
    rounding of (p + d + f) - d - p, and the mask is the shifted mask wherever the 2 x 2 footprint that `valid` asks for holds no
    hole (a hole among the four taps invalidates the pixel even at weight zero: the definition's rule), away from the last
    row and column that `inside` drops."""
    B, H, W = 3, 23, 38
    dx, dy = np.array([3.0, -2.0, 0.0]), np.array([-1.0, 4.0, 2.0])
    g = np.random.RandomState(8)
    im1 = g.randint(0, 256, size=(B, H, W, 3)).astype(np.float32)
    im2 = g.randint(0, 256, size=(B, H, W, 3)).astype(np.float32)
    flow, mask = R.noisy_gt(B, H, W, 9)
    a = dict(im1=im1, im2=im2, flow=flow, mask=mask, mats=R.whole_pixel_mats(B, H, W, dx=dx, dy=dy))
    o = _run_kernel(dev, a, 0)
    for b in range(B):
        ox, oy = int(dx[b]), int(dy[b])
        ys, xs = np.arange(H), np.arange(W)
        # output pixels whose source and its right / lower neighbour lie inside: what `inside` keeps
        yy = ys[(ys + oy >= 0) & (ys + oy + 1 <= H - 1)]
        xx = xs[(xs + ox >= 0) & (xs + ox + 1 <= W - 1)]
        sub = np.ix_(yy, xx)
        src = np.ix_(yy + oy, xx + ox)
        for k, im in ((b, im1), (b + B, im2)):
            assert np.array_equal(o['im01'][k][sub], (im[b] / np.float32(255.0))[src])
        m4 = mask[b, :, :, 0]
        want_m = (m4[src] * m4[np.ix_(yy + oy + 1, xx + ox)] * m4[np.ix_(yy + oy, xx + ox + 1)] * m4[np.ix_(yy + oy + 1, xx + ox + 1)])
        assert np.array_equal(o['mask'][b, :, :, 0][sub], want_m)
        # a mask whose holes are isolated pixels: where all four taps are valid the mask is the shifted mask
        assert np.array_equal(o['mask'][b, :, :, 0][sub][want_m > 0], m4[src][want_m > 0])
        out_of = np.ones((H, W), bool)
        out_of[sub] = False
        assert (o['mask'][b, :, :, 0][out_of] == 0).all()
        v = want_m > 0
        d = np.abs(o['flow'][b][sub][v] - flow[b][src][v]).max()
        assert d <= R.coord_floor(H, W), d
    assert np.isfinite(o['flow']).all()


@pytest.mark.parametrize("shape", R.WARP_SHAPES)
def test_warp_consistency_on_device(shape, dev):
    a = R.warp_inputs(shape)
    o = _run_kernel(dev, a, 0)
    err, n = R.warp_consistency_error(o['im01'], o['flow'], o['mask'], a['mats'])
    print("warp consistency %s: %.3f grey levels over %d valid pixels" % (shape, err, n))
    assert n > 0.4 * shape[0] * shape[1] * shape[2]
    assert err <= R.WARP_TOL


# ------------------------------------------------------------------------------------------------ engine, trainer
def _gt(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    base = torch.stack([3.0 + 2.0 * torch.sin(xx / 37.0), -1.0 + 1.5 * torch.cos(yy / 23.0)], -1)
    flow = base[None].repeat(B, 1, 1, 1) + torch.randn(B, H, W, 2, generator=g) * 0.5
    mask = (torch.rand(B, H, W, 1, generator=g) > 0.1).float()
    flow[mask.expand(-1, -1, -1, 2) == 0] = float('nan')
    return flow, mask


def test_engine_geometric_set_input(dev):
    from unflow_amd.core import augment as A
    from unflow_amd.core.engine import CHANNEL_MEAN as MEAN, FlowNetEngine
    B, H, W = 2, 128, 192
    eng = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=5, supervised=True)
    im1, im2 = (t.to(dev) for t in images(B, H, W, 81))
    fgt, mgt = (t.to(dev) for t in _gt(B, H, W, 82))
    draws = A.draw_supervised_augmentation(B, torch.Generator().manual_seed(83), geometric=True)
    eng.set_input(im1, im2, augment=draws, target=(fgt, mgt))
    eng.forward_net()
    loss = eng.forward_loss(with_grad=True)
    eng.backward_net()
    torch.cuda.synchronize()
    # the direct kernel call
    im01, x0 = torch.zeros_like(eng.im01), torch.zeros_like(eng.x0)
    flow, mask = torch.zeros_like(eng.flow_gt), torch.zeros_like(eng.mask_gt)
    A.supervised_geo_augment(im1, im2, fgt, mgt, A.affine_pixel_maps(draws['theta_global'], draws['theta_local'], H, W), draws, im01,
                             x0, flow, mask, gt_sampling='bilinear', mean=MEAN)
    torch.cuda.synchronize()
    for got, want in ((eng.im01, im01), (eng.x0, x0), (eng.flow_gt, flow), (eng.mask_gt, mask)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert 0.3 < eng.mask_gt.mean().item() < 1.0 and torch.isfinite(eng.flow_gt).all()
    assert np.isfinite(loss.item()) and loss.item() > 0
    assert torch.isfinite(eng.G).all() and eng.G.abs().max().item() > 0
    # thetas alone: identity photometric draws
    only = dict(theta_global=draws['theta_global'], theta_local=draws['theta_local'])
    eng.set_input(im1, im2, augment=only, target=(fgt, mgt))
    torch.cuda.synchronize()
    assert torch.equal(eng.im01, im01) and torch.equal(eng.flow_gt, flow)
    want = A.photometric(eng.im01, A.identity_photometric(B), out=torch.zeros_like(eng.x0), mean=MEAN)
    assert torch.equal(eng.x0, want)
    # 'nearest' through the params key
    eng.params['gt_sampling'] = 'nearest'
    eng.set_input(im1, im2, augment=draws, target=(fgt, mgt))
    A.supervised_geo_augment(im1, im2, fgt, mgt, A.affine_pixel_maps(draws['theta_global'], draws['theta_local'], H, W), draws, im01,
                             x0, flow, mask, gt_sampling='nearest', mean=MEAN)
    torch.cuda.synchronize()
    assert torch.equal(eng.flow_gt, flow) and torch.equal(eng.mask_gt, mask) and eng.mask_gt.mean().item() > 0.5
    eng.params['gt_sampling'] = 'bilinear'
    # a photometric-only dict still takes the old path: its outputs are today's (prepare_image_pair, copies, photometric)
    photo = {k: v for k, v in draws.items() if not k.startswith('theta')}
    clean = torch.nan_to_num(fgt)
    eng.set_input(im1, im2, augment=photo, target=(clean, mgt))
    torch.cuda.synchronize()
    assert torch.equal(eng.flow_gt, clean) and torch.equal(eng.mask_gt, mgt)
    assert torch.equal(eng.im01, _prepare01(im1, im2))
    assert torch.equal(eng.x0, A.photometric(eng.im01, photo, out=torch.zeros_like(eng.x0), mean=MEAN))
    with pytest.raises(ValueError, match="2 transforms"):
        eng.set_input(im1, im2, augment=dict(draws, theta_global=draws['theta_global'][:1]), target=(fgt, mgt))


@pytest.mark.parametrize("spec,B,H,W", [('C', 2, 128, 192), ('S', 1, 64, 128)])
def test_trainer_geometric_graph_matches_eager(spec, B, H, W, dev):
    from unflow_amd.core import augment as A
    from unflow_amd.core.train import Trainer
    im1, im2 = (t.to(dev) for t in images(B, H, W, 91))
    fgt, mgt = (t.to(dev) for t in _gt(B, H, W, 92))
    g = torch.Generator().manual_seed(93)
    draws = [A.draw_supervised_augmentation(B, g, geometric=True) for _ in range(3)]
    params = dict(flownet=spec, learning_rate=1e-4, augment_geometric=True)
    out = []
    for use_graph in (False, True):
        tr = Trainer(B, H, W, params, device=dev, seed=7, use_graph=use_graph, supervised=True)
        assert tr.augment_geometric
        losses = [tr.train_step(im1, im2, augment=d, target=(fgt, mgt)).clone() for d in draws]
        torch.cuda.synchronize()
        out.append((torch.cat(losses).cpu(), tr.engine.P.clone().cpu(), tr.engine.flow_gt.clone().cpu()))
    assert torch.isfinite(out[0][0]).all() and torch.isfinite(out[0][1]).all()
    assert torch.equal(out[0][1], out[1][1])                       # parameters bit-identical
    assert torch.equal(out[0][2], out[1][2])
    assert torch.allclose(out[0][0], out[1][0], rtol=1e-6, atol=0), (out[0][0], out[1][0])
    # the trainer's own draws: geometric ones, from its generator
    tr = Trainer(B, H, W, dict(params, augment_max_rotation=5.0, gt_sampling='nearest'), device=dev, seed=7, use_graph=False,
                 supervised=True)
    assert tr.geometric_ranges == dict(max_rotation=5.0) and tr.engine.params['gt_sampling'] == 'nearest'
    before = tr.engine.flow_gt.clone()
    assert np.isfinite(float(tr.train_step(im1, im2, target=(fgt, mgt))))
    assert not torch.equal(tr.engine.flow_gt, before) and not torch.equal(tr.engine.flow_gt, torch.nan_to_num(fgt))
    with pytest.raises(ValueError, match="supervised"):
        Trainer(B, H, W, params, device=dev, use_graph=False)
    with pytest.raises(ValueError, match="gt_sampling"):
        Trainer(B, H, W, dict(params, gt_sampling='cubic'), device=dev, use_graph=False, supervised=True)


# ------------------------------------------------------------------------------------------------ device loaders
def loader_threads():
    return [t.name for t in threading.enumerate() if t.name.startswith(("png-inflate", "png-producer"))]


def _same_batches(host, devit, n):
    for _ in range(n):
        hb, db = next(host), next(devit)
        assert len(hb) == len(db) == 4
        for h, d in zip(hb, db):
            assert d.is_cuda and F.same_bits(h, d.cpu().numpy())
    devit.close()


@pytest.mark.parametrize("gt", ['occ', 'noc'])
def test_sintel_device_train_gt_equals_host(tmp_path, gt, dev):
    from unflow_amd.sintel.input import SintelInput
    F.make_sintel(tmp_path, [(3, (20, 30)), (2, (16, 24)), (3, (23, 41))], seed=5, unknown=0.02)
    inp = SintelInput(F.Data(tmp_path), batch_size=3, dims=(16, 24), normalize=(gt == 'noc'))
    kw = dict(variant='final' if gt == 'noc' else 'clean', gt=gt, seed=9, shift=2)
    _same_batches(inp.input_train_gt(**kw), inp.input_train_gt(device=dev, workers=2, **kw), 4)      # 12 examples of 5: two cycles
    assert not loader_threads()
    with pytest.raises(ValueError, match=r"frame_0001\.png is 16 x 24"):
        SintelInput(F.Data(tmp_path), batch_size=5, dims=(20, 24), normalize=False).input_train_gt(device=dev)
    assert not loader_threads()


def test_chairs_device_train_gt_equals_host(tmp_path, dev):
    from test_geo_augment_cpu import _chairs_train_tree
    from unflow_amd.chairs.input import ChairsInput
    _chairs_train_tree(tmp_path, [(20, 30), (16, 24), (31, 25), (18, 40)], seed=3)
    inp = ChairsInput(F.Data(tmp_path), batch_size=3, dims=(16, 24), normalize=False)
    _same_batches(inp.input_train_gt(seed=4, shift=3), inp.input_train_gt(seed=4, shift=3, device=dev, workers=2), 3)
    assert not loader_threads()


# ------------------------------------------------------------------------------------------------ the command
def test_finetune_command_line(tmp_path, capsys, dev):
    from unflow_amd import finetune as FT
    from unflow_amd.core import tf_checkpoint as T
    F.make_sintel(tmp_path / "data", [(3, (70, 140)), (2, (64, 128))], seed=6)
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\ndata = %s\nlog = %s\ncheckpoints = %s\n\n[run]\nbatch_size = 1\n\n[train]\nflownet = S\nheight = 64\n"
                   "width = 128\nlearning_rate = 0.0001\ndecay_interval = 100000\nsave_interval = 2\ndisplay_interval = 1\n\n"
                   "[train_sintel_ft]\nlearning_rate = 0.00005\n"
                   % (tmp_path / "data", tmp_path / "log", tmp_path / "ckpt"))
    argv = ['--ex', 'ft', '--dataset', 'sintel', '--geometric', '--config', str(cfg)]
    assert FT.main(argv + ['--iters', '4']) == 0
    out = capsys.readouterr().out
    assert '-- training from i = 1 to 4' in out and 'geometric augmentation' in out
    losses = [float(l.split('loss = ')[1]) for l in out.splitlines() if l.startswith('-- train: i = ')]
    assert len(losses) == 4 and all(np.isfinite(losses))
    ck = str(tmp_path / "ckpt" / "ft")
    assert os.path.basename(T.latest_checkpoint(ck)) == 'model.ckpt-4'
    assert any('model.ckpt-2' in f for f in os.listdir(ck))
    assert os.path.basename(T.latest_checkpoint(str(tmp_path / "log" / "ex" / "ft"))) == 'model.ckpt-4'      # conclude()
    assert FT.main(argv + ['--iters', '8', '--host_decode']) == 0
    out = capsys.readouterr().out
    assert '-- training from i = 5 to 8' in out
    assert [l.split(',')[0] for l in out.splitlines() if l.startswith('-- train: i = ')] == ['-- train: i = %d' % i for i in (5, 6, 7, 8)]
    assert os.path.basename(T.latest_checkpoint(ck)) == 'model.ckpt-8'
    import gc
    gc.collect()
    assert not loader_threads()
