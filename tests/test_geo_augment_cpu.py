"""CPU (-m "not gpu"): what the geometric-augmentation GPU tests (tests/test_geo_augment_gpu.py) rest on — the comparator of
tests/geo_augment_ref.py proven on every case the GPU test runs, the pixel maps, the draw order, the transform's meaning (warp
consistency of the fp64 reference), the new entry's argument checks — and the host side of the feature: the Sintel / Chairs
input_train_gt iterators and the parser of python -m unflow_amd.finetune."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flo_fixture as F
import geo_augment_ref as R
from unflow_amd.core import augment as A


# ------------------------------------------------------------------------------------------------ the comparator
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape,kind", R.CASES)
def test_yardstick_within_bound_and_exclusions_under_cap(shape, kind, mode):
    r = R.reference(shape, kind, mode)
    print("case %s %s mode %d: excluded %s, yardstick flow %.3e px (tol %.3e), image %.3e (tol %.3e), valid share %.3f"
          % (shape, kind, mode, {k: round(float(v), 5) for k, v in r.shares.items()}, r.yard_flow_err, r.flow_tol, r.yard_im_err,
             r.im_tol, r.ref['mask'].mean()))
    for k, share in r.shares.items():
        assert share <= R.CAP, (k, share)
    if kind != 'full':
        assert max(r.shares.values()) == 0.0          # exact whole-pixel maps: every pixel is compared
    assert r.mask_mismatches(r.yard['mask']) == 0
    assert r.yard_flow_err <= r.flow_tol and r.yard_im_err <= r.im_tol
    # the bound is tight enough to catch a wrong transform: a whole pixel is far outside it
    assert r.flow_tol < 0.01 and r.im_tol < 0.01
    for o in (r.ref, r.yard):
        assert all(np.isfinite(o[k]).all() for k in ('im01', 'flow', 'mask'))
    assert 0.3 < r.ref['mask'].mean() < 1.0           # both valid and invalid pixels occur
    holes = R.case_inputs(shape, kind)['mask'].reshape(-1) == 0
    assert not np.isfinite(R.case_inputs(shape, kind)['flow'].reshape(-1, 2)[holes]).all() and holes.mean() > 0.01


# ------------------------------------------------------------------------------------------------ pixel maps
def _formula(theta, H, W):
    t = np.asarray(theta, np.float64).reshape(6)
    return np.array([[W * t[0] / (W - 1), W * t[1] / (H - 1), (W / 2) * (-t[0] - t[1] + t[2] + 1)],
                     [H * t[3] / (W - 1), H * t[4] / (H - 1), (H / 2) * (-t[3] - t[4] + t[5] + 1)]])


@pytest.mark.parametrize("H,W", [(19, 45), (320, 768)])
def test_affine_pixel_maps(H, W):
    g = torch.Generator().manual_seed(3)
    B = 5
    tg = A.draw_affine(B, horizontal_flipping=True, generator=g, **R.FULL_RANGES)
    tl = A.draw_affine(B, generator=g, **R.FULL_RANGES)
    m = A.affine_pixel_maps(tg, tl, H, W, dtype=torch.float64).numpy()
    assert m.shape == (B, 3, 6)
    assert A.affine_pixel_maps(tg, tl, H, W).dtype == torch.float32
    full = lambda a: np.vstack([a.reshape(2, 3), [0, 0, 1]])
    for b in range(B):
        G, L = full(_formula(tg[b], H, W)), full(_formula(tl[b], H, W))
        np.testing.assert_allclose(full(m[b, 0]), G, rtol=0, atol=1e-12 * W)
        np.testing.assert_allclose(full(m[b, 1]), G @ L, rtol=0, atol=1e-12 * W)
        np.testing.assert_allclose(full(m[b, 1]) @ full(m[b, 2]), np.eye(3), rtol=0, atol=1e-12)
        # the map is stn_affine_kernel's: normalised grid -> theta -> (xs + 1) W / 2
        px, py = 7.0, 3.0
        xt, yt = 2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1
        t = tg[b].double().numpy().reshape(6)
        want = ((t[0] * xt + t[1] * yt + t[2] + 1) * W / 2, (t[3] * xt + t[4] * yt + t[5] + 1) * H / 2)
        np.testing.assert_allclose(G @ [px, py, 1], [want[0], want[1], 1], rtol=0, atol=1e-10)
    ident = A.pixel_identity_theta(H, W)
    mi = A.affine_pixel_maps(ident, ident, H, W, dtype=torch.float64).numpy()[0]
    for k in range(3):
        np.testing.assert_allclose(mi[k].reshape(2, 3), np.eye(3)[:2], rtol=0, atol=1e-12)
    eye = torch.eye(3)[:2][None]
    assert abs(A.affine_pixel_maps(eye, eye, H, W, dtype=torch.float64)[0, 0, 0] - W / (W - 1)) < 1e-12      # theta = I is a zoom
    with pytest.raises(ValueError):
        A.affine_pixel_maps(eye, eye, 1, W)


def test_draw_order_of_supervised_augmentation():
    """Photometric draws first: the same with and without `geometric`; today's calls return what they returned."""
    gen = lambda: torch.Generator().manual_seed(1234)
    B = 3
    today = A.draw_photometric(B, noise_stddev=0.04, min_contrast=-0.3, max_contrast=0.3, brightness_stddev=0.02, min_colour=0.9,
                               max_colour=1.1, min_gamma=0.7, max_gamma=1.5, generator=gen())
    for call in (lambda: A.draw_supervised_augmentation(B, gen()), lambda: A.draw_supervised_augmentation(B, generator=gen())):
        d = call()
        assert sorted(d) == sorted(today) == ['brightness', 'colour', 'contrast', 'gamma', 'noise']
        assert all(torch.equal(d[k], today[k]) for k in today)
    g = gen()
    geo = A.draw_supervised_augmentation(B, g, geometric=True)
    assert sorted(geo) == sorted(list(today) + ['theta_global', 'theta_local'])
    assert all(torch.equal(geo[k], today[k]) for k in today)
    # the thetas are the NEXT draws of the stream, with the unsupervised step's ranges
    g2 = gen()
    A.draw_supervised_augmentation(B, g2)
    tg = A.draw_affine(B, horizontal_flipping=True, min_scale=0.9, max_scale=1.1, generator=g2)
    tl = A.draw_affine(B, min_scale=0.9, max_scale=1.1, generator=g2)
    assert torch.equal(geo['theta_global'], tg) and torch.equal(geo['theta_local'], tl)
    assert geo['theta_global'].shape == (B, 2, 3) and (geo['theta_global'][:, :, 2] == 0).all()
    wide = A.draw_supervised_augmentation(64, gen(), geometric=True, max_rotation=10.0, max_translation_x=0.1, local_max_scale=1.0,
                                          local_min_scale=1.0, horizontal_flipping=False)
    assert (wide['theta_global'][:, 0, 0] > 0).all() and wide['theta_global'][:, 0, 2].abs().max() > 0.05
    assert wide['theta_global'][:, 1, 0].abs().max() > 0.05
    assert torch.equal(wide['theta_local'], torch.eye(3)[:2].expand(64, 2, 3))
    with pytest.raises(TypeError):
        A.draw_supervised_augmentation(B, gen(), geometric=True, max_shear=1.0)
    with pytest.raises(TypeError):
        A.draw_supervised_augmentation(B, gen(), max_rotation=1.0)


# ------------------------------------------------------------------------------------------------ the transform's meaning
@pytest.mark.parametrize("shape", R.WARP_SHAPES)
def test_warp_consistency_of_the_reference(shape):
    a = R.warp_inputs(shape)
    o = R.evaluate(a['im1'], a['im2'], a['flow'], a['mask'], a['mats'], 0, np.float64)
    err, n = R.warp_consistency_error(o['im01'], o['flow'], o['mask'], a['mats'])
    print("warp consistency %s: %.3f grey levels over %d valid pixels" % (shape, err, n))
    assert n > 0.4 * shape[0] * shape[1] * shape[2]
    assert err <= R.WARP_TOL
    # a wrong inverse / swapped composition is tens of grey levels: the comparator sees it
    swapped = np.array(a['mats'])
    swapped[:, 2] = a['mats'][:, 0]
    bad = R.evaluate(a['im1'], a['im2'], a['flow'], a['mask'], swapped, 0, np.float64)
    assert R.warp_consistency_error(bad['im01'], bad['flow'], bad['mask'], a['mats'])[0] > 10.0


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from unflow_amd import build, _lib
    build.build()
    return _lib.lib()


def test_abi_errors_without_a_device(lib):
    fn = lib.unflow_supervised_geo_augment
    one = (ctypes.c_float * 64)()
    p = ctypes.cast(one, ctypes.c_void_p)
    two = (ctypes.c_float * 64)()
    q = ctypes.cast(two, ctypes.c_void_p)
    three = (ctypes.c_float * 64)()
    r = ctypes.cast(three, ctypes.c_void_p)
    n = ctypes.c_void_p(0)
    # im1 im2 flow mask mats contrast brightness colour gamma noise n_par mean3 im01 x0 ld_out flow_out mask_out mode B H W stream
    good = [p, p, p, p, p, p, p, p, p, p, 1, n, q, q, 4, q, r, 0, 1, 2, 2, n]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 12, 13, 15, 16):
        args = list(good)
        args[i] = n
        assert fn(*args) == -1, i
    def with_(**kw):
        names = ['im1', 'im2', 'flow', 'mask', 'mats', 'contrast', 'brightness', 'colour', 'gamma', 'noise', 'n_par', 'mean3',
                 'im01', 'x0', 'ld_out', 'flow_out', 'mask_out', 'mode', 'B', 'H', 'W', 'stream']
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args)
    assert with_(n_par=0) == -5 and with_(n_par=-1) == -5
    assert with_(H=0) == -5 and with_(W=0) == -5 and with_(B=-1) == -5 and with_(ld_out=2) == -5
    assert with_(mode=2) == -7 and with_(mode=-1) == -7
    assert with_(flow_out=p) == -7 and with_(mask_out=p) == -7 and with_(im01=p) == -7        # gathered sources are not targets
    assert with_(B=0) == 0                      # nothing to do, nothing launched
    assert with_(mask=n, B=0) == 0              # a null mask means all ones


# ------------------------------------------------------------------------------------------------ host iterators
DIMS = (16, 24)


def _inp(cls, root, B=3, dims=DIMS, normalize=False):
    return cls(F.Data(root), batch_size=B, dims=dims, normalize=normalize)


@pytest.fixture(scope="module")
def sintel_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("sintel_train")
    truth = F.make_sintel(root, [(3, (20, 30)), (2, (16, 24)), (3, (23, 41))], seed=5, unknown=0.02)
    return root, truth


def _sintel_examples(truth):
    return [truth[k] for k in sorted(truth)]


@pytest.mark.parametrize("gt", ['occ', 'noc'])
@pytest.mark.parametrize("variant", ['clean', 'final'])
def test_sintel_input_train_gt_host(sintel_tree, variant, gt):
    from unflow_amd.core.input import read_png_image
    from unflow_amd.middlebury.input import scene_pairs
    from unflow_amd.sintel.input import SintelInput
    root, truth = sintel_tree
    inp = _inp(SintelInput, root)
    pairs = scene_pairs(os.path.join(str(root), 'sintel/training', variant))
    ex = _sintel_examples(truth)
    assert len(pairs) == len(ex) == 5
    shift, seed = 2, 9
    it = inp.input_train_gt(variant=variant, gt=gt, seed=seed, shift=shift)
    rng = np.random.RandomState(seed)
    pos = shift
    h, w = DIMS
    for _ in range(4):                                   # 12 examples: more than two cycles of the 5 pairs
        im1, im2, flow, mask = next(it)
        assert im1.shape == im2.shape == (3, h, w, 3) and flow.shape == (3, h, w, 2) and mask.shape == (3, h, w, 1)
        assert all(t.dtype == np.float32 for t in (im1, im2, flow, mask))
        for k in range(3):
            (fn1, fn2), (fl, inv, occ) = pairs[pos % 5], ex[pos % 5]
            pos += 1
            a, b = read_png_image(fn1), read_png_image(fn2)
            oy = int(rng.randint(0, a.shape[0] - h + 1))
            ox = int(rng.randint(0, a.shape[1] - w + 1))
            assert 0 <= oy <= a.shape[0] - h and 0 <= ox <= a.shape[1] - w
            win = lambda t: t[oy:oy + h, ox:ox + w]
            assert np.array_equal(im1[k], win(a)) and np.array_equal(im2[k], win(b))
            m_occ = 1 - (win(inv) != 0).astype(np.float32)[..., None]
            o = (win(occ) != 0).astype(np.float32)[..., None]
            want_f, want_m = (win(fl), m_occ) if gt == 'occ' else (win(fl) * (1 - o), m_occ * (1 - o))
            assert F.same_bits(flow[k], want_f.astype(np.float32)) and F.same_bits(mask[k], want_m.astype(np.float32))
    assert set(np.unique(mask)) <= {0.0, 1.0}


def test_sintel_input_train_gt_refusals(sintel_tree, tmp_path):
    from unflow_amd.sintel.input import SintelInput
    root, _ = sintel_tree
    with pytest.raises(ValueError, match="variant"):
        _inp(SintelInput, root).input_train_gt(variant='albedo')
    with pytest.raises(ValueError, match="gt must"):
        _inp(SintelInput, root).input_train_gt(gt='all')
    with pytest.raises(ValueError, match=r"frame_0001\.png is 16 x 24"):       # scene_1 is 16 x 24: a 20 x 24 window leaves it
        it = _inp(SintelInput, root, B=5, dims=(20, 24)).input_train_gt()
        next(it)
    F.make_sintel(tmp_path, [(3, (20, 30))], seed=1)
    os.remove(os.path.join(str(tmp_path), 'sintel/training/flow/scene_0/frame_0002.flo'))
    with pytest.raises(ValueError, match="flow files"):
        _inp(SintelInput, tmp_path).input_train_gt()


def _chairs_train_tree(root, sizes, seed):
    """flying_chairs/image pairs with flying_chairs/train_flow/%05d_flow.flo (this project's training layout)."""
    rs = np.random.RandomState(seed)
    base = os.path.join(str(root), 'flying_chairs')
    flows = []
    for i, (h, w) in enumerate(sizes):
        for k in (1, 2):
            F.write_frame(os.path.join(base, 'image', '%05d_img%d.png' % (i + 1, k)), rs, h, w)
        flows.append(F.flow_field(rs, h, w, 0.05))
        F.write_flo(os.path.join(base, 'train_flow', '%05d_flow.flo' % (i + 1)), flows[-1])
    return flows


def test_chairs_input_train_gt_host(tmp_path):
    from unflow_amd.chairs.input import ChairsInput
    from unflow_amd.core.input import read_png_image
    sizes = [(20, 30), (16, 24), (31, 25), (18, 40)]
    flows = _chairs_train_tree(tmp_path, sizes, seed=3)
    inp = _inp(ChairsInput, tmp_path, normalize=True)
    files = inp.train_gt_files()
    assert [os.path.basename(f[2]) for f in files] == ['%05d_flow.flo' % (i + 1) for i in range(4)]
    assert all(os.path.basename(f[0]).endswith('img1.png') and os.path.basename(f[1]).endswith('img2.png') for f in files)
    seed, shift = 4, 3
    it = inp.input_train_gt(seed=seed, shift=shift)
    rng = np.random.RandomState(seed)
    pos = shift
    h, w = DIMS
    for _ in range(3):
        im1, im2, flow, mask = next(it)
        for k in range(3):
            i = pos % 4
            pos += 1
            a, b = read_png_image(files[i][0]), read_png_image(files[i][1])
            oy = int(rng.randint(0, a.shape[0] - h + 1))
            ox = int(rng.randint(0, a.shape[1] - w + 1))
            win = lambda t: t[oy:oy + h, ox:ox + w]
            assert np.array_equal(im1[k], inp._normalize_image(win(a)).astype(np.float32))
            assert np.array_equal(im2[k], inp._normalize_image(win(b)).astype(np.float32))
            f = win(flows[i])
            assert F.same_bits(flow[k], f)
            assert np.array_equal(mask[k, :, :, 0], ((f[..., 0] < 1e9) & (f[..., 1] < 1e9)).astype(np.float32))
    assert (mask == 0).any() and not np.isfinite(flow).all()       # the markers stay under mask 0: the consumer selects them away
    os.remove(files[3][2])
    with pytest.raises(ValueError, match="4 frame pairs in image but 3 flow files"):
        inp.input_train_gt()


def test_flo_gt_planner_matches_host_draws(sintel_tree):
    """The device iterator's host half: same examples, same windows, the table in the kernels' order."""
    from unflow_amd.core import png_device as D
    from unflow_amd.sintel.input import SintelInput
    root, _ = sintel_tree
    inp = _inp(SintelInput, root)
    pairs, lists = inp.train_files('sintel/training/clean')
    examples = [tuple(p) + tuple(g[k] for g in lists) for k, p in enumerate(pairs)]
    plan = D.GTPlanner(examples, 3, DIMS, seed=9, shift=2, gt_kind='sintel')
    rng = np.random.RandomState(9)
    pos = 2
    for _ in range(3):
        got = plan.next_batch()
        for ex in got:
            assert tuple(f[0] for f in ex) == examples[pos % 5]
            pos += 1
            assert [f[2] for f in ex] == [D.FRAME, D.FRAME, D.FLO, D.MASK, D.MASK]
            hh, ww = ex[0][1][:2]
            oy = int(rng.randint(0, hh - DIMS[0] + 1))
            ox = int(rng.randint(0, ww - DIMS[1] + 1))
            assert all((f[3], f[4]) == (oy, ox) for f in ex)
        assert [f[2] for f in plan.files(got)] == [D.FLO] * 3 + [D.MASK] * 6 + [D.FRAME] * 6
    with pytest.raises(ValueError, match="gt_kind"):
        D.GTPlanner(examples, 3, DIMS, seed=0, gt_kind='mdb')
    with pytest.raises(ValueError, match="examples of 3 files"):
        D.GTPlanner(examples, 3, DIMS, seed=0, gt_kind='flo')
    with pytest.raises(ValueError, match="leaves it"):
        D.GTPlanner(examples, 5, (20, 24), seed=0, gt_kind='sintel').next_batch()


def test_kitti_input_train_gt_unchanged(tmp_path):
    """KITTIInput.input_train_gt gives what the parent's loop gives: written out here, independent of the shared planner."""
    import kitti_gt_fixture as KF
    from unflow_amd.core.input import decode_png, read_png_image
    from unflow_amd.kitti.input import KITTIInput
    written = KF.make_gt_tree(tmp_path, n_per_dataset=(2, 3), size=(30, 41), seed=2)
    kin = KITTIInput(KF.Data(tmp_path), batch_size=2, dims=(16, 24), normalize=False)
    files = kin.train_gt_files(0)
    assert len(files) == 5 and {f[2] for f in files} == set(written)
    it = kin.input_train_gt(0, seed=3, shift=1)
    rng = np.random.RandomState(3)
    pos = 1
    for _ in range(3):
        im1, im2, flow, mask = next(it)
        for k in range(2):
            fn1, fn2, fgt = files[pos % len(files)]
            pos += 1
            a, b = read_png_image(fn1), read_png_image(fn2)
            with open(fgt, 'rb') as f:
                gt = decode_png(f.read()).astype(np.float32)
            oy = int(rng.randint(0, a.shape[0] - 16 + 1))
            ox = int(rng.randint(0, a.shape[1] - 24 + 1))
            win = lambda t: t[oy:oy + 16, ox:ox + 24]
            assert np.array_equal(im1[k], win(a)) and np.array_equal(im2[k], win(b))
            assert np.array_equal(flow[k], (win(gt)[:, :, 0:2] - 2 ** 15) / 64.0) and np.array_equal(mask[k], win(gt)[:, :, 2:3])


# ------------------------------------------------------------------------------------------------ the command
def test_finetune_parse_args():
    from unflow_amd import finetune as FT
    a = FT.parse_args(['--ex', 'x', '--dataset', 'sintel'])
    assert (a.variant, a.gt, a.geometric, a.iters, a.batch_size, a.dims, a.host_decode, a.ow) == \
        ('clean', 'occ', False, None, None, None, False, False)
    a = FT.parse_args(['--ex', 'x', '--dataset', 'sintel', '--variant', 'final', '--gt', 'noc', '--geometric', '--iters', '8',
                       '--batch_size', '2', '--dims', '128', '192', '--host_decode', '--ow'])
    assert (a.variant, a.gt, a.geometric, a.iters, a.batch_size, a.dims, a.host_decode, a.ow) == \
        ('final', 'noc', True, 8, 2, (128, 192), True, True)
    for ds in ('kitti', 'chairs'):
        a = FT.parse_args(['--ex', 'x', '--dataset', ds])
        assert a.variant is None and a.gt is None
    bad = [['--ex', 'x', '--dataset', 'kitti', '--variant', 'clean'], ['--ex', 'x', '--dataset', 'chairs', '--gt', 'noc'],
           ['--ex', 'x', '--dataset', 'mdb'], ['--dataset', 'sintel'], ['--ex', 'x', '--dataset', 'sintel', '--variant', 'albedo'],
           ['--ex', 'x', '--dataset', 'sintel', '--iters', '0'], ['--ex', 'x', '--dataset', 'sintel', '--batch_size', '0'],
           ['--ex', 'x', '--dataset', 'sintel', '--dims', '100', '192']]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            FT.parse_args(argv)
        assert e.value.code == 2, argv
    cfg = {'train': {'height': 320, 'width': 768, 'flownet': 'C'}, 'train_kitti_ft': {'height': 320, 'width': 1152, 'finetune': 'a'}}
    p = FT.finetune_params(cfg, 'kitti', True)
    assert (p['width'], p['flownet'], p['augment_geometric'], p['gt_sampling']) == (1152, 'C', True, 'nearest')
    p = FT.finetune_params(cfg, 'sintel', True)
    assert p['width'] == 768 and p['augment_geometric'] is True and 'gt_sampling' not in p and 'finetune' not in p
    assert 'augment_geometric' not in FT.finetune_params(cfg, 'kitti', False)
