"""Supervised fine-tuning input (kitti/input.py:86-146, KITTIInput.input_train_gt) on a synthetic tree with the KITTI 2015
and 2012 layouts, and the one-direction engine's layout (no GPU needed)."""
import os
import random

import numpy as np
import pytest

from kitti_gt_fixture import Data, make_gt_tree


def _restated_files(root, hold_out):
    """kitti/input.py:82-124 restated."""
    dirs = [('data_scene_flow/training/image_2', 'data_scene_flow/training/flow_occ'),
            ('data_stereo_flow/training/colored_0', 'data_stereo_flow/training/flow_occ')]
    filenames = []
    for img_dir, gt_dir in dirs:
        img_dir, gt_dir = os.path.join(root, img_dir), os.path.join(root, gt_dir)
        img_files, gt_files = sorted(os.listdir(img_dir)), sorted(os.listdir(gt_dir))
        ds = []
        for i in range(len(gt_files)):
            ds.append((os.path.join(img_dir, img_files[2 * i]), os.path.join(img_dir, img_files[2 * i + 1]),
                       os.path.join(gt_dir, gt_files[i])))
        random.seed(0)
        random.shuffle(ds)
        filenames.extend(ds[hold_out:])
    random.seed(0)
    random.shuffle(filenames)
    return filenames


def test_train_gt_files_match_reference_listing_and_hold_out(tmp_path):
    from unflow_amd.kitti.input import KITTIInput
    make_gt_tree(tmp_path, n_per_dataset=(43, 45), size=(8, 8))
    inp = KITTIInput(Data(tmp_path), 2, (8, 8), normalize=False)
    got = inp.train_gt_files(40)
    assert got == _restated_files(str(tmp_path), 40)
    assert len(got) == (43 - 40) + (45 - 40)                       # 40 held out per dataset
    for fn1, fn2, fgt in got:                                      # images 2i, 2i+1 go with GT file i
        i = int(os.path.basename(fgt)[:6])
        assert os.path.basename(fn1) == '%06d_10.png' % i and os.path.basename(fn2) == '%06d_11.png' % i
        assert os.path.dirname(fn1).endswith('image_2') == ('data_scene_flow' in fgt)
    assert {('data_scene_flow' in f[2]) for f in got} == {True, False}
    assert len(inp.train_gt_files(0)) == 88


def test_input_train_gt_joint_crop_and_decode(tmp_path):
    from unflow_amd.kitti.input import KITTIInput
    written = make_gt_tree(tmp_path, n_per_dataset=(3, 2), size=(40, 56), seed=3)
    h, w = 24, 32
    inp = KITTIInput(Data(tmp_path), 2, (h, w), normalize=False)
    files = inp.train_gt_files(0)
    it = inp.input_train_gt(0, seed=7)
    rng = np.random.RandomState(7)
    k = 0
    for _ in range(3):                                             # past the end of the list: cyclic
        im1, im2, flow, mask = next(it)
        assert im1.shape == (2, h, w, 3) and im2.shape == (2, h, w, 3)
        assert flow.shape == (2, h, w, 2) and mask.shape == (2, h, w, 1)
        assert all(a.dtype == np.float32 for a in (im1, im2, flow, mask))
        for b in range(2):
            a1, a2, f, m = written[files[k % len(files)][2]]
            k += 1
            oy, ox = int(rng.randint(0, 40 - h + 1)), int(rng.randint(0, 56 - w + 1))
            # one window for both frames and the GT; flow = (v - 2^15) / 64, mask = channel 2
            np.testing.assert_array_equal(im1[b], a1[oy:oy + h, ox:ox + w])
            np.testing.assert_array_equal(im2[b], a2[oy:oy + h, ox:ox + w])
            np.testing.assert_array_equal(flow[b], f[oy:oy + h, ox:ox + w])
            np.testing.assert_array_equal(mask[b], m[oy:oy + h, ox:ox + w])
    # normalize=True: the images as Input._normalize_image leaves them, the GT untouched
    inp_n = KITTIInput(Data(tmp_path), 2, (h, w), normalize=True)
    n1, _, nf, _ = next(inp_n.input_train_gt(0, seed=7))
    r1, _, rf, _ = next(KITTIInput(Data(tmp_path), 2, (h, w), normalize=False).input_train_gt(0, seed=7))
    np.testing.assert_allclose(n1, inp_n._normalize_image(r1), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(nf, rf)


@pytest.mark.parametrize("spec", ['C', 'S', 'CSS'])
def test_one_direction_engine_plan(spec):
    """Row ranges of the one-direction engine: FlowNetC's feature tower on 2B rows, everything from the correlation on — and
    every FlowNetS — on B; d cat2[B:2B) is first written by conv3 (zeroed before its accumulating call) and d c3[B:2B) gets
    conv3's leaky-ReLU derivative after the correlation.  The bidirectional engine has neither."""
    import torch
    from unflow_amd.core.engine import FlowNetEngine
    B = 2
    eng = FlowNetEngine(B, 64, 128, params=dict(flownet=spec, train_all=True), device='cpu', layout_only=True, supervised=True)
    for st in eng.stages:
        assert st.pairs == [(0, B, 0)]        # one block on every stage: first frames at x0 rows [0, B), second at [B, 2B)
        enc = {'c1', 'cat2', 'c3'} if st.is_c else set()
        for name in st.bufs:
            assert st.rows[name] == (2 * B if name in enc else B), (st.kind, name)
        names = st.bwd_names
        if st.is_c:
            assert {names[k]: v for k, v in st.bwd_zero_rows.items()} == {'conv3': (B, 2 * B)}
            assert {names[k]: v for k, v in st.bwd_post_act.items()} == {'corr': [(B, 2 * B, 0, 256)]}
            assert {op.l.name.split('/')[-1]: op.n for op in st.ops if op.kind == 'layer' and op.n == 2 * B} == \
                {'conv1': 4, 'conv2': 4, 'conv3': 4}
        else:
            assert not st.bwd_zero_rows and not st.bwd_post_act
            assert all(op.n == B for op in st.ops)
    bi = FlowNetEngine(B, 64, 128, params=dict(flownet=spec), device='cpu', layout_only=True)
    for st in bi.stages:
        assert st.pairs is None               # the training engine: the directed batch
        assert not st.bwd_zero_rows and not st.bwd_post_act and all(op.n == 2 * B for op in st.ops)
    # the same parameters either way
    assert bi.n_params == eng.n_params and [l.name for l in bi.layers] == [l.name for l in eng.layers]
    del torch


def test_supervised_full_res_train_all_refused():
    from unflow_amd.core.engine import FlowNetEngine
    with pytest.raises(ValueError, match="shape error"):
        FlowNetEngine(1, 64, 64, params=dict(flownet='CS', full_res=True, train_all=True), device='cpu', layout_only=True,
                      supervised=True)
    FlowNetEngine(1, 64, 64, params=dict(flownet='CS', full_res=True), device='cpu', layout_only=True, supervised=True)


def test_supervised_augmentation_draws_photometric_only():
    import torch
    from unflow_amd.core.augment import draw_supervised_augmentation, draw_training_augmentation
    a = draw_supervised_augmentation(3, torch.Generator().manual_seed(1))
    assert set(a) == {'contrast', 'gamma', 'colour', 'noise', 'brightness'}
    t = draw_training_augmentation(3, torch.Generator().manual_seed(1))
    assert set(t) - set(a) == {'theta_global', 'theta_local'}
    assert float(a['contrast'].abs().max()) <= 0.3 and 0.7 <= float(a['gamma'].min()) <= float(a['gamma'].max()) <= 1.5
