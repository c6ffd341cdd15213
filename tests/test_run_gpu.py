"""FlowNetEngine.loss_terms() against the fp64 oracle and beside the training step, and python -m unflow_amd.run end to end on
synthetic trees (a child process per invocation)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXCLUDES = os.path.join(HERE, 'golden', 'kitti_excludes')

DEFAULT = dict(flownet='C', pyramid_loss=True, border_mask=True, ternary_weight=1.0, smooth_2nd_weight=3.0)
CASES = {
    'default': (DEFAULT, 1, 128, 192),
    'train_kitti': (dict(DEFAULT, fb_weight=0.2, mask_occlusion='fb', occ_weight=12.4), 1, 128, 192),
    'photo_grad_1st': (dict(flownet='C', pyramid_loss=True, border_mask=True, photo_weight=1.0, grad_weight=1.0, smooth_1st_weight=3.0),
                       2, 128, 192),
    # this file's addition: the forward-warp branch (disocclusion mask, sym term) and create_outgoing_mask instead of the border mask
    'disocc_sym': (dict(flownet='C', pyramid_loss=True, border_mask=False, ternary_weight=1.0, smooth_2nd_weight=3.0, sym_weight=0.5,
                        mask_occlusion='disocc'), 1, 128, 192),
}
SMOOTH = ('smooth_1st', 'smooth_2nd')


def _oracle_levels(M, im1, im2, fw, bw, params):
    """Per-level compute_losses of oracle.model_ref.pyramid_loss_from_flows' loop (the function itself returns the sums only)."""
    im1_s, im2_s = M.downsample(im1 / 255.0, 4), M.downsample(im2 / 255.0, 4)
    mask_s = M.downsample(M.create_border_mask(im1, 0.1), 4)
    need = {l for l in M.LOSSES if params.get(l + '_weight')}
    out = []
    for i, (f, b) in enumerate(zip(fw, bw)):
        fs = M.FLOW_SCALE / 2 ** i
        out.append(M.compute_losses(im1_s, im2_s, f * fs, b * fs, border_mask=mask_s if params.get('border_mask') else None,
                                    mask_occlusion=params.get('mask_occlusion', ''), data_max_distance=[3, 2, 2, 1, 1][i], need=need))
        if i + 1 < len(fw):
            im1_s, im2_s, mask_s = M.downsample(im1_s, 2), M.downsample(im2_s, 2), M.downsample(mask_s, 2)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_loss_terms_vs_oracle(case, dev):
    """loss_terms() after forward_net(); forward_loss() against pyramid_loss_from_flows in fp64 on the engine's own fp32 flows.
    Bounds: those of test_losses_gpu.py::test_compute_losses_vs_oracle (2e-5 relative for the smoothness terms, 2e-3 for the terms
    that sum a thresholded mask or a data term); the total within the 1e-4 relative of test_train_gpu.py (float-atomic order).
    All cases at 128 x 192: the oracle's second-order stencil needs two rows at the coarsest level (its create_mask refuses the
    1 x 2 level of a 64 x 128 input), so 64 x 128 is left to the trainer and command tests below."""
    from unflow_amd.core.engine import LAYER_WEIGHTS, LOSSES, FlowNetEngine
    from oracle import model_ref as M
    params, B, H, W = CASES[case]
    eng = FlowNetEngine(B, H, W, params=params, device=dev, seed=5)
    g = torch.Generator().manual_seed(17)
    im1 = torch.rand(B, H, W, 3, generator=g) * 255
    im2 = torch.roll(im1, shifts=(1, -2), dims=(1, 2)) * 0.95 + torch.rand(B, H, W, 3, generator=g) * 12
    eng.set_input(im1.to(dev), im2.to(dev))
    eng.forward_net()
    total = float(eng.forward_loss(with_grad=True))
    grads = [lv['gflow'].clone() for lv in eng.lv]
    flows = [lv['flow'].clone() for lv in eng.lv]
    got = eng.loss_terms()
    torch.cuda.synchronize()
    assert float(eng.loss_acc) == total                                    # not an accumulator of loss_terms
    assert all(torch.equal(a, lv['gflow']) and torch.equal(f, lv['flow']) for a, f, lv in zip(grads, flows, eng.lv))

    on = [k for k in LOSSES if params.get(k + '_weight')]
    fl = [f.cpu().double() for f in flows]
    fw, bw = [f[:B] for f in fl], [f[B:] for f in fl]
    comb, terms = M.pyramid_loss_from_flows(im1.double(), im2.double(), fw, bw, params)
    ref_levels = _oracle_levels(M, im1.double(), im2.double(), fw, bw, params)
    tol = lambda k: 2e-5 if k in SMOOTH else 2e-3
    assert set(got['combined']) == set(LOSSES) and len(got['levels']) == 5
    for k in LOSSES:
        ref = float(terms[k])
        print("%s loss/%s: got %.9g, oracle %.9g" % (case, k, got['combined'][k], ref))
        if k not in on:
            assert got['combined'][k] == 0.0 and ref == 0.0
            continue
        assert got['combined'][k] != 0.0                                     # a comparison of zeros proves nothing
        assert abs(got['combined'][k] - ref) <= tol(k) * abs(ref), (k, got['combined'][k], ref)
        assert abs(sum(w * lv[k] for w, lv in zip(LAYER_WEIGHTS, got['levels'])) - got['combined'][k]) <= 1e-6 * abs(ref)
    for i, (lv, ref_lv) in enumerate(zip(got['levels'], ref_levels)):
        assert list(lv) == on
        for k in on:
            ref = float(ref_lv[k])
            print("%s loss%d/%s: got %.9g, oracle %.9g" % (case, i + 2, k, lv[k], ref))
            assert abs(lv[k] - ref) <= tol(k) * abs(ref), (i, k, lv[k], ref)
    weighted = sum(params[k + '_weight'] * got['combined'][k] for k in on) + got['regularization']
    print("%s total: terms %.9g, engine %.9g, oracle without regularisation %.9g" % (case, weighted, total, float(comb)))
    assert got['regularization'] > 0.0
    assert abs(weighted - total) <= 1e-4 * abs(total), (weighted, total)


def test_loss_terms_refused_where_there_are_none(dev):
    from unflow_amd.core.engine import FlowNetEngine
    eng = FlowNetEngine(1, 64, 64, params=dict(DEFAULT), device=dev, seed=0, supervised=True)
    with pytest.raises(ValueError, match='supervised'):
        eng.loss_terms()


def test_loss_terms_leaves_the_step_alone(dev):
    """Two trainers, same seed, three graph-replayed steps each; one reads the terms after every step (the first read also allocates
    its scratch after the capture).  Parameters and Adam slots bit for bit, losses within float-atomic order."""
    from unflow_amd.core.train import Trainer
    params = dict(DEFAULT, learning_rate=1e-4)
    g = torch.Generator().manual_seed(2)
    batches = [((torch.rand(1, 64, 64, 3, generator=g) * 255).to(dev), (torch.rand(1, 64, 64, 3, generator=g) * 255).to(dev))
               for _ in range(3)]
    res = []
    for read_terms in (False, True):
        tr = Trainer(1, 64, 64, params, device=dev, seed=4, augment=False)
        losses = []
        for im1, im2 in batches:
            losses.append(float(tr.train_step(im1, im2)))
            if read_terms:
                t = tr.engine.loss_terms()
                weighted = t['combined']['ternary'] + 3.0 * t['combined']['smooth_2nd'] + t['regularization']
                # the terms of THIS step.  Only the regularisation differs: it is read from the weights the step has just
                # updated, each moved by at most ~lr = 1e-4 where the initial weights are ~1e-2: below 2 lr / |w| ~ 2e-2 of a term
                # that is itself a fraction of the loss, hence 1e-2 of the loss
                assert abs(weighted - losses[-1]) <= 1e-2 * abs(losses[-1]), (weighted, losses[-1])
        torch.cuda.synchronize()
        res.append((tr.engine.P.clone(), tr.engine.M.clone(), tr.engine.V.clone(), losses))
    (p0, m0, v0, l0), (p1, m1, v1, l1) = res
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    assert len(set(l0)) == 3


# ---------------------------------------------------------------------------------------------------- the command
def _png(path, h, w, rs):
    from unflow_amd.core.input import encode_png8_rgb
    os.makedirs(os.path.dirname(path), exist_ok=True)
    small = rs.randint(0, 256, size=(h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
    with open(path, 'wb') as f:
        f.write(encode_png8_rgb(np.kron(small, np.ones((8, 8, 1), np.uint8))[:h, :w]))


def _config(tmp_path):
    cfg = tmp_path / 'config.ini'
    cfg.write_text("[dirs]\ndata = %s\nlog = %s\ncheckpoints = %s\n[run]\nbatch_size = 1\n"
                   "[train]\nflownet = C\nheight = 64\nwidth = 128\nnum_iters = 4\nsave_interval = 2\ndisplay_interval = 1\n"
                   "learning_rate = 1.0e-4\npyramid_loss = True\nborder_mask = True\nternary_weight = 1.0\nsmooth_2nd_weight = 3.0\n"
                   % (tmp_path / 'data', tmp_path / 'log', tmp_path / 'ckpt'))
    return str(cfg)


def _run(tmp_path, *flags):
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.run', '--ex', 'e', '--config', _config(tmp_path)] + list(flags),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _events(folder):
    from unflow_amd.core.summary import read_events
    return [ev for name in sorted(os.listdir(folder)) if name.startswith('events.out.tfevents.')
            for ev in read_events(os.path.join(folder, name))]


def test_run_command_end_to_end(tmp_path, dev):
    from kitti_fixture import make_tree
    from unflow_amd.core.engine import LOSSES
    rs = np.random.RandomState(0)
    # two drives of 8 frames; the list names frame 20 of drive 0005: its frames 10 and 11 fall into [10, 32)
    drives = {'2011_09_26_drive_0005_extract': range(4, 12), '2011_09_26_drive_0011_extract': range(8)}
    for drive, frames in drives.items():
        for view in ('image_02', 'image_03'):
            for n in frames:
                _png(str(tmp_path / 'data' / 'kitti_raw' / '2011_09_26' / drive / view / 'data' / ('%010d.png' % n)), 72, 136, rs)
    make_tree(tmp_path / 'data', n_pairs=2)
    out = _run(tmp_path, '--iters', '4', '--batch_size', '1', '--kitti_excludes', EXCLUDES)
    assert 'training from i = 1 to 4' in out and 'NOT excluded' not in out
    ckpt, log = tmp_path / 'ckpt' / 'e', tmp_path / 'log' / 'ex' / 'e'
    for step in (2, 4):
        assert (ckpt / ('model.ckpt-%d.index' % step)).is_file()
    assert (log / 'model.ckpt-4.index').is_file()                            # conclude() kept the final checkpoint with the logs

    printed = [(int(i), float(l)) for i, l in re.findall(r'-- train: i = (\d+), loss = (\S+)', out)]
    assert [i for i, _ in printed] == [1, 2, 3, 4]
    train = _events(str(log / 'train'))
    assert [step for step, _ in train] == [1, 2, 3, 4]
    expected = (['loss/combined'] + ['loss/' + k for k in LOSSES] + ['loss%d/%s' % (k, t) for k in range(2, 7) for t in ('ternary', 'smooth_2nd')]
                + ['weight/ternary', 'weight/smooth_2nd', 'train/learning_rate'])
    rest = []
    for (step, vals), (_, loss) in zip(train, printed):
        assert sorted(vals) == sorted(expected), sorted(vals)
        assert vals['loss/combined'] == float(np.float32(loss))              # the printed loss
        assert vals['weight/ternary'] == 1.0 and vals['weight/smooth_2nd'] == 3.0
        assert vals['train/learning_rate'] == float(np.float32(1e-4))
        assert all(np.isfinite(v) for v in vals.values())
        assert vals['loss/ternary'] > 0 and vals['loss/smooth_2nd'] > 0 and vals['loss/fb'] == 0.0
        rest.append(loss - (vals['loss/ternary'] + 3.0 * vals['loss/smooth_2nd']))      # the regularisation term of the step
    # loss - sum(weight * term) is the L2 term: positive, and the same over four steps of learning rate 1e-4 to within 2 %
    assert min(rest) > 0 and max(rest) - min(rest) <= 0.02 * max(rest), rest

    evals = _events(str(log / 'eval'))
    assert [step for step, _ in evals] == [2, 4]
    for _, vals in evals:
        for tag in ('AEE/occluded', 'outliers/occluded', 'AEE/non-occluded', 'outliers/non-occluded', 'loss/combined', 'loss/ternary'):
            assert np.isfinite(vals[tag]), (tag, vals[tag])

    with open(str(log / 'train_pairs.txt')) as f:
        pairs = [line.split() for line in f]
    frames = [p for pr in pairs for p in pr]
    assert len(pairs) == 2 * (5 + 7) and all('kitti_raw' in p for p in frames)
    assert not any('drive_0005' in p and os.path.basename(p) in ('0000000010.png', '0000000011.png') for p in frames)
    assert any('drive_0005' in p and os.path.basename(p) == '0000000009.png' for p in frames)

    # resume (--no_eval: the evaluation was checked above, and a 384 x 1280 engine is the slow part of an invocation)
    out = _run(tmp_path, '--iters', '6', '--batch_size', '1', '--kitti_excludes', EXCLUDES, '--no_eval')
    assert 'training from i = 5 to 6' in out
    assert [step for step, _ in _events(str(log / 'train'))] == [1, 2, 3, 4, 5, 6]
    assert [step for step, _ in _events(str(log / 'eval'))] == [2, 4]
    assert (log / 'model.ckpt-6.index').is_file()


def test_run_command_chairs_and_debug(tmp_path, dev):
    from unflow_amd.core.input import decode_png
    rs = np.random.RandomState(1)
    for i in range(1, 3):
        for k in (1, 2):
            _png(str(tmp_path / 'data' / 'flying_chairs' / 'image' / ('%05d_img%d.png' % (i, k))), 64, 128, rs)
    out = _run(tmp_path, '--dataset', 'chairs', '--debug', '--no_eval', '--iters', '2')
    assert 'training from i = 1 to 2' in out and 'Warning' not in out
    log = tmp_path / 'log' / 'ex' / 'e'
    events = _events(str(log / 'train'))
    assert [step for step, vals in events if 'loss/combined' in vals] == [1, 2]
    images = [(step, vals) for step, vals in events if 'loss/combined' not in vals]
    assert [step for step, _ in images] == [1, 2]
    for _, vals in images:
        assert sorted(vals) == ['train/augmented1/image/0', 'train/augmented2/image/0']        # n < min(B, 3), B = 1
        for h, w, png in vals.values():
            im = decode_png(png)
            assert (h, w) == (64, 128) and im.shape == (64, 128, 3) and im.dtype == np.uint8
            assert im.std() > 1.0                                            # a picture, not a constant
    assert not [n for n in os.listdir(str(log / 'eval')) if n.startswith('events')]
    assert (tmp_path / 'ckpt' / 'e' / 'model.ckpt-2.index').is_file() and (log / 'model.ckpt-2.index').is_file()   # --debug keeps both


def test_run_command_kitti_ft(tmp_path, dev):
    """The supervised branch: finetune.py's batches (41 + 42 examples, 40 of each held out), loss/combined and the learning rate only."""
    from kitti_gt_fixture import make_gt_tree
    make_gt_tree(tmp_path / 'data', n_per_dataset=(41, 42), size=(72, 136))
    out = _run(tmp_path, '--dataset', 'kitti_ft', '--no_eval', '--iters', '2')
    assert 'training from i = 1 to 2' in out and 'Warning' not in out
    log = tmp_path / 'log' / 'ex' / 'e'
    events = _events(str(log / 'train'))
    assert [step for step, _ in events] == [1, 2]
    printed = [float(l) for l in re.findall(r'-- train: i = \d+, loss = (\S+)', out)]
    for (_, vals), loss in zip(events, printed):
        assert sorted(vals) == ['loss/combined', 'train/learning_rate']
        assert vals['loss/combined'] == float(np.float32(loss)) and np.isfinite(loss)
    assert not (log / 'train_pairs.txt').exists()                            # the raw-frame list is the unsupervised datasets'
    assert (log / 'model.ckpt-2.index').is_file()
