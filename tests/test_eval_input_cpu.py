"""CPU (-m "not gpu"): the host half of the evaluation / fine-tuning input on the device (core/png_device.py) — the planners of
DeviceGTBatches and DeviceEvalBatches against the host iterators of kitti/input.py (file order, crop draws, pairing, origins),
the validation of ground-truth files, and the host-only behaviour of unflow_png_to_window / unflow_png_to_flow_gt."""
import ctypes
import os
import re

import numpy as np
import pytest

import png_cases as P
from kitti_gt_fixture import Data, make_gt_tree
from unflow_amd.core import input as I
from unflow_amd.core import png_device as D
from unflow_amd.core.inference import frame_origin
from unflow_amd.kitti import input as K


def coordinate_frame(h, w):
    """A frame whose pixels carry their own coordinates: a crop of it shows its origin."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return np.stack([yy, xx, np.zeros_like(yy)], axis=2).astype(np.float32)


def test_gt_planner_files_and_draws_equal_input_train_gt(tmp_path, monkeypatch):
    """Three batches of four over six examples from shift 5 (the walk wraps): the planner — which reads only headers — names
    the files the host iterator reads, in its order, with its (oy, ox)."""
    make_gt_tree(tmp_path, n_per_dataset=(3, 3), size=(72, 100))
    kin = K.KITTIInput(Data(tmp_path), 4, (64, 96), normalize=False)
    files = kin.train_gt_files(0)
    assert len(files) == 6
    seen = []

    def stub(path):
        seen.append(path)
        return coordinate_frame(72, 100)
    monkeypatch.setattr(K, "read_png_image", stub)
    host = kin.input_train_gt(0, seed=11, shift=5)
    plan = D.GTPlanner(files, 4, (64, 96), seed=11, shift=5)
    pos = 5
    for _ in range(3):
        del seen[:]
        im1, im2, flow, mask = next(host)
        got = plan.next_batch()
        assert [f for ex in got for f in ex[:2]] == seen
        for k, ex in enumerate(got):
            assert tuple(ex[:3]) == tuple(files[pos % 6])
            pos += 1
            assert ex[3][:2] == ex[4][:2] == ex[5][:2] == (72, 100) and ex[5][2:] == (16, 2)
            oy, ox = ex[6:]
            assert (oy, ox) == (int(im1[k, 0, 0, 0]), int(im1[k, 0, 0, 1])) == (int(im2[k, 0, 0, 0]), int(im2[k, 0, 0, 1]))
        roles = plan.files(got)
        assert [f[0] for f in roles] == [e[0] for e in got] + [e[1] for e in got] + [e[2] for e in got]
        assert [f[2] for f in roles] == [D.FRAME] * 8 + [D.GT] * 4
        assert [(f[3], f[4]) for f in roles] == [(e[6], e[7]) for e in got] * 3


SIZES = [(17, 30), (20, 33), (26, 25), (15, 36), (20, 30)]        # below, equal to and above dims = (20, 30); odd and even differences


def eval_tree(root):
    """data_stereo_flow/training/{colored_0, flow_occ, flow_noc}: headers only (all a planner may read)."""
    base = os.path.join(str(root), 'data_stereo_flow/training')
    for d in ('colored_0', 'flow_occ', 'flow_noc'):
        os.makedirs(os.path.join(base, d))
    for i, (h, w) in enumerate(SIZES):
        for k in (10, 11):
            with open(os.path.join(base, 'colored_0', '%06d_%d.png' % (i, k)), 'wb') as f:
                f.write(P.png_file(w, h, 8, 2, b''))
        for d in ('flow_occ', 'flow_noc'):
            with open(os.path.join(base, d, '%06d_10.png' % i), 'wb') as f:
                f.write(P.png_file(w, h, 16, 2, b''))


def size_of(path):
    return SIZES[int(os.path.basename(path)[:6])]


@pytest.mark.parametrize("hold_out_inv", [None, 3])
def test_eval_planner_pairing_and_origins_equal_input_train(tmp_path, monkeypatch, hold_out_inv):
    eval_tree(tmp_path)
    kin = K.KITTIInput(Data(tmp_path), 2, (20, 30), normalize=False)
    seen = []

    def image_stub(path):
        seen.append(path)
        return coordinate_frame(*size_of(path)) + 1.0          # + 1: a padded pixel (0) differs from pixel (0, 0)

    def flow_stub(path):
        import torch
        seen.append(path)
        h, w = size_of(path)
        return torch.zeros(h, w, 2), torch.ones(h, w, 1)
    monkeypatch.setattr(K, "read_png_image", image_stub)
    monkeypatch.setattr(K, "read_kitti_flow_png", flow_stub)
    captured = {}

    class Recorder:
        def __init__(self, pairs, batch_size, dims, normalize, mean, stddev, gt_lists=(), **kw):
            captured.update(pairs=pairs, batch_size=batch_size, dims=dims, gt_lists=gt_lists, kw=kw)
    monkeypatch.setattr(D, "DeviceEvalBatches", Recorder)
    assert isinstance(kin.input_train_2012(hold_out_inv=hold_out_inv, device='cuda:0', workers=3, prefetch=1), Recorder)
    assert captured['kw'] == dict(device='cuda:0', workers=3, prefetch=1)
    plan = D.EvalPlanner(captured['pairs'], captured['batch_size'], captured['dims'], captured['gt_lists'])
    n_ex = 0
    for batch in kin.input_train_2012(hold_out_inv=hold_out_inv):
        got = plan.next_batch()
        assert len(got) == batch[0].shape[0]
        assert [f[0] for ex in got for f in ex] == seen                    # im1, im2, occ, noc per example, in the host's order
        del seen[:]
        for k, ex in enumerate(got):
            assert [f[2] for f in ex] == [D.FRAME, D.FRAME, D.GT, D.GT]
            h, w = size_of(ex[0][0])
            assert tuple(batch[2][k]) == (h, w, 3) == (ex[0][1][0], ex[0][1][1], 3)
            for f in ex:
                assert (f[3], f[4]) == (-frame_origin(h, 20), -frame_origin(w, 30))
            # the origin is where the host's crop-or-pad put the frame: output (y, x) shows frame pixel (y + oy, x + ox)
            oy, ox = ex[0][3], ex[0][4]
            for y, x in ((0, 0), (19, 29), (10, 15), (0, 29), (19, 0)):
                inside = 0 <= y + oy < h and 0 <= x + ox < w
                want = (y + oy + 1.0, x + ox + 1.0) if inside else (0.0, 0.0)
                assert tuple(batch[0][k, y, x, :2]) == want
        n_ex += len(got)
    assert plan.next_batch() is None
    assert n_ex == (5 if hold_out_inv is None else 3)


def test_window_origin_is_crop_or_pad_for_every_difference():
    for size in (8, 9):
        for n in range(1, 20):
            o = D.window_origin(n, size)
            assert o == -frame_origin(n, size)
            a = (np.arange(n, dtype=np.float32) + 1).reshape(n, 1, 1)
            want = I.resize_image_with_crop_or_pad(a, size, 1).reshape(size)
            got = [a[y + o, 0, 0] if 0 <= y + o < n else 0.0 for y in range(size)]
            assert list(want) == got, (n, size)


def header_file(path, h, w, depth, ctype):
    with open(str(path), 'wb') as f:
        f.write(P.png_file(w, h, depth, ctype, b''))
    return str(path)


def test_ground_truth_files_are_validated_with_their_path(tmp_path):
    im = header_file(tmp_path / "im.png", 20, 30, 8, 2)
    good = header_file(tmp_path / "good.png", 20, 30, 16, 2)
    D.GTPlanner([(im, im, good)], 1, (16, 24), seed=0).next_batch()
    bad = {"eight_bit": (20, 30, 8, 2), "grey": (20, 30, 16, 0), "small": (15, 23, 16, 2)}
    for name, (h, w, depth, ctype) in bad.items():
        gt = header_file(tmp_path / (name + ".png"), h, w, depth, ctype)
        with pytest.raises(ValueError, match=re.escape(gt)):
            D.GTPlanner([(im, im, gt)], 1, (16, 24), seed=0).next_batch()
    # the window must also lie inside the second frame and inside im1 itself
    short = header_file(tmp_path / "short.png", 15, 30, 8, 2)
    with pytest.raises(ValueError, match=re.escape(short)):
        D.GTPlanner([(im, short, good)], 1, (16, 24), seed=0).next_batch()
    with pytest.raises(ValueError, match=re.escape(short)):
        D.GTPlanner([(short, im, good)], 1, (16, 24), seed=0).next_batch()
    # evaluation pads and crops, so a size is never wrong there — the format still is
    for name in ("eight_bit", "grey"):
        gt = str(tmp_path / (name + ".png"))
        with pytest.raises(ValueError, match=re.escape(gt)):
            D.EvalPlanner([(im, im)], 1, (16, 24), ([gt],)).next_batch()
    ex, = D.EvalPlanner([(im, im)], 1, (16, 24), ([str(tmp_path / "small.png")],)).next_batch()
    assert (ex[2][3], ex[2][4]) == (0, 0) and (ex[0][3], ex[0][4]) == (2, 3)
    with pytest.raises(ValueError):
        D.EvalPlanner([(im, im)], 1, (16, 24), ([good, good],))


def test_host_iterators_without_a_device_are_unchanged(tmp_path):
    make_gt_tree(tmp_path, n_per_dataset=(1, 1), size=(10, 12))
    kin = K.KITTIInput(Data(tmp_path), 2, (8, 8), normalize=False)
    batch = next(kin.input_train_gt(0))
    assert [type(t) for t in batch] == [np.ndarray] * 4 and batch[3].shape == (2, 8, 8, 1)
    im1, im2, shp = next(iter(kin.input_test('data_scene_flow/training/image_2')))
    assert type(im1) is np.ndarray and im1.shape == (1, 8, 8, 3) and tuple(shp[0]) == (10, 12, 3)
    # the host readers are still generators: a directory is listed at the first next(), not at the call
    gone = K.KITTIInput(Data(tmp_path / "nowhere"), 2, (8, 8), normalize=False)
    for it in (gone.input_train_2015(), gone.input_train_2012(hold_out_inv=1), gone.input_test_2015(), gone.input_train_gt(0)):
        with pytest.raises(OSError):
            next(it)


@pytest.fixture(scope="module")
def lib():
    from unflow_amd import build, _lib
    build.build()
    return _lib.lib()


def test_window_entries_answer_on_the_host(lib):
    n = ctypes.c_void_p(0)
    one = ctypes.c_void_p(64)          # never dereferenced: another pointer is NULL, or the shape is refused first
    L, F = ctypes.c_long, ctypes.c_float
    assert lib.unflow_png_to_window(n, L(16), n, 1, 4, 4, n, F(1), n, n) == -1
    assert lib.unflow_png_to_window(one, L(16), one, 1, 4, 4, n, F(1), n, n) == -1
    assert lib.unflow_png_to_window(one, L(16), n, 1, 4, 4, n, F(1), one, n) == -1
    assert lib.unflow_png_to_window(one, L(16), one, 1, 0, 4, n, F(1), one, n) == -5
    assert lib.unflow_png_to_window(one, L(16), one, 0, 4, 4, n, F(1), one, n) == -5
    assert lib.unflow_png_to_window(one, L(16), one, 65536, 4, 4, n, F(1), one, n) == -5
    assert lib.unflow_png_to_window(one, L(0), one, 1, 4, 4, n, F(1), one, n) == -5
    assert lib.unflow_png_to_window(one, L(16), one, 1, 1 << 15, 1 << 15, n, F(1), one, n) == -5
    mean = (ctypes.c_float * 3)(1, 2, 3)
    assert lib.unflow_png_to_window(one, L(16), one, 1, 4, 4, mean, F(0), one, n) == -5
    assert lib.unflow_png_to_flow_gt(n, L(16), n, 1, 4, 4, n, n, n) == -1
    assert lib.unflow_png_to_flow_gt(one, L(16), one, 1, 4, 4, n, one, n) == -1
    assert lib.unflow_png_to_flow_gt(one, L(16), one, 1, 4, 4, one, n, n) == -1
    assert lib.unflow_png_to_flow_gt(one, L(16), one, 1, 4, 0, one, one, n) == -5
    assert lib.unflow_png_to_flow_gt(one, L(16), one, 0, 4, 4, one, one, n) == -5
    assert lib.unflow_png_to_flow_gt(one, L(0), one, 1, 4, 4, one, one, n) == -5
    assert lib.unflow_png_to_flow_gt(one, L(16), one, 1, 1 << 15, 1 << 15, one, one, n) == -5
