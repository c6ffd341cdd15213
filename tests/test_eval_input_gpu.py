"""GPU: evaluation and fine-tuning input decoded on the device — unflow_png_to_window, unflow_png_to_flow_gt
(csrc/png_decode.hip), DeviceGTBatches / DeviceEvalBatches (core/png_device.py) behind KITTIInput's readers, and their consumers
(FlowEstimator.evaluate / export on device batches, the supervised Trainer, sequence inference on device frames).  Every
comparison is exact: the device path is bit-identical to the host path it replaces.  The PNG files come from tests/png_cases.py
with a random filter per row (Average and Paeth rows, 6-byte pixels); the host decoder reads each file once (cached)."""
import ctypes
import gc
import os
import threading

import numpy as np
import pytest
import torch

import png_cases as P
from unflow_amd import _lib
from unflow_amd.core import input as I
from unflow_amd.core import png_device as D
from unflow_amd.kitti import input as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEAN, STDDEV = np.asarray(I.Input.mean, dtype=np.float32), np.float32(I.Input.stddev)
CANARY = -7.0


class Data:
    def __init__(self, root):
        self.current_dir = str(root)


def loader_threads():
    return [t for t in threading.enumerate() if t.name.startswith(("png-producer", "png-inflate"))]


# ------------------------------------------------------------------------------------------------------------- kernels
def rgb_of(arr):
    """read_png_image's channel rule on a decoded array: high byte of 16 bit, grey replicated, alpha dropped."""
    a = (arr >> 8).astype(np.uint8) if arr.dtype == np.uint16 else arr
    a = np.repeat(a[:, :, :1], 3, axis=2) if a.shape[2] in (1, 2) else a[:, :, :3]
    return a.astype(np.float32)


def window_of(img, oy, ox, Hs, Ws):
    """Output (y, x) = img[y + oy, x + ox] inside the frame, 0 outside."""
    h, w = img.shape[:2]
    out = np.zeros((Hs, Ws) + img.shape[2:], dtype=img.dtype)
    y0, y1, x0, x1 = max(0, -oy), min(Hs, h - oy), max(0, -ox), min(Ws, w - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = img[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def pack(arrays):
    """Decoded frames back to back as the unfilter kernel leaves them -> (device bytes, [(offset, h, w, bpp, sample bytes)])."""
    blobs, geo, off = [], [], 0
    for a in arrays:
        b, depth, _, bpp = P.sample_bytes(a)
        geo.append((off, a.shape[0], a.shape[1], bpp, depth // 8))
        blobs.append(b.reshape(-1))
        off += b.size
    return torch.from_numpy(np.concatenate(blobs)).to(DEV), geo


@pytest.mark.parametrize("normalize", [False, True])
def test_to_window_against_numpy(normalize, tmp_path):
    Hs, Ws = 39, 51
    rs = np.random.RandomState(20)
    shapes = [(37, 53, 1, 8), (41, 50, 2, 8), (37, 53, 3, 8), (41, 50, 4, 8), (41, 50, 1, 16), (37, 53, 2, 16), (37, 53, 3, 16),
              (41, 50, 4, 16), (45, 60, 3, 8)]
    arrays = [P.random_image(rs, h, w, ch, depth) for h, w, ch, depth in shapes]
    dec, geo = pack(arrays)
    pad_crop = lambda a: (D.window_origin(a.shape[0], Hs), D.window_origin(a.shape[1], Ws))      # noqa: E731
    # (image, origin): crop-or-pad of every image (37 x 53: pad in y, odd; crop in x, even.  41 x 50: crop in y, pad in x, odd),
    # a window inside the 45 x 60 frame, windows that hang over one corner, and windows that miss the frame in one axis
    entries = [(k, pad_crop(a)) for k, a in enumerate(arrays)]
    entries += [(8, (4, 7)), (8, (0, 0)), (2, (-5, 10)), (7, (9, -6)), (6, (100, 0)), (3, (0, -51)), (0, (-39, 2)), (5, (2, 53))]
    rows = [(0,) + geo[k] + o for k, o in entries]
    bad_bpp = len(rows)
    rows.append((0, geo[2][0], 37, 53, 5, 1, 0, 0))                       # invalid: 5 bytes per pixel
    too_big = len(rows)
    rows.append((0, geo[8][0], 45, 61, 3, 1, 0, 0))                       # invalid: runs past the decoded buffer
    n = len(rows)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    out = torch.full((n + 1, Hs, Ws, 3), CANARY, dtype=torch.float32, device=DEV)       # one slot more than the launch has images
    mean_c = (ctypes.c_float * 3)(*[float(m) for m in MEAN]) if normalize else None
    _lib.check(_lib.lib().unflow_png_to_window(_lib.ptr(dec), _lib.cl(dec.numel()), _lib.ptr(table), n, Hs, Ws, mean_c,
                                               _lib.cf(STDDEV), _lib.ptr(out), _lib.stream(DEV)), "png_to_window")
    got = out.cpu().numpy()
    for i, (k, (oy, ox)) in enumerate(entries):
        want = window_of(rgb_of(arrays[k]), oy, ox, Hs, Ws)
        if normalize:
            want = (want - MEAN) / STDDEV
        assert want.dtype == np.float32 and np.array_equal(got[i], want), (i, shapes[k], oy, ox)
    for i in (bad_bpp, too_big, n):
        assert (got[i] == CANARY).all(), "slot %d was written" % i
    # and the crop-or-pad entries are Input._preprocess_image(read_png_image(file))
    inp = I.Input(None, 1, (Hs, Ws), normalize=normalize)
    for k, a in enumerate(arrays):
        f = tmp_path / ("%d.png" % k)
        f.write_bytes(P.encode_png(a, 0))
        want = inp._preprocess_image(I.read_png_image(str(f)))
        assert np.array_equal(got[k], want), shapes[k]


def test_to_flow_gt_against_numpy():
    Hs, Ws = 20, 28
    rs = np.random.RandomState(21)
    gt = P.random_image(rs, 21, 30, 3, 16)
    gt[..., 2] = np.asarray([0, 1, 2, 65535], dtype=np.uint16)[rs.randint(0, 4, size=(21, 30))]
    special = np.asarray([0, 32768, 65535, 32767, 32769, 1], dtype=np.uint16)
    pick = rs.rand(21, 30, 2) < 0.3
    gt[..., :2][pick] = special[rs.randint(0, len(special), size=int(pick.sum()))]
    gt[3, 4] = (0, 65535, 65535)                # the first pixel inside the window padded at the top and the left
    gt[0, 0] = (32768, 0, 2)
    rgb8, rgba16 = P.random_image(rs, 21, 30, 3, 8), P.random_image(rs, 21, 30, 4, 16)
    dec, geo = pack([gt, rgb8, rgba16])
    origins = [(-3, -4), (5, 10), (0, 0), (-25, 0), (1, 2)]               # pads top + left; bottom + right; none; misses; crop
    rows = [(0,) + geo[0] + o for o in origins] + [(0,) + geo[1] + (0, 0), (0,) + geo[2] + (0, 0)]      # 8-bit RGB, 16-bit RGBA
    n = len(rows)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    flow = torch.full((n + 1, Hs, Ws, 2), CANARY, dtype=torch.float32, device=DEV)
    mask = torch.full((n + 1, Hs, Ws), CANARY, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().unflow_png_to_flow_gt(_lib.ptr(dec), _lib.cl(dec.numel()), _lib.ptr(table), n, Hs, Ws, _lib.ptr(flow),
                                                _lib.ptr(mask), _lib.stream(DEV)), "png_to_flow_gt")
    gf, gm = flow.cpu().numpy(), mask.cpu().numpy()
    g = gt.astype(np.float32)                                             # read_kitti_flow_png's arithmetic
    want_flow, want_mask = (g[:, :, 0:2] - 2 ** 15) / 64.0, g[:, :, 2]
    assert want_flow.dtype == np.float32
    for i, (oy, ox) in enumerate(origins):
        assert np.array_equal(gf[i], window_of(want_flow, oy, ox, Hs, Ws)), (oy, ox)
        assert np.array_equal(gm[i], window_of(want_mask, oy, ox, Hs, Ws)), (oy, ox)
    assert set(np.unique(gm[0])) >= {0.0, 1.0, 2.0, 65535.0} and gf[0].min() == -512.0 and gf[0].max() == (65535 - 32768) / 64.0
    for i in range(len(origins), n + 1):                                  # skipped entries and the slot behind the launch
        assert (gf[i] == CANARY).all() and (gm[i] == CANARY).all(), "slot %d was written" % i


# ------------------------------------------------------------------------------------------------------------- trees
LAYOUTS = (('data_scene_flow/training', 'image_2'), ('data_stereo_flow/training', 'colored_0'))


def write_png(path, arr, rs):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(P.encode_png(arr, P.random_filters(rs, arr.shape[0])))


def flow_map(rs, h, w):
    u16 = P.random_image(rs, h, w, 3, 16)
    u16[..., :2] = 32768 + rs.randint(-640, 640, size=(h, w, 2))          # flows within +-10 px
    u16[..., 2] = rs.rand(h, w) < 0.6
    u16[0, 0], u16[h - 1, w - 1] = (0, 65535, 1), (65535, 0, 1)
    return u16


def make_kitti(root, sizes, seed, kinds=None, testing=()):
    """A KITTI tree with both training layouts: sizes[d][i] = (h, w) of example i of dataset d (frames _10 / _11, flow_occ and
    flow_noc maps), kinds[d][i] = (channels, depth) of its frames (default 8-bit RGB); testing: sizes of
    data_scene_flow/testing/image_2's pairs."""
    rs = np.random.RandomState(seed)
    for d, (base, img) in enumerate(LAYOUTS):
        for i, (h, w) in enumerate(sizes[d]):
            ch, depth = kinds[d][i] if kinds else (3, 8)
            for k in (10, 11):
                write_png(os.path.join(str(root), base, img, '%06d_%d.png' % (i, k)), P.random_image(rs, h, w, ch, depth), rs)
            for sub in ('flow_occ', 'flow_noc'):
                write_png(os.path.join(str(root), base, sub, '%06d_10.png' % i), flow_map(rs, h, w), rs)
    for i, (h, w) in enumerate(testing):
        for k in (10, 11):
            write_png(os.path.join(str(root), 'data_scene_flow/testing/image_2', '%06d_%d.png' % (i, k)),
                      P.random_image(rs, h, w, 3, 8), rs)


@pytest.fixture(scope="module")
def host():
    """The host readers over a cached decode_png: the interpreter decodes every file (Average / Paeth rows) once per module.
    read_png_image, read_kitti_flow_png and input_train_gt all decode through the module attribute patched here."""
    real_decode, cache = I.decode_png, {}

    def decode(data):
        if data not in cache:
            cache[data] = real_decode(data)
        return cache[data].copy()

    def patch(monkeypatch):
        monkeypatch.setattr(I, "decode_png", decode)
        monkeypatch.setattr(K, "decode_png", decode)
    return patch


@pytest.fixture(scope="module")
def gt_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("gt_tree")
    make_kitti(root, ([(72, 132)] * 3, [(75, 140)] * 3), seed=23)
    return root


@pytest.fixture(scope="module")
def eval_tree(tmp_path_factory):
    """Frame sizes below, equal to and above dims = (64, 96) on each axis, odd and even differences; a 16-bit and a grey pair."""
    root = tmp_path_factory.mktemp("eval_tree")
    make_kitti(root, ([(72, 101), (64, 96), (59, 90)], [(61, 110), (75, 96), (64, 85)]), seed=24,
               kinds=([(3, 8), (3, 16), (3, 8)], [(1, 8), (3, 8), (4, 8)]), testing=[(70, 90), (60, 100), (64, 96)])
    return root


def assert_batches_equal(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, torch.Tensor):
            assert g.device == DEV and g.dtype == torch.float32, (what, j)
            g = g.cpu().numpy()
        else:
            assert j == 2 and g.dtype == np.int32, (what, j)              # input_shape stays on the host
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), "%s, array %d" % (what, j)


# ------------------------------------------------------------------------------------------------------------- loaders
@pytest.mark.parametrize("normalize", [True, False])
def test_input_train_gt_on_the_device_equals_the_host(gt_tree, host, monkeypatch, normalize):
    """Three batches of four over six examples (the walk wraps, from shift 1), a ring of two slots: every batch is used by work
    enqueued on the current stream BEFORE the next next(), which is all the iterator promises."""
    host(monkeypatch)
    kin = K.KITTIInput(Data(gt_tree), 4, (64, 96), normalize=normalize)
    ref = kin.input_train_gt(0, seed=5, shift=1)
    it = kin.input_train_gt(0, seed=5, shift=1, device=DEV, workers=4, prefetch=1)
    assert type(it) is D.DeviceGTBatches
    try:
        kept = []
        for k in range(3):
            batch = next(it)
            assert [tuple(t.shape) for t in batch] == [(4, 64, 96, 3), (4, 64, 96, 3), (4, 64, 96, 2), (4, 64, 96, 1)]
            assert all(t.is_contiguous() for t in batch)
            kept.append([t.clone() for t in batch])
        for k, got in enumerate(kept):
            assert_batches_equal(got, next(ref), "batch %d" % k)
    finally:
        it.close()
    assert not loader_threads()
    with pytest.raises(RuntimeError):
        next(it)


@pytest.mark.parametrize("variant,hold_out_inv,normalize", [
    ("train_2015", None, False), ("train_2015", 2, True), ("train_2012", None, True), ("train_2012", 2, False),
    ("test_2015", None, True), ("test_2015", 2, False)])
def test_evaluation_readers_on_the_device_equal_the_host(eval_tree, host, monkeypatch, variant, hold_out_inv, normalize):
    host(monkeypatch)
    kin = K.KITTIInput(Data(eval_tree), 2, (64, 96), normalize=normalize)
    reader = getattr(kin, "input_" + variant)
    want = list(reader(hold_out_inv=hold_out_inv))
    it = reader(hold_out_inv=hold_out_inv, device=DEV, prefetch=1)
    assert type(it) is D.DeviceEvalBatches
    got = [[t.clone() if isinstance(t, torch.Tensor) else t for t in batch] for batch in it]
    assert [b[0].shape[0] for b in got] == ([2, 1] if hold_out_inv is None else [2])      # a short last batch
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == (7 if variant.startswith("train") else 3)
        assert_batches_equal(g, w, "%s batch %d" % (variant, k))
    assert not loader_threads()                                           # an exhausted iterator has stopped its threads
    with pytest.raises(StopIteration):
        next(it)


def test_loader_lifecycle(tmp_path):
    make_kitti(tmp_path, ([(20, 24)] * 2, [(20, 24)] * 2), seed=25)
    kin = K.KITTIInput(Data(tmp_path), 2, (16, 16), normalize=False)
    it = kin.input_train_gt(0, device=DEV)
    next(it)
    assert loader_threads()
    del it
    gc.collect()
    assert not loader_threads()
    it = K.KITTIInput(Data(tmp_path), 1, (16, 16), normalize=False).input_train_2015(device=DEV)      # two batches of one
    next(it)
    it.close()
    assert not loader_threads()
    with pytest.raises(RuntimeError):                                     # closed with a batch still to come: not a clean end
        next(it)
    # a corrupt ground-truth file: the worker's error surfaces from next(), and the threads stop
    bad = os.path.join(str(tmp_path), 'data_scene_flow/training/flow_occ/000001_10.png')
    rows, depth, ctype, bpp = P.sample_bytes(flow_map(np.random.RandomState(0), 20, 24))
    stream = P.filter_rows(rows, bpp, [0] * 20)
    stream[7, 0] = 7
    with open(bad, 'wb') as f:
        f.write(P.png_file(24, 20, 16, 2, stream.tobytes()))
    it = kin.input_train_2015(device=DEV)
    with pytest.raises(ValueError, match="bad PNG filter 7"):
        for _ in it:
            pass
    assert not loader_threads()
    # a ground-truth file that is no 16-bit RGB map is refused by name before anything is decoded
    with open(bad, 'wb') as f:
        f.write(P.encode_png(P.random_image(np.random.RandomState(1), 20, 24, 3, 8), 0))
    with pytest.raises(ValueError, match="000001_10.png"):
        list(kin.input_train_2015(device=DEV))
    with pytest.raises(ValueError, match="000001_10.png"):
        it = kin.input_train_gt(0, device=DEV)
        for _ in range(2):
            next(it)
    gc.collect()
    assert not loader_threads()


# ------------------------------------------------------------------------------------------------------------- consumers
def scaled_params(eng, seed):
    tfp = eng.init_params(seed=seed)
    return {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}


def files_of(folder):
    return {n: open(os.path.join(folder, n), 'rb').read() for n in sorted(os.listdir(folder))}


def test_estimator_evaluates_and_exports_device_batches_identically(tmp_path, host, monkeypatch):
    from unflow_amd.core.inference import FlowEstimator
    host(monkeypatch)
    make_kitti(tmp_path / "kitti", ([(60, 120), (64, 128), (70, 133)], []), seed=26)
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(72, 136), device=DEV, bidirectional=True,
                        visual=True)
    est.load_tf_params(scaled_params(est.engine, 6))
    kin = K.KITTIInput(Data(tmp_path / "kitti"), 2, (64, 128), normalize=False)
    want = est.evaluate(kin.input_train_2015())
    got = est.evaluate(kin.input_train_2015(device=DEV))
    assert want['num_examples'] == 3 and 'occ/F1' in want and len(want['occ_counts']) == 3
    assert got == want                                                    # every score, per-example row and occlusion count
    for name, kw in (("all", dict(backward=True, occlusion=True, visual=True)), ("two", dict(num=2))):
        a = est.export(kin.input_train_2015(), str(tmp_path / (name + "_host")), **kw)
        b = est.export(kin.input_train_2015(device=DEV), str(tmp_path / (name + "_dev")), **kw)
        assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b]
        fa, fb = files_of(str(tmp_path / (name + "_host"))), files_of(str(tmp_path / (name + "_dev")))
        assert list(fa) == list(fb) and len(fa) == len(a)
        for n in fa:
            assert fa[n] == fb[n], n
    assert len(a) == 2
    pics_h = list(est.pictures(kin.input_train_2015()))
    pics_d = list(est.pictures(kin.input_train_2015(device=DEV)))
    assert len(pics_d) == 3
    for ph, pd in zip(pics_h, pics_d):
        assert list(ph) == list(pd) and all(np.array_equal(ph[k], pd[k]) for k in ph)
    # a device batch is consumed whole: one larger than the estimator's batch cannot be
    big = K.KITTIInput(Data(tmp_path / "kitti"), 3, (64, 128), normalize=False).input_train_2015(device=DEV)
    try:
        with pytest.raises(ValueError, match="device batch of 3"):
            est.evaluate(big)
    finally:
        big.close()
    assert not loader_threads()


def test_supervised_trainer_fed_by_the_device_loader(gt_tree, host, monkeypatch):
    """Two FlowNetC steps, the step's graph captured while the loader's threads work on the next batches: engine.P is
    bit-identical to two steps fed by the host iterator."""
    from unflow_amd.core.train import Trainer
    host(monkeypatch)
    kin = K.KITTIInput(Data(gt_tree), 2, (64, 128), normalize=True)
    params = dict(flownet='C', learning_rate=1e-4, save_interval=2, display_interval=1)
    finals = []
    for device in (None, DEV):
        tr = Trainer(2, 64, 128, params, device=DEV, seed=3, augment=False, use_graph=True, supervised=True)
        it = kin.input_train_gt(0, seed=2, device=device)
        try:
            losses = []
            for _ in range(2):
                im1, im2, flow_gt, mask_gt = next(it)
                losses.append(float(tr.train_step(im1, im2, target=(flow_gt, mask_gt))))
            finals.append((losses, tr.engine.P.clone()))
        finally:
            if device is not None:
                it.close()
    # the loss VALUE is a sum of block partials by atomicAdd (csrc/supervised.hip: its last bits vary run to run); the gradients
    # and so the parameters are bit-reproducible
    assert np.isfinite(finals[0][0]).all() and np.allclose(finals[0][0], finals[1][0], rtol=1e-5, atol=0)
    assert torch.equal(finals[0][1], finals[1][1])
    assert not loader_threads()


def test_trainer_eval_fed_by_the_device_reader(tmp_path, host, monkeypatch):
    """Trainer.eval on batch-1 tuples whose input_shape is a host int32 array and whose other six entries are device tensors:
    the rows of the host-fed evaluation.  The inputs are bit-identical and the forward pass sums in a fixed order, so the flow
    is too: the outlier percentages, counts of 0 / 1 over a count, are exact.  AEE (unflow_flow_error_sums) and the loss add
    their block partials with atomicAdd in whatever order the blocks finish: non-negative fp32 terms, fewer than 100 partials
    at this size, each addition within 2^-24 relative — below 100 * 2^-24 = 6e-6; rtol 1e-5."""
    from unflow_amd.core.train import Trainer
    host(monkeypatch)
    make_kitti(tmp_path / "kitti", ([(60, 120), (64, 128), (59, 101)], []), seed=28)       # frames within dims: Trainer.eval undoes padding only
    params = dict(flownet='C', pyramid_loss=True, border_mask=True, ternary_weight=1.0, smooth_2nd_weight=3.0,
                  learning_rate=1e-4, save_interval=1, display_interval=1)
    from unflow_amd.core import tf_checkpoint as T
    tr = Trainer(1, 64, 128, params, device=DEV, seed=3, augment=False)
    # the checkpoint round trip is tests/test_eval_gpu.py's subject and costs seconds of host CRC per FlowNetC file: here the
    # evaluation engine takes its networks straight from memory
    tfp = scaled_params(tr.engine, 4)
    ckpt_dir = str(tmp_path / "ckpt")
    monkeypatch.setattr(T, "latest_checkpoint", lambda d: os.path.join(d, "model.ckpt-5"))
    monkeypatch.setattr(tr, "restore", lambda d, engine=None: engine.load_tf_params(tfp))
    kin = K.KITTIInput(Data(tmp_path / "kitti"), 1, (64, 128), normalize=False)
    seen = []

    def device_batches():
        for batch in kin.input_train_2015(device=DEV):
            seen.append([type(t) for t in batch] + [t.device for t in batch if isinstance(t, torch.Tensor)])
            yield batch
    want = tr.eval(lambda: kin.input_train_2015(), ckpt_dir, resized=(64, 128))
    got = tr.eval(device_batches, ckpt_dir, resized=(64, 128))
    assert seen == [[torch.Tensor] * 2 + [np.ndarray] + [torch.Tensor] * 4 + [DEV] * 6] * 3
    assert got['num_examples'] == want['num_examples'] == 3 and got['global_step'] == 5
    rows_g, rows_w = np.asarray(got['per_example']), np.asarray(want['per_example'])
    assert np.isfinite(rows_w).all() and (rows_w[:, 0] > 0).all()
    assert np.array_equal(rows_g[:, (1, 3)], rows_w[:, (1, 3)]), (rows_g, rows_w)
    assert np.allclose(rows_g[:, (0, 2, 4)], rows_w[:, (0, 2, 4)], rtol=1e-5, atol=0), (rows_g, rows_w)
    assert not loader_threads()


def test_sequence_inference_from_device_decoded_frames(tmp_path):
    from unflow_amd import sequence as S
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import save_checkpoint
    H, W = 64, 128
    rs = np.random.RandomState(27)
    fdir = tmp_path / "frames"
    base = rs.randint(0, 256, size=(H // 8 + 1, W // 8 + 3, 3)).astype(np.uint8)
    big = np.kron(base, np.ones((8, 8, 1), np.uint8))
    files = []
    for i in range(5):
        files.append(str(fdir / ("f%03d.png" % i)))
        write_png(files[-1], np.ascontiguousarray(big[:H, 2 * i:2 * i + W]), rs)
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=DEV, sequence=True)
    tfp = scaled_params(est.engine, 9)
    est.load_tf_params(tfp)
    host_frames = [S.read_frame(p) for p in files]
    dev_frames = list(S.device_frames(files, 2, DEV))
    assert len(dev_frames) == 5
    for a, b in zip(host_frames, dev_frames):
        assert b.device == DEV and b.dtype == torch.uint8 and np.array_equal(a, b.cpu().numpy())
    want = est.export_sequence(host_frames, str(tmp_path / "host"))
    got = est.export_sequence(S.device_frames(files, 2, DEV), str(tmp_path / "dev"))
    assert [os.path.basename(p) for p in got] == [os.path.basename(p) for p in want] == ['%06d_10.png' % i for i in range(4)]
    fh, fd = files_of(str(tmp_path / "host")), files_of(str(tmp_path / "dev"))
    assert fh == fd
    flows = est.estimate_sequence(dev_frames)
    assert max(float(np.abs(f).max()) for f in flows) > 0.05
    # the command line (in this process): the same files from the same checkpoint
    ck = tmp_path / "ckpt" / "clip"
    ck.mkdir(parents=True)
    save_checkpoint(str(ck / "model.ckpt-7"), tfp, 7)
    (ck / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-7"\n')
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp_path / "log", tmp_path / "ckpt"))
    argv = ['--ex', 'clip', '--frames', str(fdir), '--out', str(tmp_path / "cli"), '--batch', '2', '--net_size', str(H), str(W),
            '--config', str(cfg)]
    assert S.main(argv) == 0
    assert files_of(str(tmp_path / "cli" / "clip")) == fh
    assert S.main(argv + ['--host_decode', '--out', str(tmp_path / "cli_host")]) == 0
    assert files_of(str(tmp_path / "cli_host" / "clip")) == fh
    # read_frame's messages survive: a grey frame in the clip is refused by name, a broken file too
    grey = str(fdir / "f005.png")
    with open(grey, 'wb') as f:
        f.write(P.encode_png(P.random_image(rs, H, W, 1, 8), 0))
    for reader in (lambda: S.read_frame(grey), lambda: list(S.device_frames(files + [grey], 2, DEV))):
        with pytest.raises(ValueError) as err:
            reader()
        assert str(err.value) == "%s: not an 8-bit RGB PNG (uint8 (%d, %d, 1))" % (grey, H, W)
    with open(grey, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\nxxxx')
    with pytest.raises(ValueError, match="not a readable PNG"):
        list(S.device_frames([grey], 2, DEV))
    assert not loader_threads()
