"""GPU: the device PNG decoder — unflow_png_unfilter, unflow_png_to_batch (csrc/png_decode.hip), decode_png_device and
DevicePairBatches (core/png_device.py).  Every comparison is exact.  The expected image of an unfilter case is the array that
tests/png_cases.py encoded; the host decoder is used only where it is the reference by definition, on small frames."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

import png_cases as P
from unflow_amd import _lib
from unflow_amd.core import input as I
from unflow_amd.core.png_device import DevicePairBatches, decode_png_device

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
CH_DEPTH_OF_BPP = {1: (1, 8), 2: (2, 8), 3: (3, 8), 4: (4, 8), 6: (3, 16), 8: (4, 16)}


def unfilter(cases):
    """[(array [h,w,ch], filters per row), ...] -> ONE unflow_png_unfilter launch; returns the decoded byte rows per image
    and the expected ones."""
    streams, rows, want, src, dst = [], [], [], 0, 0
    for arr, filters in cases:
        b, depth, ctype, bpp = P.sample_bytes(arr)
        s = P.filter_rows(b, bpp, filters).reshape(-1)
        rows.append((src, dst, arr.shape[0], arr.shape[1], bpp, depth // 8, 0, 0))
        streams.append(s)
        want.append(b)
        src, dst = src + s.size, dst + b.size
    raw = torch.from_numpy(np.concatenate(streams)).to(DEV)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    dec = torch.full((dst + 64,), 0xA5, dtype=torch.uint8, device=DEV)        # 64 guard bytes behind the last image
    _lib.check(_lib.lib().unflow_png_unfilter(_lib.ptr(raw), _lib.cl(src), _lib.ptr(dec), _lib.cl(dst), _lib.ptr(table), len(rows),
                                              _lib.stream(DEV)), "png_unfilter")
    out = dec.cpu().numpy()
    assert (out[dst:] == 0xA5).all(), "bytes written behind the last image"
    got = [out[r[1]:r[1] + w.size].reshape(w.shape) for r, w in zip(rows, want)]
    return got, want


def assert_all_equal(got, want, names):
    bad = [n for g, w, n in zip(got, want, names) if not np.array_equal(g, w)]
    assert not bad, "%d of %d images differ: %s" % (len(bad), len(names), bad[:8])


def test_unfilter_every_filter_every_bpp():
    rs = np.random.RandomState(0)
    cases, names = [], []
    for bpp, (ch, depth) in CH_DEPTH_OF_BPP.items():
        for ft in P.FILTERS:
            cases.append((P.random_image(rs, 5, 7, ch, depth), [ft] * 5))
            names.append("bpp %d filter %d" % (bpp, ft))
    assert_all_equal(*unfilter(cases), names)


def test_unfilter_shapes_past_every_boundary():
    R = _lib.png_unfilter_rows()
    assert R > 1
    rs = np.random.RandomState(1)
    cases, names = [], []
    for depth in (8, 16):
        for h in (1, 2, R - 1, R, R + 1, 2 * R + 3):
            for w in (1, 2, 63, 64, 65, 131):
                first = len(cases) % 5                        # the first row takes each of the five filters in turn
                cases.append((P.random_image(rs, h, w, 3, depth), P.random_filters(rs, h, first=first)))
                names.append("RGB%d %dx%d first filter %d" % (depth, h, w, first))
    assert_all_equal(*unfilter(cases), names)


@pytest.mark.parametrize("ch,depth", [(3, 8), (4, 16)])
def test_unfilter_content_that_hits_the_arithmetic(ch, depth):
    """Bytes from {0, 1, 2} and {253, 254, 255}: Paeth ties and mod-256 wraps on almost every pixel; all-255 under Average: the
    9-bit sum (255 + 255) >> 1 = 255, not 127."""
    R = _lib.png_unfilter_rows()
    h, w = R + 6, 67
    rs = np.random.RandomState(2)
    cases, names = [], []
    for label, values in (("uniform", None), ("low", (0, 1, 2)), ("high", (253, 254, 255)), ("mixed ends", (0, 1, 2, 253, 254, 255))):
        for fl, filters in (("paeth", [4] * h), ("average", [3] * h), ("random", P.random_filters(rs, h))):
            cases.append((P.random_image(rs, h, w, ch, depth, values), filters))
            names.append("%s / %s" % (label, fl))
    cases.append((np.full((h, w, ch), 255 if depth == 8 else 65535, dtype=np.uint8 if depth == 8 else np.uint16), [3] * h))
    names.append("all 255 / average")
    assert_all_equal(*unfilter(cases), names)


def test_unfilter_one_launch_with_mixed_images():
    R = _lib.png_unfilter_rows()
    rs = np.random.RandomState(3)
    shapes = [(1, 1, 3, 8), (R + 2, 70, 1, 8), (9, 130, 4, 16), (33, 5, 2, 16)]
    cases = [(P.random_image(rs, h, w, ch, depth), P.random_filters(rs, h)) for h, w, ch, depth in shapes]
    assert_all_equal(*unfilter(cases), [str(s) for s in shapes])


def test_decode_png_device_equals_decode_png():
    rs = np.random.RandomState(4)
    datas = [open(os.path.join(GOLDEN, "tiny_kitti_flow.png"), "rb").read()]
    for ch in (1, 2, 3, 4):
        for depth in (8, 16):
            datas.append(P.encode_png(P.random_image(rs, 16, 24, ch, depth), P.random_filters(rs, 16)))
    got = decode_png_device(datas, device=DEV)
    assert len(got) == len(datas)
    for data, g in zip(datas, got):
        want = I.decode_png(data)
        assert g.device == DEV and tuple(g.shape) == want.shape
        g = g.cpu().numpy()
        assert g.dtype == want.dtype and np.array_equal(g, want)
    assert decode_png_device([], device=DEV) == []


@pytest.mark.parametrize("ch,depth", [(1, 8), (2, 8), (4, 8), (3, 8), (1, 16), (2, 16), (3, 16), (4, 16)])
@pytest.mark.parametrize("normalize", [False, True])
def test_to_batch_crops_channels_and_normalisation(ch, depth, normalize, tmp_path):
    """Windows at the four corners and in the interior of a 40 x 50 frame, and the whole frame, against read_png_image + numpy."""
    rs = np.random.RandomState(5 + ch + depth)
    arr = P.random_image(rs, 40, 50, ch, depth)
    f = tmp_path / "a.png"
    f.write_bytes(P.encode_png(arr, 0))
    ref = I.read_png_image(str(f))                                              # float32 [40,50,3]
    mean, stddev = np.asarray(I.Input.mean, dtype=np.float32), np.float32(I.Input.stddev)
    b, _, _, bpp = P.sample_bytes(arr)
    dec = torch.from_numpy(b.reshape(-1).copy()).to(DEV)
    for (H, W), origins in (((32, 32), [(0, 0), (0, 18), (8, 0), (8, 18), (3, 7)]), ((40, 50), [(0, 0)])):
        rows = [(0, 0, 40, 50, bpp, depth // 8, oy, ox) for oy, ox in origins]
        table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        out = torch.full((len(rows), H, W, 3), -7.0, dtype=torch.float32, device=DEV)
        mean_c = (ctypes.c_float * 3)(*[float(m) for m in mean]) if normalize else None
        _lib.check(_lib.lib().unflow_png_to_batch(_lib.ptr(dec), _lib.cl(dec.numel()), _lib.ptr(table), len(rows), H, W, mean_c,
                                                  _lib.cf(stddev), _lib.ptr(out), _lib.stream(DEV)), "png_to_batch")
        got = out.cpu().numpy()
        for k, (oy, ox) in enumerate(origins):
            want = ref[oy:oy + H, ox:ox + W]
            if normalize:
                want = (want - mean) / stddev
            assert want.dtype == np.float32 and np.array_equal(got[k], want), (H, W, oy, ox)


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """Six 72 x 80 RGB frames with mixed row filters on disk, and a read_png_image that decodes each of them once (the host
    decoder takes a good part of a second per frame of Average / Paeth rows; RawPairBatches reads every frame many times)."""
    d = tmp_path_factory.mktemp("frames")
    rs = np.random.RandomState(6)
    for i in range(6):
        (d / ("%06d.png" % i)).write_bytes(P.encode_png(P.random_image(rs, 72, 80, 3, 8), P.random_filters(rs, 72, first=i % 5)))
    real, cache = I.read_png_image, {}

    def cached(path):
        if path not in cache:
            cache[path] = real(path)
        return cache[path].copy()
    return str(d), cached


def loader_pairs(d):
    class Data:
        def get_raw_dirs(self):
            return [d]
    return Data()


def producer_threads():
    return [t for t in threading.enumerate() if t.name.startswith(("png-producer", "png-inflate"))]


@pytest.mark.parametrize("needs_crop,normalize,workers,prefetch", [
    (True, True, 8, 2), (True, False, 8, 2), (False, True, 8, 2), (False, False, 8, 2), (True, True, 1, 1)])
def test_loader_equals_raw_pair_batches(frames, monkeypatch, needs_crop, normalize, workers, prefetch):
    """Four consecutive batches of two examples over six pairs (the walk wraps) against RawPairBatches on the same seed.
    Without a crop RawPairBatches takes only frames of exactly `dims`, so that case runs at dims = the frame, (72, 80)."""
    d, cached = frames
    monkeypatch.setattr(I, "read_png_image", cached)
    dims = (64, 64) if needs_crop else (72, 80)
    inp = I.Input(loader_pairs(d), 2, dims, normalize=normalize)
    ref = inp.input_raw(needs_crop=needs_crop, seed=3)
    it = inp.input_raw(needs_crop=needs_crop, seed=3, device=DEV, workers=workers, prefetch=prefetch)
    assert type(ref) is I.RawPairBatches and type(it) is DevicePairBatches
    try:
        for k in range(4):
            want1, want2 = next(ref)
            im1, im2 = next(it)
            for got, want in ((im1, want1), (im2, want2)):
                assert got.device == DEV and got.dtype == torch.float32 and got.is_contiguous()
                assert tuple(got.shape) == (2,) + dims + (3,)
                assert np.array_equal(got.cpu().numpy(), want), "batch %d" % k
    finally:
        it.close()
    assert not producer_threads()
    with pytest.raises(RuntimeError):
        next(it)


def test_loader_without_crop_rejects_frames_of_another_size(frames):
    d, _ = frames
    inp = I.Input(loader_pairs(d), 2, (64, 64), normalize=False)
    with pytest.raises(ValueError):
        inp.input_raw(needs_crop=False, seed=0, device=DEV)
    with pytest.raises(ValueError):
        next(inp.input_raw(needs_crop=False, seed=0))
    assert not producer_threads()


def test_loader_reports_a_bad_file_and_stops(tmp_path):
    rs = np.random.RandomState(7)
    arr = P.random_image(rs, 8, 8, 3, 8)
    (tmp_path / "0.png").write_bytes(P.encode_png(arr, 4))
    rows, depth, ctype, bpp = P.sample_bytes(arr)
    stream = P.filter_rows(rows, bpp, [0] * 8)
    stream[5, 0] = 7
    (tmp_path / "1.png").write_bytes(P.png_file(8, 8, 8, 2, stream.tobytes()))
    pairs = [(str(tmp_path / "0.png"), str(tmp_path / "1.png"))]
    it = DevicePairBatches(pairs, 1, (8, 8), False, False, I.Input.mean, I.Input.stddev, 0, device=DEV)
    with pytest.raises(ValueError, match="bad PNG filter 7"):
        next(it)
    assert not producer_threads()


def test_dropping_the_iterator_stops_its_threads(frames):
    d, _ = frames
    it = I.Input(loader_pairs(d), 2, (64, 64)).input_raw(seed=1, device=DEV)
    next(it)
    assert producer_threads()
    del it
    import gc
    gc.collect()
    assert not producer_threads()


def test_loader_runs_beside_a_graph_capture(frames, monkeypatch):
    """StepRunner captures the step's hipGraph at the first train_step, when the loader's threads are already at work on the
    next batches.  A capture in the default (global) mode turns allocations and synchronising calls of ANY thread into errors, so
    the producer thread may only enqueue.  Here: graphs captured and replayed between next() calls, batches still exact."""
    d, cached = frames
    monkeypatch.setattr(I, "read_png_image", cached)
    inp = I.Input(loader_pairs(d), 2, (64, 64), normalize=True)
    ref = inp.input_raw(seed=5)
    it = inp.input_raw(seed=5, device=DEV, prefetch=2)
    x = torch.zeros(1024, device=DEV)
    try:
        for k in range(6):
            im1, im2 = next(it)                       # schedules a batch: its workers and the producer run during the capture
            got = im1.cpu().numpy(), im2.cpu().numpy()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(200):
                    x.add_(1.0)
            g.replay()
            want = next(ref)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "batch %d" % k
        torch.cuda.synchronize()
        assert float(x[0]) == 6 * 200
    finally:
        it.close()


def test_input_raw_on_the_device_feeds_trainer_run(frames, tmp_path):
    """test_input_raw_feeds_trainer_run with the device loader: PNG frames (Average / Paeth rows among them) -> device batches
    on the side stream -> train steps on the current stream -> checkpoints."""
    from unflow_amd.core.train import Trainer
    d, _ = frames
    inp = I.Input(loader_pairs(d), 2, (64, 64), normalize=False)
    params = dict(flownet='S', learning_rate=1e-4, decay_interval=100000, save_interval=2, display_interval=1)
    tr = Trainer(2, 64, 64, params, device=DEV, seed=1, augment=True, use_graph=False)
    ck = str(tmp_path / "ck")
    log = tr.run(0, 4, lambda off: inp.input_raw(shift=2 * off, seed=0, device=DEV), ck)
    assert [i for i, _ in log] == [1, 2, 3, 4] and all(np.isfinite(l) for _, l in log)
    assert tr.checkpoint_step(ck) == 4
