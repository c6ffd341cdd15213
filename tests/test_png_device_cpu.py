"""CPU (-m "not gpu"): the host half of the device PNG decoder (core/png_device.py) — chunk parsing and inflate, the errors of
decode_png, the filter-byte check, the loader's pair order and crop draws, and the host-only behaviour of the two new entries."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

import png_cases as P
from unflow_amd.core import input as I
from unflow_amd.core.png_device import PairPlanner, png_header, png_scanlines

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("ch,depth", [(c, d) for c in (1, 2, 3, 4) for d in (8, 16)])
def test_scanlines_agree_with_the_writer(ch, depth, tmp_path):
    rs = np.random.RandomState(10 * ch + depth)
    arr = P.random_image(rs, 9, 11, ch, depth)
    filters = P.random_filters(rs, 9)
    rows, d, ctype, bpp = P.sample_bytes(arr)
    stream = P.filter_rows(rows, bpp, filters).tobytes()
    data = P.encode_png(arr, filters)
    h, w, got_depth, got_ctype, raw = png_scanlines(data)
    assert (h, w, got_depth, got_ctype) == (9, 11, depth, P.CTYPE_OF_CHANNELS[ch])
    assert bytes(raw) == stream
    f = tmp_path / "a.png"
    f.write_bytes(data)
    assert png_header(str(f)) == (9, 11, depth, P.CTYPE_OF_CHANNELS[ch])
    # and the writer itself is a PNG writer: the host decoder reads the array back
    assert np.array_equal(I.decode_png(data), arr)


def test_scanlines_of_a_file_split_over_several_idat_chunks():
    arr = P.random_image(np.random.RandomState(1), 6, 5, 3, 8)
    rows, depth, ctype, bpp = P.sample_bytes(arr)
    stream = P.filter_rows(rows, bpp, [4] * 6).tobytes()
    z = zlib.compress(stream)
    data = (b'\x89PNG\r\n\x1a\n' + P.chunk(b'IHDR', struct.pack('>IIBBBBB', 5, 6, 8, 2, 0, 0, 0)) + P.chunk(b'tEXt', b'k\0v') +
            P.chunk(b'IDAT', z[:7]) + P.chunk(b'IDAT', z[7:]) + P.chunk(b'IEND', b''))
    assert bytes(png_scanlines(data)[4]) == stream


def test_scanlines_raise_what_decode_png_raises():
    arr = P.random_image(np.random.RandomState(2), 4, 4, 3, 8)
    rows, depth, ctype, bpp = P.sample_bytes(arr)
    stream = P.filter_rows(rows, bpp, [0, 1, 2, 3]).tobytes()
    good = P.png_file(4, 4, 8, 2, stream)
    png_scanlines(good)
    cases = {
        "signature": (b'\x89PNX' + good[4:], ValueError),
        "no IHDR": (b'\x89PNG\r\n\x1a\n' + P.chunk(b'IDAT', zlib.compress(stream)) + P.chunk(b'IEND', b''), ValueError),
        "interlace": (P.png_file(4, 4, 8, 2, stream, interlace=1), NotImplementedError),
        "palette": (P.png_file(4, 4, 8, 3, stream), NotImplementedError),
        "depth 4": (P.png_file(4, 4, 4, 0, stream), NotImplementedError),
        "truncated": (P.png_file(4, 4, 8, 2, stream[:-5]), ValueError),
    }
    for name, (data, exc) in cases.items():
        with pytest.raises(exc) as dev_err:
            png_scanlines(data)
        with pytest.raises(exc) as host_err:
            I.decode_png(data)
        assert str(dev_err.value) == str(host_err.value), name


@pytest.mark.parametrize("row", [0, 2, 3])
def test_scanlines_reject_a_filter_byte_above_four(row):
    arr = P.random_image(np.random.RandomState(3), 4, 4, 3, 8)
    rows, depth, ctype, bpp = P.sample_bytes(arr)
    stream = P.filter_rows(rows, bpp, [0, 0, 0, 0])
    stream[row, 0] = 5
    with pytest.raises(ValueError, match="bad PNG filter 5"):
        png_scanlines(P.png_file(4, 4, 8, 2, stream.tobytes()))


@pytest.mark.parametrize("needs_crop", [True, False])
def test_planner_pair_order_and_crop_draws_equal_raw_pair_batches(needs_crop, tmp_path, monkeypatch):
    """RawPairBatches against a stubbed decode (a frame whose pixels carry their own coordinates, so a batch shows its crop
    windows) and the planner of DevicePairBatches, which reads only the IHDR: same files in the same order over a wrapping walk
    of the pair list, same windows."""
    sizes = [(20, 30), (24, 28), (20, 30), (22, 33), (26, 30)] if needs_crop else [(16, 18)] * 5
    files = []
    for i, (h, w) in enumerate(sizes):
        f = tmp_path / ("%02d.png" % i)
        f.write_bytes(P.png_file(w, h, 8, 2, b''))          # a header is all the planner may read
        files.append(str(f))
    pairs = [(files[i], files[(i + 1) % 5]) for i in range(5)]
    dims = (16, 18)
    seen = []

    def stub(path):
        h, w = sizes[files.index(path)]
        seen.append(path)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        return np.stack([yy, xx, np.zeros_like(yy)], axis=2).astype(np.float32)
    monkeypatch.setattr(I, "read_png_image", stub)
    ref = I.RawPairBatches(pairs, 3, dims, needs_crop, False, [0, 0, 0], 1.0, seed=7)
    plan = PairPlanner(pairs, 3, dims, needs_crop, seed=7)
    for _ in range(4):                                       # 12 examples: wraps the five pairs twice
        del seen[:]
        im1, im2 = next(ref)
        got = plan.next_batch()
        assert [f for ex in got for f in ex[:2]] == seen
        for k, (fn1, fn2, m1, m2, oy, ox) in enumerate(got):
            assert m1[:2] == sizes[files.index(fn1)] and m2[:2] == sizes[files.index(fn2)]
            assert (oy, ox) == (int(im1[k, 0, 0, 0]), int(im1[k, 0, 0, 1])) == (int(im2[k, 0, 0, 0]), int(im2[k, 0, 0, 1]))


def test_planner_rejects_what_raw_pair_batches_rejects(tmp_path):
    f = tmp_path / "a.png"
    f.write_bytes(P.png_file(30, 20, 8, 2, b''))
    with pytest.raises(ValueError):
        PairPlanner([(str(f), str(f))], 1, (16, 18), False, seed=0).next_batch()      # no crop: the frame must be dims
    with pytest.raises(ValueError):
        PairPlanner([(str(f), str(f))], 1, (24, 18), True, seed=0).next_batch()       # a window taller than the frame


def test_input_raw_without_a_device_is_unchanged(tmp_path):
    for i in range(4):
        (tmp_path / ("%06d.png" % i)).write_bytes(I.encode_png8_rgb(np.full((8, 8, 3), i, dtype=np.uint8)))

    class Data:
        def get_raw_dirs(self):
            return [str(tmp_path)]
    it = I.Input(Data(), 2, (8, 8), normalize=False).input_raw(needs_crop=False)
    assert type(it) is I.RawPairBatches
    assert next(it)[0].shape == (2, 8, 8, 3)


@pytest.fixture(scope="module")
def lib():
    from unflow_amd import build, _lib
    build.build()
    return _lib.lib()


def test_new_entries_answer_on_the_host(lib):
    from unflow_amd import _lib
    n = ctypes.c_void_p(0)
    one = ctypes.c_void_p(64)          # never dereferenced: the other pointer is NULL
    L = ctypes.c_long
    assert lib.unflow_png_unfilter_rows() > 0
    assert _lib.png_unfilter_rows() == lib.unflow_png_unfilter_rows()
    assert lib.unflow_png_unfilter(n, L(16), n, L(16), n, 1, n) == -1
    assert lib.unflow_png_unfilter(one, L(16), one, L(16), n, 1, n) == -1
    assert lib.unflow_png_unfilter(one, L(16), one, L(16), one, 0, n) == -5
    assert lib.unflow_png_to_batch(n, L(16), n, 1, 4, 4, n, ctypes.c_float(1), n, n) == -1
    assert lib.unflow_png_to_batch(one, L(16), one, 1, 4, 4, n, ctypes.c_float(1), n, n) == -1
    assert lib.unflow_png_to_batch(one, L(16), one, 1, 0, 4, n, ctypes.c_float(1), one, n) == -5
    mean = (ctypes.c_float * 3)(1, 2, 3)
    assert lib.unflow_png_to_batch(one, L(16), one, 1, 4, 4, mean, ctypes.c_float(0), one, n) == -5
