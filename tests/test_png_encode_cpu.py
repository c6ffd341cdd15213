"""CPU (-m "not gpu"): the host half of the device PNG encoder (core/png_device.py) — the reference filter rule of
png_filter_ref.py pinned against the project's own decoder, the writer pool, and the output flags of the four commands."""
import os
import threading
import time
import zlib

import numpy as np
import pytest

import png_filter_ref as R
from unflow_amd.core import input as I
from unflow_amd.core import png_device as P

WIDTHS, HEIGHTS, KINDS = (1, 2, 3, 63, 64, 65, 257), (1, 2, 5), ('gray8', 'rgb8', 'rgb16')


@pytest.mark.parametrize("kind", KINDS)
def test_reference_scanlines_decode_to_the_image(kind):
    rng = np.random.RandomState(KINDS.index(kind))
    for h in HEIGHTS:
        for w in WIDTHS:
            x = R.random_image(rng, h, w, kind)
            scan, filters, meta = R.reference_scanlines(x)
            assert scan.shape == (h, 1 + w * {'gray8': 1, 'rgb8': 3, 'rgb16': 6}[kind]) and (scan[:, 0] == filters).all()
            got = I.decode_png(P.assemble_png(*meta, scan.tobytes()))
            assert got.dtype == x.dtype and np.array_equal(got.reshape(x.shape), x), (kind, h, w)


@pytest.mark.parametrize("kind", ('rgb8', 'rgb16'))
def test_five_filter_case_has_every_filter_and_decodes(kind):
    x = R.five_filter_case(kind)
    scan, filters, meta = R.reference_scanlines(x)
    assert set(filters.tolist()) == {0, 1, 2, 3, 4}
    assert filters[0] == 1                       # a first row where Sub wins: 1, never 4
    assert np.array_equal(I.decode_png(P.assemble_png(*meta, scan.tobytes(), level=1)), x)


def test_the_rule_on_hand_made_rows():
    # an all-zero image: filter 0 everywhere; a constant first row: Sub (cost of one pixel) beats None, and ties with Paeth -> 1
    scan, filters = R.filter_rows(np.zeros((3, 6), np.uint8), 3)
    assert filters.tolist() == [0, 0, 0] and not scan.any()
    scan, filters = R.filter_rows(np.full((2, 9), 100, np.uint8), 3)
    assert filters.tolist() == [1, 2]
    assert scan[0].tolist() == [1] + [100] * 3 + [0] * 6 and scan[1].tolist() == [2] + [0] * 9
    # the cost is |int8|: byte 128 costs 128, byte 129 costs 127
    _, f = R.filter_rows(np.array([[128, 1]], np.uint8), 1)       # None: 128 + 1; Sub: 128 + |int8(129)| = 255
    assert f.tolist() == [0]


def _jobs(tmp_path, n=9):
    rng = np.random.RandomState(5)
    out = []
    for k in range(n):
        kind = KINDS[k % 3]
        x = R.random_image(rng, 4 + k, 30 + 7 * k, kind)
        scan, _, meta = R.reference_scanlines(x)
        out.append(('%02d_%s.png' % (k, kind), x, meta + (scan.tobytes(),)))
    return out


def _write(jobs, out_dir, workers, level=6):
    os.makedirs(out_dir)
    with P.DeviceFileWriter(workers, level) as pool:
        for name, _, payload in jobs:
            pool.submit(os.path.join(out_dir, name), 'png', payload)
        flow = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2)
        pool.submit(os.path.join(out_dir, 'f.flo'), 'flo', P.flo_file_bytes(flow))
    return pool


def test_pool_files_do_not_depend_on_the_worker_count(tmp_path):
    jobs = _jobs(tmp_path)
    p1 = _write(jobs, str(tmp_path / "w1"), 1)
    p4 = _write(jobs, str(tmp_path / "w4"), 4)
    names = [j[0] for j in jobs] + ['f.flo']
    assert [os.path.basename(p) for p in p1.paths] == names == [os.path.basename(p) for p in p4.paths]      # submission order
    assert p1.written == p4.written == len(names) and p1.file_bytes == p4.file_bytes
    for name, x, _ in jobs:
        a = (tmp_path / "w1" / name).read_bytes()
        assert a == (tmp_path / "w4" / name).read_bytes()
        assert np.array_equal(I.decode_png(a).reshape(x.shape), x)
    flow, _ = I.read_flo(str(tmp_path / "w4" / 'f.flo'))
    assert np.array_equal(flow.numpy(), np.arange(12, dtype=np.float32).reshape(2, 3, 2))
    tmp = str(tmp_path / "ref.flo")
    I.write_flo(tmp, flow.numpy())
    assert open(tmp, 'rb').read() == (tmp_path / "w1" / 'f.flo').read_bytes()


def test_pool_level_is_passed_to_deflate(tmp_path):
    jobs = _jobs(tmp_path, 3)
    _write(jobs, str(tmp_path / "l1"), 2, level=1)
    for name, x, payload in jobs:
        data = (tmp_path / "l1" / name).read_bytes()
        assert data == P.assemble_png(*payload, level=1)
        assert np.array_equal(I.decode_png(data).reshape(x.shape), x)
    with pytest.raises(ValueError):
        P.DeviceFileWriter(2, level=10)
    with pytest.raises(ValueError):
        P.assemble_png(2, 2, 8, 0, b'\0' * 5)                      # 2 rows of 1 + 2 bytes are 6


def test_pool_reports_the_first_failing_path(tmp_path):
    jobs = _jobs(tmp_path, 4)
    ok_dir = tmp_path / "ok"
    ok_dir.mkdir()
    bad = str(tmp_path / "missing_dir" / "x.png")
    pool = P.DeviceFileWriter(2)
    pool.submit(str(ok_dir / jobs[0][0]), 'png', jobs[0][2])
    pool.submit(bad, 'png', jobs[1][2])
    pool.submit(str(tmp_path / "missing_dir" / "y.png"), 'png', jobs[2][2])
    pool.submit(str(ok_dir / jobs[3][0]), 'png', jobs[3][2])
    with pytest.raises(RuntimeError) as e:
        pool.close()
    assert bad in str(e.value) and isinstance(e.value.__cause__, OSError)
    assert (ok_dir / jobs[0][0]).exists() and (ok_dir / jobs[3][0]).exists()      # the others were still written
    with pytest.raises(RuntimeError):
        pool.submit(bad, 'png', jobs[0][2])                                        # closed
    with pytest.raises(ValueError):
        P.DeviceFileWriter(1).submit(bad, 'jpeg', b'')


def test_pool_bounded_queue_blocks_the_producer(tmp_path):
    gate, seen = threading.Event(), []

    def slow(data, level):                       # a compressor that waits for the test
        gate.wait(30)
        return zlib.compress(data, level)
    pool = P.DeviceFileWriter(2, compress=slow)
    assert pool.bound == 4
    payload = _jobs(tmp_path, 1)[0][2]
    total = 11

    def produce():
        for k in range(total):
            pool.submit(str(tmp_path / ("%02d.png" % k)), 'png', payload)
            seen.append(pool.pending)
    t = threading.Thread(target=produce)
    t.start()
    deadline = time.monotonic() + 30
    while len(pool.paths) < pool.bound and time.monotonic() < deadline:      # the producer fills the bound ...
        time.sleep(0.001)
    # ... and cannot get further while the workers are held: submit number bound + 1 blocks
    assert len(pool.paths) == pool.bound and pool.pending == pool.bound and t.is_alive()
    gate.set()
    t.join(30)
    pool.close()
    assert not t.is_alive() and len(pool.paths) == total and pool.written == total
    assert pool.max_pending <= pool.bound and max(seen) <= pool.bound


def test_pool_workers_are_capped():
    pool = P.DeviceFileWriter(workers=10 ** 6)
    assert pool.workers == P.MAX_WORKERS == 16 and pool.bound == 32
    pool.close()
    pool = P.DeviceFileWriter(workers=0)
    assert pool.workers == 1
    pool.close()


def _clip_dir(tmp_path):
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(2):
        (d / ("%04d.png" % k)).write_bytes(I.encode_png8_rgb(np.zeros((64, 128, 3), np.uint8)))
    return str(d)


def _parsers(tmp_path):
    from unflow_amd import evaluate, evaluate_flo, sequence, visualize
    return [(evaluate, ['--ex', 'x']), (visualize, ['--ex', 'x']), (evaluate_flo, ['--ex', 'x', '--dataset', 'chairs']),
            (sequence, ['--ex', 'x', '--frames', _clip_dir(tmp_path)])]


def test_cli_output_flags(tmp_path, capsys):
    for mod, base in _parsers(tmp_path):
        a = mod.parse_args(base)
        assert (a.workers, a.level, a.host_encode, a.encode_workers) == (0, 6, False, 0), mod.__name__      # the commands' files stay the host writers' unless asked
        a = mod.parse_args(base + ['--workers', '3', '--level', '1'])
        assert (a.workers, a.level, a.encode_workers) == (3, 1, 3)
        a = mod.parse_args(base + ['--host_encode', '--workers', '8'])
        assert a.host_encode and a.workers == 8 and a.encode_workers == 0
        for bad in (['--level', '10'], ['--level', '-1'], ['--workers', '-1'], ['--level', 'fast']):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(base + bad)
            assert e.value.code == 2, (mod.__name__, bad)
        capsys.readouterr()


def test_estimator_signatures_default_to_the_host_writers():
    import inspect
    from unflow_amd.core.inference import FlowEstimator
    for fn in (FlowEstimator.export, FlowEstimator.export_sequence):
        p = inspect.signature(fn).parameters
        assert p['workers'].default == 0 and p['level'].default == 6
