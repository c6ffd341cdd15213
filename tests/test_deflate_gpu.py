"""-m gpu: deflate on the device (csrc/deflate.hip, core/png_device.py) — unflow_deflate against the Python model
of deflate_ref.py byte for byte and through zlib.decompress, at a small chunk size and the default: the stream lengths around
a chunk, all zeros, uniform bytes (stored wins), Fibonacci counts (the length limit's repair rule), the run lengths around 3
and 258, a run across a chunk boundary, every source alignment, several streams with guard bytes in one launch; then
encode_png_device, FlowEstimator.export / export_sequence / pictures with deflate='device', and the host-side refusals."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import deflate_ref as D
import kitti_fixture
import png_filter_ref as R

pytestmark = pytest.mark.gpu

CHUNKS = (4096, None)                        # None: the package default


def _P():
    from unflow_amd.core import png_device as P
    return P


def _chunk(chunk):
    from unflow_amd import _lib
    return _lib.DEFLATE_CHUNK_DEFAULT if chunk is None else chunk


@functools.lru_cache(maxsize=None)
def _reference(chunk):
    """[(name, bytes, reference stream, codings)] of deflate_ref.cases, computed once per chunk size."""
    out = []
    for name, data in D.cases(chunk):
        codings = []
        out.append((name, data, D.deflate(data, chunk, codings), tuple(codings)))
    return out


def _pack(datas, dev, lead=0, gap=0):
    """The streams back to back (lead bytes in front, gap between) in one device buffer; spans [(offset, bytes)]."""
    parts, spans, pos = [bytes([0xEE]) * lead], [], lead
    for d in datas:
        spans.append((pos, len(d)))
        parts += [d, bytes([0xEE]) * gap]
        pos += len(d) + gap
    buf = np.frombuffer(b''.join(parts), dtype=np.uint8).copy()
    return torch.from_numpy(buf).to(dev), spans


# ------------------------------------------------------------------------------------------------- 1. kernel vs reference
@pytest.mark.parametrize("chunk", CHUNKS)
def test_kernel_equals_the_reference(chunk, dev):
    """Every case of deflate_ref.cases in ONE launch (the streams lie back to back, so they start at many alignments):
    lengths 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3 of zeros and of noise, uniform bytes, Fibonacci counts, runs of
    exactly 2, 3, 258, 259, 260, 516 (and 1, 257, 774), a run across a chunk boundary."""
    P, c = _P(), _chunk(chunk)
    ref = _reference(c)
    scan, spans = _pack([data for _, data, _, _ in ref], dev, lead=3)
    got = P.deflate_device(scan, spans, None, chunk)
    assert len(got) == len(ref)
    for (name, data, want, codings), z in zip(ref, got):
        assert zlib.decompress(z) == data, name
        assert z == want, (name, len(z), len(want), codings)
    by_name = {name: codings for name, _, _, codings in ref}
    assert by_name['uniform'] == (0,) and by_name['fibonacci'] == (1,) and by_name['runs'] == (2,)     # conditions on the inputs
    assert D.fibonacci_depth(dict((n, d) for n, d, _, _ in ref)['fibonacci']) > 15


def test_every_source_alignment(dev):
    """The same 1500 bytes (runs and noise) at source offsets 0 .. 15 mod 16, one stream each, chunk 512: the 16-byte loads of
    the staging and the byte loads at its ragged ends; and every stream is the same."""
    P = _P()
    data = D.runs_bytes([3, 40, 300]) + D.noise_bytes(1500 - len(D.runs_bytes([3, 40, 300])), 3)
    want = D.deflate(data, 512)
    buf = bytearray()
    spans = []
    for k in range(16):
        buf += bytes([0xEE]) * ((k - len(buf)) % 16)
        spans.append((len(buf), len(data)))
        buf += data
    base = torch.zeros(len(buf) + 16, dtype=torch.uint8, device=dev)
    lead = (-base.data_ptr()) % 16                                           # make offset k really k mod 16 in memory
    base[lead:lead + len(buf)] = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(dev)
    scan = base[lead:lead + len(buf)]
    assert sorted((scan.data_ptr() + o) % 16 for o, _ in spans) == list(range(16))
    got = P.deflate_device(scan, spans, None, 512)
    assert all(z == want for z in got), [k for k, z in enumerate(got) if z != want]
    assert zlib.decompress(got[5]) == data


def test_five_streams_with_guard_bytes(dev):
    """Five streams of different sizes in one launch through the low-level call, their output ranges with gaps: every byte
    before, between and behind the ranges — and inside a range behind the stream's end — keeps its 0xCD."""
    from unflow_amd import _lib
    P, chunk = _P(), 4096
    datas = [D.runs_bytes([5, 700]) + D.noise_bytes(1, 40), D.noise_bytes(4096, 41), D.runs_bytes([5, 700]) + D.noise_bytes(9000, 42),
             D.noise_bytes(333, 43, top=256), D.noise_bytes(4097, 44)]          # 712, 4096, 9711, 333 and 4097 bytes
    scan, spans = _pack(datas, dev, lead=7, gap=5)
    plan = P.DeflatePlan(spans, chunk)
    gap, lead = 13, 5
    rows = plan.rows.copy()
    rows[:, 2] += lead + gap * np.arange(len(datas))                         # odd gaps: the output starts at odd addresses
    n_out = plan.out_bytes + lead + gap * len(datas) + 9
    out = torch.full((n_out,), 0xCD, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(len(datas), dtype=torch.int64, device=dev)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    meta = torch.zeros(plan.meta_chunks * _lib.DEFLATE_META, dtype=torch.int32, device=dev)
    P.deflate_launch(scan, rows, torch.from_numpy(rows).to(dev), plan.max_chunks, chunk, scratch, meta, out, sizes,
                     torch.cuda.current_stream(dev))
    host, sz = out.cpu().numpy(), sizes.cpu().numpy().tolist()
    written = np.zeros(n_out, bool)
    for k, data in enumerate(datas):
        dst = int(rows[k, 2])
        want = D.deflate(data, chunk)
        assert sz[k] == len(want) and host[dst:dst + sz[k]].tobytes() == want, k
        written[dst:dst + sz[k]] = True
    assert (host[~written] == 0xCD).all()
    m = meta.cpu().numpy().reshape(-1, _lib.DEFLATE_META)
    codings = []
    for data in datas:
        D.deflate(data, chunk, codings)
    assert m[:, 3].tolist() == codings and {0, 1, 2} == set(codings)


# ------------------------------------------------------------------------------------------------- 2. PNG files
def test_encode_png_device_with_device_deflate(dev):
    from unflow_amd.core.input import decode_png
    P = _P()
    rng = np.random.RandomState(17)
    xs = [R.random_image(rng, 37, 53, kind) for kind in ('gray8', 'rgb8', 'rgb16')] + [R.random_image(rng, 200, 300, 'rgb16')]
    tens = [torch.from_numpy(x).to(dev) for x in xs]
    datas = P.encode_png_device(tens, deflate='device')
    assert -(-200 * (1 + 300 * 6) // _chunk(None)) > 1                       # the large image takes several chunks
    for x, d, back in zip(xs, datas, P.decode_png_device(datas, dev)):
        assert d[:8] == P.PNG_SIGNATURE and len(P._walk_chunks(d)[1]) == 1
        assert np.array_equal(back.cpu().numpy().reshape(x.shape), x)
        assert np.array_equal(decode_png(d).reshape(x.shape), x)
        scan = R.reference_scanlines(x)[0].tobytes()
        assert P._walk_chunks(d)[1][0] == D.deflate(scan, _chunk(None))      # the IDAT body is the model's stream
    small = P.encode_png_device(tens[:3], deflate='device', chunk_bytes=256)
    for x, d in zip(xs, small):
        assert np.array_equal(decode_png(d).reshape(x.shape), x)
    # deflate='host' is what it was
    assert P.encode_png_device(tens[:1], level=6) == P.encode_png_device(tens[:1], level=6, deflate='host')
    assert P.encode_png_device([], deflate='device') == []


def _params(est):
    """tests/test_sequence_gpu.py::_params: seed 31."""
    tfp = {k: v.cpu() for k, v in est.engine.init_params(seed=31).items()}
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    est.load_tf_params(tfp)


def test_export_with_device_deflate_equals_the_host_writers(dev, tmp_path, monkeypatch):
    """Flow, backward flow, occlusion masks and pictures of the synthetic KITTI tree: workers=2, deflate='device' against
    workers=0 — the same names, the same decoded pixels; the IDAT of every new file inflates to the filter kernel's
    scanlines; the captured graph is the same object."""
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.kitti.input import KITTIInput
    P = _P()
    monkeypatch.setattr(kitti_fixture, 'SIZES', [(90, 151), (86, 149), (90, 150)])
    kitti_fixture.make_tree(tmp_path / "kitti", n_pairs=3)
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(96, 160), device=dev, bidirectional=True, visual=True)
    _params(est)
    einput = KITTIInput(kitti_fixture.Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(96, 160))
    kw = dict(backward=True, occlusion=True, visual=True)
    host = est.export(einput.input_train_2012(), str(tmp_path / "host"), fmt='png', **kw)
    graph = est.graph
    devp = est.export(einput.input_train_2012(), str(tmp_path / "dev"), fmt='png', workers=2, deflate='device', **kw)
    assert est.graph is graph and graph is not None
    names = [os.path.basename(p) for p in host]
    assert names == [os.path.basename(p) for p in devp] and len(names) == 3 * 8
    assert sorted(os.listdir(str(tmp_path / "dev"))) == sorted(names)
    da = P.decode_png_device([open(os.path.join(str(tmp_path / "host"), n), 'rb').read() for n in names], dev)
    datas = [open(os.path.join(str(tmp_path / "dev"), n), 'rb').read() for n in names]
    for n, a, b, data in zip(names, da, P.decode_png_device(datas, dev), datas):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), n
        x = b.cpu().numpy()
        scan = R.reference_scanlines(x[:, :, 0] if x.shape[2] == 1 else x)[0].tobytes()
        idat = P._walk_chunks(data)[1]
        assert len(idat) == 1 and idat[0] == D.deflate(scan, _chunk(None)), n
    # .flo files are not compressed: the same bytes, beside the deflated occlusion masks
    hf = est.export(einput.input_train_2012(), str(tmp_path / "hflo"), fmt='flo', occlusion=True)
    pf = est.export(einput.input_train_2012(), str(tmp_path / "pflo"), fmt='flo', occlusion=True, workers=2, deflate='device')
    assert [os.path.basename(p) for p in hf] == [os.path.basename(p) for p in pf]
    for a, b in zip(hf, pf):
        if a.endswith('.flo'):
            assert open(a, 'rb').read() == open(b, 'rb').read()
        else:
            xa, xb = P.decode_png_device([open(a, 'rb').read(), open(b, 'rb').read()], dev)
            assert torch.equal(xa, xb)
    assert est.graph is graph
    with pytest.raises(ValueError):                                          # refused on the host, before any launch
        est.export(einput.input_train_2012(), str(tmp_path / "bad"), workers=0, deflate='device')
    with pytest.raises(ValueError):
        est.export(einput.input_train_2012(), str(tmp_path / "bad"), workers=2, deflate='gpu')


def test_pictures_and_write_pictures_with_device_deflate(dev, tmp_path, monkeypatch):
    """pictures(scanlines=True, deflate='device') hands zlib streams ('scanlines_kind' 'png_z') to write_pictures' pool: the
    files decode to the host writers' pixels."""
    from unflow_amd import visualize as V
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.kitti.input import KITTIInput
    P = _P()
    monkeypatch.setattr(kitti_fixture, 'SIZES', [(90, 151), (86, 149), (90, 150)])
    kitti_fixture.make_tree(tmp_path / "kitti", n_pairs=3)
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(96, 160), device=dev, visual=True)
    _params(est)
    einput = KITTIInput(kitti_fixture.Data(tmp_path / "kitti"), batch_size=2, normalize=False, dims=(96, 160))
    for d in ("host", "dev"):
        os.makedirs(str(tmp_path / d))
    host = V.write_pictures(est.pictures(einput.input_train_2012()), str(tmp_path / "host"))
    exs = list(est.pictures(einput.input_train_2012(), scanlines=True, deflate='device'))
    assert all(ex['scanlines_kind'] == 'png_z' for ex in exs)
    h, w, depth, ctype, z = exs[0]['scanlines']['flow']
    assert (depth, ctype) == (8, 2) and len(zlib.decompress(z)) == h * (1 + 3 * w)
    devp = V.write_pictures(iter(exs), str(tmp_path / "dev"), workers=2)
    assert [os.path.basename(p) for p in host] == [os.path.basename(p) for p in devp] and len(host) == 3 * 5
    for a, b in zip(host, devp):
        xa, xb = P.decode_png_device([open(a, 'rb').read(), open(b, 'rb').read()], dev)
        assert torch.equal(xa, xb), a
    with pytest.raises(ValueError):
        next(est.pictures(einput.input_train_2012(), deflate='device'))      # needs scanlines=True


def test_export_sequence_with_device_deflate(dev, tmp_path):
    from test_sequence_gpu import clip
    from unflow_amd.core.inference import FlowEstimator
    P = _P()
    est = FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), max_frame=(90, 151), device=dev, sequence=True)
    _params(est)
    frames = clip(5, 90, 151, 50, u8=True)
    host = est.export_sequence(frames, str(tmp_path / "host"), fmt='png')
    graph = est.graph
    devp = est.export_sequence(iter(frames), str(tmp_path / "dev"), fmt='png', workers=2, deflate='device')
    assert est.graph is graph and graph is not None
    assert [os.path.basename(p) for p in host] == [os.path.basename(p) for p in devp] == ['%06d_10.png' % i for i in range(4)]
    for a, b in zip(host, devp):
        xa, xb = P.decode_png_device([open(a, 'rb').read(), open(b, 'rb').read()], dev)
        assert xa.shape == (90, 151, 3) and xa.dtype == torch.uint16 and torch.equal(xa, xb), a
    with pytest.raises(ValueError):
        est.export_sequence(frames, str(tmp_path / "bad"), fmt='png', workers=0, deflate='device')


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_host_side_refusals(dev):
    P = _P()
    scan = torch.zeros(1000, dtype=torch.uint8, device=dev)
    for bad in (0, 65536, 4096.5, True):
        with pytest.raises(ValueError):
            P.deflate_device(scan, [(0, 1000)], None, bad)
        with pytest.raises(ValueError):
            P.encode_png_device([scan.view(10, 100)], deflate='device', chunk_bytes=bad)
    for spans in ([(0, 1001)], [(990, 11)], [(-1, 5)], [(0, 0)]):            # a table that leaves its buffer
        with pytest.raises(ValueError):
            P.deflate_device(scan, spans)
    with pytest.raises(ValueError):
        P.encode_png_device([scan.view(10, 100)], deflate='gpu')
    with pytest.raises(ValueError):
        P.deflate_device(scan.cpu(), [(0, 10)])
    assert zlib.decompress(P.deflate_device(scan, [(0, 1000)])[0]) == bytes(1000)
