"""CPU (-m "not gpu"): the deflate rule of unflow_deflate on its reference model tests/deflate_ref.py — every case
the GPU test codes inflates to its input under zlib with zlib's Adler-32; the size of the format against zlib's own Huffman-only
and RLE strategies; a 'png_z' payload through the writer pool; the new symbols."""
import os
import re
import zlib

import numpy as np
import pytest

import deflate_ref as D
import png_filter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (4096, D.CHUNK_DEFAULT)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_reference_streams_inflate_to_their_input(chunk):
    used = set()
    for name, data in D.cases(chunk):
        codings = []
        z = D.deflate(data, chunk, codings)
        assert zlib.decompress(z) == data, name
        assert int.from_bytes(z[-4:], 'big') == zlib.adler32(data), name
        assert z[:2] == b'\x78\x01' and len(z) <= D.stream_bound(len(data), chunk), name
        assert len(codings) == D.chunk_count(len(data), chunk)
        used |= set(codings)
        if name == 'uniform':
            assert codings == [0], codings                       # all 256 values uniformly: stored wins
        if name == 'fibonacci':
            assert codings == [1] and D.fibonacci_depth(data) > 15, (codings, D.fibonacci_depth(data))   # the repair rule ran
        if name.startswith('zeros_') and len(data) >= 64:
            assert set(codings) <= {0, 2} and codings[0] == 2, (name, codings)
    assert used == {0, 1, 2}


def test_run_splitting_loses_nothing():
    """Runs of exactly 2, 3, 258, 259, 260, 516: the tokens of coding 2 rebuild the bytes, matches are 3 .. 258 long."""
    for L in (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 518, 519, 774, 1000):
        data = b'\x01\x02' + b'\x05' * (L + 1) + b'\x06'
        toks = D.tokens(data, 2)
        out = bytearray()
        for kind, v in toks:
            assert kind == 0 or 3 <= v <= 258, (L, toks)
            out += bytes([v]) if kind == 0 else bytes([out[-1]]) * v
        assert bytes(out) == data, L
        matched = sum(v for kind, v in toks if kind)
        assert matched == (L if L >= 3 and L % 258 >= 3 or L % 258 == 0 and L >= 3 else L - L % 258 if L >= 3 else 0), (L, toks)


def test_length_limit_and_canonical_codes():
    counts = [0] * 286
    for s, c in zip(range(0, 60, 2), [1, 1, 3, 4] + [0] * 26):
        counts[s] = c
    a, b = 3, 4
    for s in range(8, 60, 2):
        a, b = b, a + b
        counts[s] = b
    lens = D.huff_lengths(counts, 15)
    assert max(lens) == 15 and sum(2.0 ** -v for v in lens if v) == 1.0             # limited, and still a complete code
    order = sorted((s for s in range(286) if counts[s]), key=lambda s: (counts[s], s))
    assert [lens[s] for s in order] == sorted((lens[s] for s in order), reverse=True)
    codes = D.canonical_codes(lens)
    words = sorted(format(codes[s], '0%db' % lens[s]) for s in order)
    assert all(not y.startswith(x) for x, y in zip(words, words[1:]))                # prefix-free
    assert D.huff_lengths([0, 5, 0], 7) == [0, 1, 0] and D.huff_lengths([0, 0], 7) == [0, 0]


def test_size_against_zlib_huffman_only_and_rle():
    """A condition on the FORMAT: for the synthetic noisy flow map, the 0 / 255 mask and png_filter_ref.random_image at 96 x 160,
    the stream is no larger than the smaller of zlib's Z_HUFFMAN_ONLY and Z_RLE streams of the same bytes plus n_chunks x
    HEADER_BOUND_BYTES (268, derived in deflate_ref from the header encoding) plus SLACK for zlib's finer block adaptivity.
    Measured here against zlib (chunk 16384; stream, min of zlib's two, excess before any allowance):
        flow 39715 / 39460 / +255,  mask 311 / 311 / 0,  rgb16 picture 69371 / 69285 / +86   (6, 1 and 6 chunks)
    — zlib at memLevel 9 closes a block every 32767 symbols, two of these chunks, and at most 43 bytes per chunk separate the
    two: its adaptivity buys nothing here that the per-chunk header allowance (268) does not cover already.  SLACK = 0."""
    SLACK = 0
    scan, _, _ = R.reference_scanlines(R.random_image(np.random.RandomState(0), 96, 160, 'rgb16'))
    inputs = [('flow', D.noisy_flow_scanlines()), ('mask', D.mask_scanlines()), ('picture', scan.tobytes())]
    for name, data in inputs:
        z = D.deflate(data, D.CHUNK_DEFAULT)
        assert zlib.decompress(z) == data
        best = min(len(D.zlib_stream(data, zlib.Z_HUFFMAN_ONLY)), len(D.zlib_stream(data, zlib.Z_RLE)))
        allowance = D.chunk_count(len(data), D.CHUNK_DEFAULT) * D.HEADER_BOUND_BYTES + SLACK
        print("%s: %d bytes -> %d, zlib %d, excess %+d, allowance %d" % (name, len(data), len(z), best, len(z) - best, allowance))
        assert len(z) <= best + allowance, (name, len(z), best, allowance)


def test_png_z_payload_through_the_writer_pool(tmp_path):
    from unflow_amd.core.input import decode_png
    from unflow_amd.core.png_device import DeviceFileWriter, assemble_png_z
    rng = np.random.RandomState(4)
    xs = [R.random_image(rng, 37, 53, kind) for kind in ('gray8', 'rgb8', 'rgb16')]
    paths = [str(tmp_path / ("%d.png" % k)) for k in range(len(xs))]
    with DeviceFileWriter(workers=2) as pool:
        for x, p in zip(xs, paths):
            scan, _, (h, w, depth, ctype) = R.reference_scanlines(x)
            pool.submit(p, 'png_z', (h, w, depth, ctype, D.deflate(scan.tobytes(), 4096)))
    assert pool.written == 3 and pool.paths == paths
    for x, p in zip(xs, paths):
        data = open(p, 'rb').read()
        assert np.array_equal(decode_png(data).reshape(x.shape), x)
    scan, _, (h, w, depth, ctype) = R.reference_scanlines(xs[2])
    assert open(paths[2], 'rb').read() == assemble_png_z(h, w, depth, ctype, D.deflate(scan.tobytes(), 4096))
    with pytest.raises(ValueError):
        DeviceFileWriter(workers=1).submit(paths[0], 'png_zz', None)


def test_new_symbols_in_the_header_and_the_binding():
    from unflow_amd import _lib, build
    build.build()
    txt = open(os.path.join(ROOT, "include", "unflow_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ('unflow_deflate', 'unflow_deflate_segment_bound', 'unflow_deflate_stream_bound', 'unflow_deflate_slot_bytes'):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(_lib.lib(), name), name
    for macro, value in (('UNFLOW_DEFLATE_FIELDS', _lib.DEFLATE_FIELDS), ('UNFLOW_DEFLATE_META', _lib.DEFLATE_META),
                         ('UNFLOW_DEFLATE_CHUNK_MAX', _lib.DEFLATE_CHUNK_MAX),
                         ('UNFLOW_DEFLATE_CHUNK_DEFAULT', _lib.DEFLATE_CHUNK_DEFAULT)):
        assert re.search(r"#define %s %d\b" % (macro, value), code), macro
    assert _lib.DEFLATE_CHUNK_DEFAULT == D.CHUNK_DEFAULT and _lib.DEFLATE_CHUNK_MAX == D.CHUNK_MAX
    # the host-only sizes, without a GPU
    assert _lib.deflate_segment_bound(4096) == 4101 and _lib.deflate_segment_bound() == D.CHUNK_DEFAULT + 5
    for n, c in ((1, 4096), (4096, 4096), (4097, 4096), (100000, 65535)):
        assert _lib.deflate_stream_bound(n, c) == D.stream_bound(n, c)
    from unflow_amd.core import png_device as P
    assert _lib.deflate_slot_bytes(4096) == P.deflate_slot_bytes(4096) == 4112 + 16
    for bad in (0, 65536, -1):
        with pytest.raises(ValueError):
            _lib.deflate_segment_bound(bad)
        with pytest.raises(ValueError):
            P.check_chunk_bytes(bad)


def test_host_refusals_need_no_gpu():
    from unflow_amd.core import png_device as P
    plan = P.DeflatePlan([(0, 5000), (5000, 100)], 4096)
    assert plan.rows[0, :6].tolist() == [0, 5000, 0, 2 + 5000 + 10 + 4, 0, 0] and plan.max_chunks == 2 and plan.meta_chunks == 3
    ok = dict(in_bytes=5100, out_bytes=plan.out_bytes, scratch_bytes=plan.scratch_bytes, meta_chunks=plan.meta_chunks)
    P.check_deflate_table(plan.rows, 4096, **ok)
    for field, value in ((0, 5001), (1, 0), (2, -1), (2, plan.out_bytes), (3, 5015), (4, 8), (4, plan.scratch_bytes), (5, 3)):
        rows = plan.rows.copy()
        rows[1 if field in (0, 5) else 0, field] = value
        with pytest.raises(ValueError):
            P.check_deflate_table(rows, 4096, **ok)
    rows = plan.rows.copy()
    rows[1, 2] = 16                                            # overlaps stream 0's range
    with pytest.raises(ValueError):
        P.check_deflate_table(rows, 4096, **ok)
    for mode, workers in (('gpu', 2), ('device', 0)):
        with pytest.raises(ValueError):
            P.check_deflate_mode(mode, workers)
    assert P.check_deflate_mode('device', 1) and not P.check_deflate_mode('host', 0)
