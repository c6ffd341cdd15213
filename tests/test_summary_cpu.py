"""core/summary.py against an event file assembled independently (tests/golden/make_events_golden.py: own CRC-32C table, own
protobuf and PNG writers, nothing of the package imported): the writer's bytes, the reader's round trip, damaged files."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'events_golden.tfevents')


def _maker():
    spec = importlib.util.spec_from_file_location('make_events_golden', os.path.join(HERE, 'golden', 'make_events_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write(tmp_path):
    from unflow_amd.core.summary import SummaryWriter
    G = _maker()
    w = SummaryWriter(str(tmp_path), wall_time=G.WALL_TIME, hostname='host')
    w.add_scalars(G.SCALAR_STEP, dict(G.SCALARS))
    w.add_images(G.IMAGE_STEP, {G.IMAGE_TAG: np.asarray(G.image_pixels(), dtype=np.uint8)})
    w.close()
    return w.path


def test_golden_file_is_what_its_script_builds():
    with open(GOLDEN, 'rb') as f:
        assert f.read() == _maker().build()


def test_writer_bytes_equal_the_independent_file(tmp_path):
    path = _write(tmp_path)
    assert os.path.basename(path) == 'events.out.tfevents.1500000000.host'
    with open(path, 'rb') as f, open(GOLDEN, 'rb') as g:
        assert f.read() == g.read()


def test_two_writers_of_one_folder_do_not_share_a_file(tmp_path):
    assert _write(tmp_path) != _write(tmp_path)
    assert len(os.listdir(str(tmp_path))) == 2


def test_read_events_round_trip():
    from unflow_amd.core.input import decode_png
    from unflow_amd.core.summary import read_events
    G = _maker()
    events = read_events(GOLDEN)
    assert [step for step, _ in events] == [G.SCALAR_STEP, G.IMAGE_STEP]
    scalars = events[0][1]
    assert list(scalars) == [t for t, _ in G.SCALARS]
    for tag, v in G.SCALARS:
        assert scalars[tag] == float(np.float32(v))
    h, w, png = events[1][1][G.IMAGE_TAG]
    assert (h, w) == (G.IMAGE_H, G.IMAGE_W)
    assert np.array_equal(decode_png(png), np.asarray(G.image_pixels(), dtype=np.uint8))


def test_negative_step_and_images_argument_check(tmp_path):
    from unflow_amd.core.summary import SummaryWriter, read_events
    with SummaryWriter(str(tmp_path)) as w:
        w.add_scalars(-3, {'a': 2.0})
        with pytest.raises(ValueError):
            w.add_images(1, {'x': np.zeros((2, 3, 3), dtype=np.float32)})
    assert read_events(w.path)[0] == (-3, {'a': 2.0})


def test_damaged_files_raise(tmp_path):
    from unflow_amd.core.summary import read_events
    with open(GOLDEN, 'rb') as f:
        good = f.read()
    first = 8 + 4 + int.from_bytes(good[:8], 'little') + 4            # size of the file-version record
    flipped = bytearray(good)
    flipped[first + 12 + 5] ^= 0x10                                     # a payload byte of the scalar record
    p = tmp_path / 'flipped'
    p.write_bytes(bytes(flipped))
    with pytest.raises(ValueError, match='checksum'):
        read_events(str(p))
    head = bytearray(good)
    head[first] ^= 0x01                                                 # the length of the scalar record
    p = tmp_path / 'length'
    p.write_bytes(bytes(head))
    with pytest.raises(ValueError, match='checksum'):
        read_events(str(p))
    for cut in (len(good) - 3, first + 6):                              # inside the last payload's checksum; inside a header
        p = tmp_path / ('cut%d' % cut)
        p.write_bytes(good[:cut])
        with pytest.raises(ValueError, match='truncated'):
            read_events(str(p))
