"""TensorBoard event files without TensorFlow: what tf.summary.FileWriter leaves in the train/ and eval/ folders of an experiment
(train.py:208-213, 254-255, 365-370), written and read on the host with the record checksum and the protobuf wire helpers of
core/tf_checkpoint.py.

File     events.out.tfevents.<unix time, 10 digits>.<host name>: a sequence of TFRecords
Record   uint64 little-endian payload length | masked CRC-32C of those 8 bytes | payload | masked CRC-32C of the payload
Payload  a serialized Event.  The first one of a file is Event{wall_time = 1: double, file_version = 3: "brain.Event:2"}, every
         later one Event{wall_time = 1, step = 2: int64, summary = 5: Summary}
Summary  repeated value = 1: Value{tag = 1: string, simple_value = 2: float}  or
                             Value{tag = 1, image = 4: Image{height = 1, width = 2, colorspace = 3 (always 3, RGB),
                                                             encoded_image_string = 4: PNG bytes}}
The PNG bytes are those of core/input.encode_png8_rgb.  One process writes (rank 0); nothing here needs torch or a GPU."""
import os
import socket
import struct
import time

from .tf_checkpoint import _field, _mask, _proto_fields, _put_varint, crc32c

FILE_VERSION = b'brain.Event:2'


def _double_field(fn, value):
    return _put_varint((fn << 3) | 1) + struct.pack('<d', float(value))


def _float_field(fn, value):
    return _field(fn, 5, struct.unpack('<I', struct.pack('<f', float(value)))[0])


def _record(payload):
    head = struct.pack('<Q', len(payload))
    return head + struct.pack('<I', _mask(crc32c(head))) + payload + struct.pack('<I', _mask(crc32c(payload)))


def version_event(wall_time):
    return _double_field(1, wall_time) + _field(3, 2, FILE_VERSION)


def scalar_value(tag, value):
    return _field(1, 2, _field(1, 2, tag.encode('utf-8')) + _float_field(2, value))


def image_value(tag, height, width, png):
    image = _field(1, 0, int(height)) + _field(2, 0, int(width)) + _field(3, 0, 3) + _field(4, 2, bytes(png))
    return _field(1, 2, _field(1, 2, tag.encode('utf-8')) + _field(4, 2, image))


def summary_event(wall_time, step, values):
    """values: the concatenated scalar_value / image_value fields of one Summary."""
    return _double_field(1, wall_time) + _field(2, 0, int(step) & 0xffffffffffffffff) + _field(5, 2, values)


class SummaryWriter:
    """tf.summary.FileWriter(logdir) for scalars and RGB images: one new event file per writer (a resumed run adds a second file
    to the folder, as the reference's per-chunk writers do), every record flushed when it is added.  wall_time: a fixed value
    for every record (tests); None = the clock."""

    def __init__(self, logdir, wall_time=None, hostname=None):
        os.makedirs(logdir, exist_ok=True)
        self._fixed = wall_time
        now = self._now()
        stem = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), hostname or socket.gethostname()))
        self.path, n = stem, 0
        while os.path.exists(self.path):          # two writers of one folder within a second
            n += 1
            self.path = '%s.%d' % (stem, n)
        self._f = open(self.path, 'wb')
        self._write(version_event(now))

    def _now(self):
        return time.time() if self._fixed is None else self._fixed

    def _write(self, payload):
        self._f.write(_record(payload))
        self._f.flush()

    def add_scalars(self, step, scalars):
        """One Event at `step` with a simple_value per {tag: number}, in the dict's order."""
        self._write(summary_event(self._now(), step, b''.join(scalar_value(t, v) for t, v in scalars.items())))

    def add_images(self, step, images):
        """One Event at `step` with an image per {tag: uint8 [h,w,3]}."""
        from .input import encode_png8_rgb
        vals = []
        for tag, im in images.items():
            h, w, c = im.shape
            if c != 3 or str(im.dtype) != 'uint8':
                raise ValueError("add_images: %r must be uint8 [h,w,3], got %s %s" % (tag, im.dtype, tuple(im.shape)))
            vals.append(image_value(tag, h, w, encode_png8_rgb(im)))
        self._write(summary_event(self._now(), step, b''.join(vals)))

    def close(self):
        if not self._f.closed:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _one(fields, number, default=None):
    vals = [v for fn, _, v in fields if fn == number]
    return vals[-1] if vals else default


def read_records(path):
    """The payloads of a TFRecord file; a length or payload checksum that does not match, or a record cut short, raises
    ValueError naming the offset."""
    with open(path, 'rb') as f:
        data = f.read()
    pos, out = 0, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("%s: truncated record header at byte %d" % (path, pos))
        head = data[pos:pos + 8]
        n, = struct.unpack('<Q', head)
        if struct.unpack_from('<I', data, pos + 8)[0] != _mask(crc32c(head)):
            raise ValueError("%s: length checksum mismatch at byte %d" % (path, pos))
        if pos + 12 + n + 4 > len(data):
            raise ValueError("%s: truncated record at byte %d (%d payload bytes announced)" % (path, pos, n))
        payload = data[pos + 12:pos + 12 + n]
        if struct.unpack_from('<I', data, pos + 12 + n)[0] != _mask(crc32c(payload)):
            raise ValueError("%s: payload checksum mismatch at byte %d" % (path, pos))
        out.append(payload)
        pos += 16 + n
    return out


def read_events(path):
    """[(step, {tag: float | (height, width, png bytes)})] of an event file's summary records, in file order; the first
    record must be the file-version event."""
    records = read_records(path)
    if not records or _one(list(_proto_fields(records[0])), 3) != FILE_VERSION:
        raise ValueError("%s: no %s record at the start" % (path, FILE_VERSION.decode()))
    out = []
    for payload in records[1:]:
        ev = list(_proto_fields(payload))
        summary = _one(ev, 5)
        if summary is None:
            continue
        step = _one(ev, 2, 0)
        step = step - (1 << 64) if step >= 1 << 63 else step
        vals = {}
        for fn, _, raw in _proto_fields(summary):
            if fn != 1:
                continue
            v = list(_proto_fields(raw))
            tag = _one(v, 1, b'').decode('utf-8')
            image = _one(v, 4)
            if image is not None:
                im = list(_proto_fields(image))
                vals[tag] = (_one(im, 1, 0), _one(im, 2, 0), _one(im, 4, b''))
            else:
                vals[tag] = struct.unpack('<f', struct.pack('<I', _one(v, 2, 0)))[0]
        out.append((step, vals))
    return out
