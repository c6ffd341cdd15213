#!/usr/bin/env python3
"""A TensorBoard event file assembled byte by byte from the format descriptions, WITHOUT importing unflow_amd (in particular
neither core/summary.py, whose writer and reader this fixture pins, nor core/tf_checkpoint.py's checksum):

  * TFRecord framing (tensorflow/core/lib/io/record_writer.h): uint64 length little endian, masked CRC-32C of those eight
    bytes, the payload, masked CRC-32C of the payload; masked = rotate-right-15 + 0xa282ead8; the CRC-32C table is built here
    from the reflected Castagnoli polynomial 0x82f63b78.
  * tensorflow/core/util/event.proto: Event {1: wall_time double, 2: step int64, 3: file_version string, 5: summary};
    tensorflow/core/framework/summary.proto: Summary {1: repeated Value {1: tag, 2: simple_value float, 4: image
    {1: height, 2: width, 3: colorspace, 4: encoded_image_string}}}.
  * the PNG of the image record: 8-bit RGB, filter 0 on every row, one IDAT of zlib level 6 (RFC 2083).

Three records, all at wall_time 1500000000.25: the file-version record, a two-scalar record at step 7 and a 2 x 3 image record
at step 300 (a two-byte varint).  Values are closed-form (SCALARS, image_pixels), so the test rebuilds what it hands the writer
without any file.

    python tests/golden/make_events_golden.py      # rewrites tests/golden/events_golden.tfevents
"""
import os
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "events_golden.tfevents")

WALL_TIME = 1500000000.25
SCALAR_STEP, IMAGE_STEP = 7, 300
SCALARS = [("loss/combined", 1.5), ("train/learning_rate", 0.0001)]
IMAGE_TAG = "train/augmented1/image/0"
IMAGE_H, IMAGE_W = 2, 3


def image_pixels():
    """[h][w][3] ints: pixel (y, x), channel c = (y * 3 + x) * 40 + c * 7."""
    return [[[(y * IMAGE_W + x) * 40 + c * 7 for c in range(3)] for x in range(IMAGE_W)] for y in range(IMAGE_H)]


TABLE = []
for n in range(256):
    r = n
    for _ in range(8):
        r = (r >> 1) ^ 0x82f63b78 if r & 1 else r >> 1
    TABLE.append(r)


def crc32c(data):
    c = 0xffffffff
    for b in data:
        c = TABLE[(c ^ b) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff


def masked(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xffffffff


def varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([v & 0x7f | 0x80])
        v >>= 7
    return out + bytes([v])


def f_varint(number, v):
    return varint(number << 3 | 0) + varint(v)


def f_bytes(number, payload):
    return varint(number << 3 | 2) + varint(len(payload)) + payload


def f_double(number, v):
    return varint(number << 3 | 1) + struct.pack("<d", v)


def f_float(number, v):
    return varint(number << 3 | 5) + struct.pack("<f", v)


def record(payload):
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", masked(head)) + payload + struct.pack("<I", masked(payload))


def png(pixels):
    h, w = len(pixels), len(pixels[0])
    raw = b"".join(b"\x00" + bytes(v for px in row for v in px) for row in pixels)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) +
            chunk(b"IEND", b""))


def build():
    version = f_double(1, WALL_TIME) + f_bytes(3, b"brain.Event:2")
    scalars = b"".join(f_bytes(1, f_bytes(1, tag.encode()) + f_float(2, v)) for tag, v in SCALARS)
    image = f_varint(1, IMAGE_H) + f_varint(2, IMAGE_W) + f_varint(3, 3) + f_bytes(4, png(image_pixels()))
    images = f_bytes(1, f_bytes(1, IMAGE_TAG.encode()) + f_bytes(4, image))
    return (record(version) + record(f_double(1, WALL_TIME) + f_varint(2, SCALAR_STEP) + f_bytes(5, scalars)) +
            record(f_double(1, WALL_TIME) + f_varint(2, IMAGE_STEP) + f_bytes(5, images)))


if __name__ == "__main__":
    with open(OUT, "wb") as f:
        f.write(build())
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
