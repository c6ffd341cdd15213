"""PNG decode on the device: the training input that keeps up with the step.

core/input.py::decode_png reconstructs Average / Paeth scanlines one pixel at a time in the interpreter (seconds per KITTI
frame).  Here the host only parses chunks and inflates (zlib releases the GIL, so a thread pool scales), and the GPU does the
rest (csrc/png_decode.hip):

  * unflow_png_unfilter   the five PNG row filters for a whole batch of images in one launch;
  * unflow_png_to_batch   read_png_image's channel rule, the crop and the normalisation -> float32 [n,H,W,3];
  * unflow_png_to_window  the same on a window with a signed origin: crop, central crop and zero padding in one rule;
  * unflow_png_to_flow_gt KITTI's 16-bit flow maps on such a window -> flow [n,H,W,2] and mask [n,H,W,1].

png_scanlines / decode_png_device are the building blocks; DevicePairBatches is the device twin of RawPairBatches (same pair
order, same crop draws, bit-identical batches) with the next batches in flight on a side stream while the step runs.
DeviceGTBatches is the twin of KITTIInput.input_train_gt (supervised fine-tuning) and DeviceEvalBatches of the evaluation
readers (KITTIInput.input_train_2012 / 2015, input_test_*): the same pipeline over a list of files per batch, each with a
role (frame or ground truth) and an origin.
.flo ground truth (Sintel, FlyingChairs, Middlebury) rides the same ring: a .flo body needs no inflate, so a worker reads it
straight into the pinned staging slot and csrc/flo_decode.hip cuts the window and derives the masks —

  * unflow_flo_to_flow_gt the Middlebury / Chairs rule: the file's floats and mask = both components < 1e9;
  * unflow_sintel_gt      Sintel's composition of a .flo file with its `invalid` and `occlusions` PNGs -> two maps.

The output side mirrors it (the end of this file): unflow_png_filter (csrc/png_encode.hip) chooses and applies the
PNG row filters on the device, DeviceFileWriter deflates and writes on a thread pool; encode_png_device is decode_png_device's
counterpart.  With deflate='device'  the entropy coder runs on the device too: unflow_deflate (csrc/deflate.hip)
turns the scanlines into finished zlib streams (deflate_device, DeviceDeflater), only compressed bytes come back, and a writer
thread forms the chunk CRCs and writes (kind 'png_z').

There is no host fallback: without the library's kernels these raise."""
import collections
import ctypes
import os
import queue
import struct
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from .input import FLO_TAG

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
FLO_HEADER_BYTES = 12    # tag, width, height
FLO_ALIGN = 16           # a .flo body's offset in the staging buffer (the kernels need 4; 16 keeps whole-pair and wider loads open)
MAX_WORKERS = 16         # a command's CPU budget on a GPU box; never sized from os.cpu_count()


def _check_variant(depth, ctype, interlace):
    if interlace or depth not in (8, 16) or ctype not in _CHANNELS:
        raise NotImplementedError("PNG variant (depth %d, colour type %d, interlace %d)" % (depth, ctype, interlace))


def _walk_chunks(data):
    """(IHDR fields or None, [IDAT bodies]) — decode_png's chunk walk."""
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("not a PNG")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, typ = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if typ == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif typ == b'IDAT':
            idat.append(body)
        elif typ == b'IEND':
            break
    if hdr is None:
        raise ValueError("PNG without an IHDR chunk")
    return hdr, idat


def png_scanlines(data):
    """PNG bytes -> (h, w, depth, ctype, raw): the inflated scanlines, h rows of 1 + w * bpp bytes with the filter byte first.
    Host only.  Raises what decode_png raises (bad signature, no IHDR, interlace / unsupported variants, truncated data), and
    ValueError for a filter byte above 4 — checked here, on a strided view of the filter column, so the kernel never sees one."""
    hdr, idat = _walk_chunks(data)
    w, h, depth, ctype, _, _, interlace = hdr
    _check_variant(depth, ctype, interlace)
    stride = w * _CHANNELS[ctype] * depth // 8
    raw = zlib.decompress(b''.join(idat))
    if len(raw) < h * (stride + 1):
        raise ValueError("truncated PNG image data")
    filters = np.frombuffer(raw, dtype=np.uint8, count=h * (stride + 1)).reshape(h, stride + 1)[:, 0]
    if h and int(filters.max()) > 4:
        raise ValueError("bad PNG filter %d" % int(filters.max()))
    return h, w, depth, ctype, raw


def png_header(path):
    """(h, w, depth, ctype) of a PNG file from its IHDR (the first chunk of every conforming file: 33 bytes are read; any other
    layout falls back to the chunk walk).  Unsupported variants raise as png_scanlines does."""
    with open(path, 'rb') as f:
        head = f.read(33)
        if head[:8] != PNG_SIGNATURE:
            raise ValueError("not a PNG")
        if len(head) == 33 and head[12:16] == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', head[16:29])
        else:
            hdr, _ = _walk_chunks(head + f.read())
    w, h, depth, ctype, _, _, interlace = hdr
    _check_variant(depth, ctype, interlace)
    return h, w, depth, ctype


def flo_header(path):
    """(h, w) of a .flo file: the tag 202021.25, a positive width and height, and a file of exactly 12 + 8 * w * h bytes;
    anything else raises ValueError naming the file."""
    with open(path, 'rb') as f:
        head = f.read(12)
        size = os.fstat(f.fileno()).st_size
    if len(head) < 12 or struct.unpack('<f', head[:4])[0] != FLO_TAG:
        raise ValueError("%s: not a .flo file (no 'PIEH' tag)" % path)
    w, h = struct.unpack('<ii', head[4:])
    if w <= 0 or h <= 0:
        raise ValueError("%s: a .flo file of %d x %d" % (path, h, w))
    if size != FLO_HEADER_BYTES + 8 * w * h:
        raise ValueError("%s: a %d x %d .flo file has %d bytes, this one %d" % (path, h, w, FLO_HEADER_BYTES + 8 * w * h, size))
    return h, w


def _bpp(depth, ctype):
    return _CHANNELS[ctype] * depth // 8


def _table_row(src, dst, h, w, depth, ctype, oy=0, ox=0):
    """One entry of the kernels' table (include/unflow_hip.h): src, dst, h, w, bpp, sample_bytes, oy, ox."""
    return (src, dst, h, w, _bpp(depth, ctype), depth // 8, oy, ox)


def _device(device):
    dev = torch.device('cuda' if device is None else device)
    if dev.type != 'cuda':
        raise ValueError("the PNG kernels need a GPU device, got %r" % (device,))
    return torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)


def _stream_ptr(stream):
    return ctypes.c_void_p(stream.cuda_stream)


def _unfilter(raw_dev, n_raw, dec_dev, n_dec, table_dev, n, stream):
    check(_lib.lib().unflow_png_unfilter(ptr(raw_dev), _lib.cl(n_raw), ptr(dec_dev), _lib.cl(n_dec), ptr(table_dev), n,
                                         _stream_ptr(stream)), "png_unfilter")


def _to_batch(dec_dev, n_dec, table_dev, n, H, W, mean, stddev, out, stream):
    mean_host = None if mean is None else (ctypes.c_float * 3)(*[float(m) for m in mean])
    check(_lib.lib().unflow_png_to_batch(ptr(dec_dev), _lib.cl(n_dec), ptr(table_dev), n, H, W, mean_host,
                                         _lib.cf(0.0 if stddev is None else stddev), ptr(out), _stream_ptr(stream)), "png_to_batch")


def decode_png_device(datas, device=None):
    """[PNG bytes, ...] -> [device tensor uint8 / uint16 [h, w, ch], ...], each equal to decode_png(data) exactly; one
    unflow_png_unfilter launch on the current stream serves the whole list."""
    return decode_scanlines_device([png_scanlines(data) for data in datas], device)


def decode_scanlines_device(scans, device=None):
    """decode_png_device behind the inflate: scans = [png_scanlines(data), ...] (which a thread pool can produce ahead)."""
    dev = _device(device)
    metas, raws, rows, src, dst = [], [], [], 0, 0
    for h, w, depth, ctype, raw in scans:
        n_in, n_out = h * (w * _bpp(depth, ctype) + 1), h * w * _bpp(depth, ctype)
        metas.append((h, w, depth, ctype, dst, n_out))
        raws.append(np.frombuffer(raw, dtype=np.uint8, count=n_in))
        rows.append(_table_row(src, dst, h, w, depth, ctype))
        src, dst = src + n_in, dst + n_out
    if not metas:
        return []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        raw_dev = torch.from_numpy(np.concatenate(raws)).to(dev)
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        dec = torch.empty(max(dst, 1), dtype=torch.uint8, device=dev)
        _unfilter(raw_dev, src, dec, dst, table, len(rows), stream)
        out = []
        for h, w, depth, ctype, off, n_out in metas:
            ch = _CHANNELS[ctype]
            a = dec[off:off + n_out]
            if depth == 16:      # big-endian samples -> uint16: swap each byte pair, then reinterpret
                a = a.view(h, w, ch, 2).flip(-1).contiguous().view(torch.uint16).view(h, w, ch)
            else:
                a = a.view(h, w, ch)
            out.append(a)
    return out


def _to_window(dec_dev, n_dec, table_dev, n, H, W, mean, stddev, out, stream):
    mean_host = None if mean is None else (ctypes.c_float * 3)(*[float(m) for m in mean])
    check(_lib.lib().unflow_png_to_window(ptr(dec_dev), _lib.cl(n_dec), ptr(table_dev), n, H, W, mean_host,
                                          _lib.cf(0.0 if stddev is None else stddev), ptr(out), _stream_ptr(stream)), "png_to_window")


def _to_flow_gt(dec_dev, n_dec, table_dev, n, H, W, flow, mask, stream):
    check(_lib.lib().unflow_png_to_flow_gt(ptr(dec_dev), _lib.cl(n_dec), ptr(table_dev), n, H, W, ptr(flow), ptr(mask),
                                           _stream_ptr(stream)), "png_to_flow_gt")


def _flo_to_flow_gt(raw_dev, n_raw, table_dev, n, H, W, flow, mask, stream):
    check(_lib.lib().unflow_flo_to_flow_gt(ptr(raw_dev), _lib.cl(n_raw), ptr(table_dev), n, H, W, ptr(flow), ptr(mask),
                                           _stream_ptr(stream)), "flo_to_flow_gt")


def _sintel_gt(raw_dev, n_raw, dec_dev, n_dec, table_dev, n, H, W, flow, mask, stream):
    check(_lib.lib().unflow_sintel_gt(ptr(raw_dev), _lib.cl(n_raw), ptr(dec_dev), _lib.cl(n_dec), ptr(table_dev), n, H, W,
                                      ptr(flow), ptr(mask), _stream_ptr(stream)), "sintel_gt")


def sintel_gt_device(triples, device=None):
    """Sintel's two-map ground truth of n pairs at the files' OWN size, composed on the device: triples = [(.flo, invalid PNG,
    occlusions PNG), ...], all of one size (h, w) -> (flow [2, n, h, w, 2], mask [2, n, h, w]) fp32 device tensors, map 0 =
    (flow, 1 - invalid), map 1 = (flow * (1 - occ), (1 - invalid) * (1 - occ)) — unflow_sintel_gt over the full-size window
    (origin 0, no crop, no padding), on the current stream, the bits of SintelInput.read_gt_full.  A file of another size, or a
    mask whose size differs from its .flo's, raises ValueError naming it.  (Synchronous host reads: the ground truth of a clip's
    replay, B files of each kind; evaluate_flo --sequence.)"""
    dev = _device(device)
    n = len(triples)
    if n == 0:
        raise ValueError("sintel_gt_device: no files")
    h, w = flo_header(triples[0][0])
    parts, rows, src, dst = [], [], 0, 0
    for col in range(3):
        for t in triples:
            path = t[col]
            if col == 0:
                if flo_header(path) != (h, w):
                    raise ValueError("%s is %d x %d, the clip's first flow file %s %d x %d"
                                     % ((path,) + flo_header(path) + (triples[0][0], h, w)))
                pad = -src % FLO_ALIGN
                parts.append(np.zeros(pad, np.uint8))
                src += pad
                with open(path, 'rb') as f:
                    body = np.frombuffer(f.read()[FLO_HEADER_BYTES:], dtype=np.uint8)
                rows.append((src, 0, h, w, 8, 4, 0, 0))
                parts.append(body)
                src += body.size
            else:
                with open(path, 'rb') as f:
                    mh, mw, depth, ctype, raw = png_scanlines(f.read())
                if (mh, mw) != (h, w):
                    raise ValueError("%s is %d x %d, its flow file %s %d x %d" % (path, mh, mw, t[0], h, w))
                n_in, n_out = mh * (mw * _bpp(depth, ctype) + 1), mh * mw * _bpp(depth, ctype)
                rows.append(_table_row(src, dst, mh, mw, depth, ctype))
                parts.append(np.frombuffer(raw, dtype=np.uint8, count=n_in))
                src, dst = src + n_in, dst + n_out
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        raw_dev = torch.from_numpy(np.concatenate(parts)).to(dev)
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        dec = torch.empty(max(dst, 1), dtype=torch.uint8, device=dev)
        _unfilter(raw_dev, src, dec, dst, table[n:], 2 * n, stream)
        flow = torch.empty(2, n, h, w, 2, dtype=torch.float32, device=dev)
        mask = torch.empty(2, n, h, w, dtype=torch.float32, device=dev)
        _sintel_gt(raw_dev, src, dec, dst, table, n, h, w, flow, mask, stream)
    return flow, mask


class PairPlanner:
    """The host-only half of DevicePairBatches: which files form the next batch and where they are cropped.  Walks the pair list
    as RawPairBatches does (in order, cyclically, `batch_size` examples per batch) and makes the same
    np.random.RandomState(seed) crop draws in the same order — the draw needs only the two frames' sizes, which are read from
    the files' IHDR (cached per path).  Called on the consumer's thread only, so the draws never depend on worker timing."""

    def __init__(self, pairs, batch_size, dims, needs_crop, seed):
        self.pairs, self.batch_size, self.dims = list(pairs), batch_size, tuple(dims)
        self.needs_crop = needs_crop
        self.pos = 0
        self.rng = np.random.RandomState(seed)
        self._headers = {}

    def header(self, path):
        if path not in self._headers:
            self._headers[path] = png_header(path)
        return self._headers[path]

    def next_batch(self):
        """[(file 1, file 2, header 1, header 2, oy, ox), ...] of the next batch."""
        h, w = self.dims
        out = []
        for _ in range(self.batch_size):
            fn1, fn2 = self.pairs[self.pos % len(self.pairs)]
            self.pos += 1
            m1, m2 = self.header(fn1), self.header(fn2)
            if self.needs_crop:
                lim_h, lim_w = min(m1[0], m2[0]), min(m1[1], m2[1])
                oy = int(self.rng.randint(0, lim_h - h + 1))
                ox = int(self.rng.randint(0, lim_w - w + 1))
            else:
                oy = ox = 0
                for fn, m in ((fn1, m1), (fn2, m2)):
                    if (m[0], m[1]) != (h, w):
                        raise ValueError("%s is %d x %d, not the %d x %d of dims (needs_crop=False)" % (fn, m[0], m[1], h, w))
            out.append((fn1, fn2, m1, m2, oy, ox))
        return out


def _inflate_into(path, meta, dst):
    """Worker: file -> inflated scanlines in `dst`, a numpy view of the pinned staging slot.  Returns the seconds it took."""
    t0 = time.perf_counter()
    with open(path, 'rb') as f:
        h, w, depth, ctype, raw = png_scanlines(f.read())
    if (h, w, depth, ctype) != tuple(meta):
        raise ValueError("%s changed on disk while it was being read" % path)
    dst[:] = np.frombuffer(raw, dtype=np.uint8, count=dst.size)
    return time.perf_counter() - t0


def _read_flo_into(path, meta, dst):
    """Worker: the body of a .flo file -> `dst`, a numpy view of the pinned staging slot (no intermediate copy, nothing to
    inflate).  Returns the seconds it took."""
    t0 = time.perf_counter()
    with open(path, 'rb') as f:
        head = f.read(FLO_HEADER_BYTES)
        ok = len(head) == FLO_HEADER_BYTES and struct.unpack('<fii', head) == (FLO_TAG, meta[1], meta[0])
        if not ok or f.readinto(memoryview(dst)) != dst.size or f.read(1):
            raise ValueError("%s changed on disk while it was being read" % path)
    return time.perf_counter() - t0


# A file's role: FRAME through unflow_png_to_batch / _to_window, GT (a KITTI flow PNG) through unflow_png_to_flow_gt, FLO (a .flo
# body, never unfiltered) through unflow_flo_to_flow_gt or, with its two MASK PNGs (Sintel's invalid and occlusions), through
# unflow_sintel_gt.  A batch's table holds its files in TABLE_ORDER, so the PNG rows are one run (one unfilter launch) and
# the rows of unflow_sintel_gt another.
FRAME, GT, FLO, MASK = 'frame', 'gt', 'flo', 'mask'
TABLE_ORDER = (FLO, MASK, FRAME, GT)
GT_KINDS = {'kitti': None, 'flo': (FLO,), 'sintel': (FLO, MASK, MASK)}       # roles of the ground-truth lists (kitti: GT each)
NO_GT = 'none'           # what gt_kind=None means without lists: a test split, frames only


def window_origin(n, size):
    """Where the window of resize_image_with_crop_or_pad(frame, size) starts in a frame axis of n pixels: its central-crop offset
    (n > size) or minus its zero-padding offset (n <= size; the odd extra goes to the bottom / right, as in TF).  The negative
    of core/inference.frame_origin."""
    return (n - size) // 2 if n > size else -((size - n) // 2)


def check_gt_header(path, meta):
    """A KITTI flow map is 16-bit RGB; anything else: ValueError naming the file."""
    if (meta[2], meta[3]) != (16, 2):
        raise ValueError("%s: not a 16-bit RGB flow map (depth %d, colour type %d)" % (path, meta[2], meta[3]))


def check_window_inside(path, meta, oy, ox, dims):
    """The (h, w) window at (oy, ox) must lie inside the file's frame (the crops of training); else ValueError naming the file."""
    h, w = dims
    if oy < 0 or ox < 0 or oy + h > meta[0] or ox + w > meta[1]:
        raise ValueError("%s is %d x %d: the %d x %d window at (%d, %d) leaves it" % (path, meta[0], meta[1], h, w, oy, ox))


TRAIN_GT_KINDS = ('kitti', 'flo', 'sintel')


class GTPlanner(PairPlanner):
    """The host-only half of DeviceGTBatches: walks an example list as the input_train_gt iterators do — from `shift`, in order,
    cyclically — and draws oy, then ox, per example from np.random.RandomState(seed) with limits from im1's header.  The window
    must lie inside every file of the example.
    gt_kind 'kitti' (default): KITTIInput.train_gt_files' (im1, im2, gt) list, the ground truth a 16-bit RGB PNG.
    gt_kind 'flo': (im1, im2, .flo) — ChairsInput.input_train_gt; 'sintel': (im1, im2, .flo, invalid PNG, occlusions PNG) —
    SintelInput.input_train_gt; a .flo file is checked by flo_header, a Sintel mask must have its .flo's size."""

    def __init__(self, files, batch_size, dims, seed, shift=0, gt_kind='kitti'):
        super().__init__(files, batch_size, dims, True, seed)
        self.pos = int(shift)
        if gt_kind not in TRAIN_GT_KINDS:
            raise ValueError("gt_kind must be one of %s, got %r" % (TRAIN_GT_KINDS, gt_kind))
        self.gt_kind = gt_kind
        self.gt_roles = GT_KINDS[gt_kind] or (GT,)
        self.n_maps = 2 if gt_kind == 'sintel' else 1
        for ex in self.pairs:
            if len(ex) != 2 + len(self.gt_roles):
                raise ValueError("gt_kind %r takes examples of %d files, got %d" % (gt_kind, 2 + len(self.gt_roles), len(ex)))

    def header(self, path, role=FRAME):
        if role != FLO:
            return super().header(path)
        if path not in self._headers:
            self._headers[path] = flo_header(path)
        return self._headers[path]

    def next_batch(self):
        """gt_kind 'kitti': [(im1, im2, gt, header 1, header 2, header gt, oy, ox), ...] of the next batch; the .flo kinds:
        [[file of im1, of im2, of every ground-truth file], ...] — (path, header, role, oy, ox) each, as EvalPlanner's."""
        if self.gt_kind != 'kitti':
            return self._next_batch_flo()
        h, w = self.dims
        out = []
        for _ in range(self.batch_size):
            fn1, fn2, fgt = self.pairs[self.pos % len(self.pairs)]
            self.pos += 1
            m1, m2, mg = self.header(fn1), self.header(fn2), self.header(fgt)
            check_gt_header(fgt, mg)
            check_window_inside(fn1, m1, 0, 0, self.dims)
            oy = int(self.rng.randint(0, m1[0] - h + 1))
            ox = int(self.rng.randint(0, m1[1] - w + 1))
            for fn, m in ((fn2, m2), (fgt, mg)):
                check_window_inside(fn, m, oy, ox, self.dims)
            out.append((fn1, fn2, fgt, m1, m2, mg, oy, ox))
        return out

    def _next_batch_flo(self):
        h, w = self.dims
        out = []
        for _ in range(self.batch_size):
            ex = self.pairs[self.pos % len(self.pairs)]
            self.pos += 1
            roles = (FRAME, FRAME) + tuple(self.gt_roles)
            metas = [self.header(fn, r) for fn, r in zip(ex, roles)]
            check_window_inside(ex[0], metas[0], 0, 0, self.dims)
            oy = int(self.rng.randint(0, metas[0][0] - h + 1))
            ox = int(self.rng.randint(0, metas[0][1] - w + 1))
            for fn, m in zip(ex[1:], metas[1:]):
                check_window_inside(fn, m, oy, ox, self.dims)
            for fn, m in zip(ex[3:], metas[3:]):
                if tuple(m[:2]) != tuple(metas[2][:2]):
                    raise ValueError("%s is %d x %d, its flow file %s %d x %d" % ((fn,) + tuple(m[:2]) + (ex[2],) + tuple(metas[2][:2])))
            out.append([(fn, m, r, oy, ox) for fn, m, r in zip(ex, metas, roles)])
        return out

    def files(self, examples):
        if self.gt_kind != 'kitti':
            return EvalPlanner.table_files(examples)
        return [(e[0], e[3], FRAME, e[6], e[7]) for e in examples] + [(e[1], e[4], FRAME, e[6], e[7]) for e in examples] + \
               [(e[2], e[5], GT, e[6], e[7]) for e in examples]


class EvalPlanner(PairPlanner):
    """The host-only half of DeviceEvalBatches: one pass over the pair list, `batch_size` examples per batch (a short last one),
    ground-truth files position by position as KITTIInput._input_train pairs them; every file gets the origin of
    resize_image_with_crop_or_pad for its OWN size (window_origin).
    gt_kind: None — no lists: a test split, frames only (with lists, for the callers of 7.7: 'kitti'); 'kitti' — every list holds
    KITTI flow PNGs, one map each; 'flo' — one list of .flo files, one map (Middlebury,
    FlyingChairs); 'sintel' — three lists (.flo, invalid PNGs, occlusion PNGs), two maps.  A .flo file is checked by flo_header,
    and a Sintel mask whose size differs from its .flo's raises ValueError naming it."""

    def __init__(self, pairs, batch_size, dims, gt_lists=(), gt_kind=None):
        super().__init__(pairs, batch_size, dims, False, 0)
        self.gt_lists = [list(g) for g in gt_lists]
        if gt_kind is None:
            gt_kind = 'kitti' if self.gt_lists else NO_GT
        elif gt_kind not in GT_KINDS:
            raise ValueError("gt_kind must be None or one of %s, got %r" % (sorted(GT_KINDS), gt_kind))
        self.gt_kind = gt_kind
        self.gt_roles = GT_KINDS.get(gt_kind) or (GT,) * len(self.gt_lists)
        if len(self.gt_lists) != len(self.gt_roles):
            raise ValueError("gt_kind %r takes %d ground-truth lists, got %d" % (gt_kind, len(self.gt_roles), len(self.gt_lists)))
        self.n_maps = {NO_GT: 0, 'kitti': len(self.gt_lists), 'flo': 1, 'sintel': 2}[gt_kind]
        for g in self.gt_lists:
            if len(g) != len(self.pairs):
                raise ValueError("%d ground-truth files for %d pairs" % (len(g), len(self.pairs)))

    def header(self, path, role=FRAME):
        if role != FLO:
            return super().header(path)
        if path not in self._headers:
            self._headers[path] = flo_header(path)
        return self._headers[path]

    def _file(self, path, role):
        m = self.header(path, role)
        if role == GT:
            check_gt_header(path, m)
        return (path, m, role, window_origin(m[0], self.dims[0]), window_origin(m[1], self.dims[1]))

    def next_batch(self):
        """[[file of im1, of im2, of every ground-truth list], ...] per example — (path, header, role, oy, ox) each — or None
        behind the last pair."""
        if self.pos >= len(self.pairs):
            return None
        out = []
        for k in range(self.pos, min(self.pos + self.batch_size, len(self.pairs))):
            fn1, fn2 = self.pairs[k]
            ex = [self._file(fn1, FRAME), self._file(fn2, FRAME)] + [self._file(g[k], r) for g, r in zip(self.gt_lists, self.gt_roles)]
            for f in ex[3:] if self.gt_kind == 'sintel' else ():
                if f[1][:2] != ex[2][1][:2]:
                    raise ValueError("%s is %d x %d, its flow file %s %d x %d" % ((f[0],) + f[1][:2] + (ex[2][0],) + ex[2][1][:2]))
            out.append(ex)
        self.pos += len(out)
        return out

    @staticmethod
    def files(examples):
        """Column-major: all first frames, all second frames, then each ground-truth list."""
        return [ex[c] for c in range(len(examples[0])) for ex in examples]

    @classmethod
    def table_files(cls, examples):
        """files() with the columns in TABLE_ORDER (stable): .flo files, Sintel's masks, the frames, KITTI maps."""
        cols = sorted(range(len(examples[0])), key=lambda c: TABLE_ORDER.index(examples[0][c][2]))
        return [ex[c] for c in cols for ex in examples]


class _Slot:
    """Staging and output of one batch in flight.  Every buffer is allocated (and grown) on the CONSUMER's thread, see
    _DeviceBatches._schedule."""

    def __init__(self, n_rows, n_frames, n_maps, H, W, dev):
        n = n_rows                                # table rows: the batch's files; n_maps ground-truth maps come out of them
        self.staging = None                       # pinned uint8: the batch's inflated streams, back to back
        self.table_host = torch.empty(n, _lib.PNG_DESC_FIELDS, dtype=torch.int64).pin_memory()
        self.table = torch.empty(n, _lib.PNG_DESC_FIELDS, dtype=torch.int64, device=dev)
        self.raw = self.dec = None                # device: inflated streams, decoded frames
        self.out = torch.empty(n_frames, H, W, 3, dtype=torch.float32, device=dev)
        self.flow = torch.empty(n_maps, H, W, 2, dtype=torch.float32, device=dev) if n_maps else None
        self.mask = torch.empty(n_maps, H, W, 1, dtype=torch.float32, device=dev) if n_maps else None
        self.uploaded = None                      # side-stream event: the pinned buffers have been read

    def reserve(self, n_raw, n_dec, dev):
        """Grow the buffers to the batch's sizes; True when something was allocated."""
        grown = False
        if self.staging is None or self.staging.numel() < n_raw:
            self.staging, grown = torch.empty(n_raw, dtype=torch.uint8).pin_memory(), True
        if self.raw is None or self.raw.numel() < n_raw:
            self.raw, grown = torch.empty(n_raw, dtype=torch.uint8, device=dev), True
        if self.dec is None or self.dec.numel() < n_dec:
            self.dec, grown = torch.empty(n_dec, dtype=torch.uint8, device=dev), True
        return grown


class _Job:
    """One batch: its slot, its files [(file, header, role, oy, ox)] in TABLE_ORDER (.flo files, Sintel's masks, the frames,
    KITTI maps), the kernels' table rows, each file's span in the staging buffer, the byte totals, the workers' futures and the
    event behind which the slot may be rewritten.  A .flo span starts at a multiple of FLO_ALIGN: the PNG streams around it have
    arbitrary lengths, and the kernels read its floats in place.  `plan` is what the planner returned (the iterator builds
    its result from it)."""

    def __init__(self, slot, files, plan=None):
        self.slot, self.files, self.plan = slot, files, plan
        roles = [f[2] for f in files]
        self.n_flo, self.n_mask, self.n_frames, self.n_gt = (roles.count(r) for r in TABLE_ORDER)
        assert roles == sorted(roles, key=TABLE_ORDER.index) and self.n_mask in (0, 2 * self.n_flo)
        self.rows, self.spans, src, dst = [], [], 0, 0
        for _, meta, role, oy, ox in self.files:
            if role == FLO:
                h, w = meta
                src = -(-src // FLO_ALIGN) * FLO_ALIGN
                n_in, n_out = 8 * h * w, 0
                self.rows.append((src, 0, h, w, 8, 4, oy, ox))
            else:
                h, w, depth, ctype = meta
                n_in, n_out = h * (w * _bpp(depth, ctype) + 1), h * w * _bpp(depth, ctype)
                self.rows.append(_table_row(src, dst, h, w, depth, ctype, oy, ox))
            self.spans.append((src, n_in))
            src, dst = src + n_in, dst + n_out
        self.n_raw, self.n_dec = src, dst
        self.free_event = self.futures = self.submitted = None
        self.done = threading.Event()
        self.error = self.ready = self.marks = None
        self.times = {}


_loader_streams = {}
_loader_streams_lock = threading.Lock()


def loader_stream(dev):
    """The side stream of the loaders on `dev`: ONE stream per device and process, created by the library
    (unflow_stream_create) and never destroyed.  torch.cuda.Stream() returns the streams of a pool of 32 round-robin, so a
    stream taken there can be the very stream on which the consumer's thread captures a hipGraph (torch.cuda.graph's default
    capture stream, the engine's capture stream) — the producer thread's uploads and kernels would then be enqueued INSIDE the
    capture, which ends with "capturing stream has unjoined work".  Whether that happens depends only on how many streams the
    process created before, so it must not be left to chance.  Loaders that run at the same time share the stream: their work
    is ordered by events as before, only serialised with each other."""
    with _loader_streams_lock:
        s = _loader_streams.get(dev.index)
        if s is None:
            handle = ctypes.c_void_p()
            with torch.cuda.device(dev):
                check(_lib.lib().unflow_stream_create(ctypes.byref(handle)), "stream_create")
            s = _loader_streams[dev.index] = torch.cuda.ExternalStream(handle.value, device=dev)
        return s


class _Pipeline:
    """What the producer thread owns: the worker pool, the side stream and the launches.  It does not refer to the iterator, so
    dropping the iterator stops it (_DeviceBatches.__del__).

    The producer thread only enqueues on the side stream (waits on events, asynchronous copies from pinned memory, the
    kernels, event records): it never allocates and never synchronises, so it may run while the consumer's thread captures a
    hipGraph of the training step (allocations and synchronising calls of ANY thread are errors during a capture).
    window: the frames go through unflow_png_to_window (signed origins, zero padding) instead of unflow_png_to_batch."""

    def __init__(self, dev, dims, mean, stddev, workers, timing, window=False):
        self.dev, self.dims, self.mean, self.stddev, self.timing, self.window = dev, dims, mean, stddev, timing, window
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)), thread_name_prefix="png-inflate")
        self.side = loader_stream(dev)
        self.jobs = queue.Queue()
        self.closed = False
        self.thread = threading.Thread(target=self._run, name="png-producer", daemon=True)
        self.thread.start()

    def _run(self):
        torch.cuda.set_device(self.dev)
        while True:
            job = self.jobs.get()
            if job is None:
                return
            try:
                if not self.closed:
                    self._produce(job)
            except BaseException as e:      # handed to the consumer's next()
                job.error = e
            job.done.set()

    def _produce(self, job):
        slot, (H, W) = job.slot, self.dims
        n, nf = len(job.rows), job.n_frames
        f0 = job.n_flo + job.n_mask                            # the first frame's row; the PNG rows start behind the .flo rows
        slot.table_host[:n].copy_(torch.tensor(job.rows, dtype=torch.int64))
        errors = [f.exception() for f in job.futures]         # waits for every worker: none is left writing into the slot
        job.times['inflate_s'] = time.perf_counter() - job.submitted          # submit -> last frame staged
        for e in errors:
            if e is not None:
                raise e
        job.times['worker_s'] = sum(f.result() for f in job.futures)          # thread-seconds of the batch's frames
        marks = [torch.cuda.Event(enable_timing=self.timing) for _ in range(5)]
        with torch.cuda.stream(self.side):
            self.side.wait_event(job.free_event)               # the consumer has passed the batch this slot held
            marks[0].record(self.side)
            slot.raw[:job.n_raw].copy_(slot.staging[:job.n_raw], non_blocking=True)
            slot.table[:n].copy_(slot.table_host[:n], non_blocking=True)
            marks[1].record(self.side)
            _unfilter(slot.raw, job.n_raw, slot.dec, job.n_dec, slot.table[job.n_flo:], n - job.n_flo, self.side)
            marks[2].record(self.side)
            to_frames = _to_window if self.window else _to_batch
            to_frames(slot.dec, job.n_dec, slot.table[f0:], nf, H, W, self.mean, self.stddev, slot.out, self.side)
            marks[3].record(self.side)
            if job.n_gt:
                _to_flow_gt(slot.dec, job.n_dec, slot.table[f0 + nf:], job.n_gt, H, W, slot.flow, slot.mask, self.side)
            elif job.n_mask:
                _sintel_gt(slot.raw, job.n_raw, slot.dec, job.n_dec, slot.table, job.n_flo, H, W, slot.flow, slot.mask, self.side)
            elif job.n_flo:
                _flo_to_flow_gt(slot.raw, job.n_raw, slot.table, job.n_flo, H, W, slot.flow, slot.mask, self.side)
            marks[4].record(self.side)
        slot.uploaded, job.marks, job.ready = marks[1], marks, marks[4]

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.jobs.put(None)
        if threading.current_thread() is not self.thread:
            self.thread.join()
        self.pool.shutdown(wait=True, cancel_futures=True)
        self.side.synchronize()


class _DeviceBatches:
    """The loader ring that the three iterators share.  A subclass plans a batch on the consumer's thread (_plan: the files of
    the next batch with their roles and origins, or None when a finite input is exhausted) and names what next() returns
    (_result: views of the slot's tensors).

    Up to `workers` (at most 16) threads read the files and inflate them into pinned staging; the upload and the kernels run
    on one side stream; `prefetch` batches are in flight while the consumer works.  next() makes the current stream wait for the
    batch's event, so kernels launched on the current stream afterwards (the engine's) see the batch.  The tensors belong
    to a ring of prefetch + 1 slots: they stay valid for work enqueued on the current stream before the NEXT next() call (which is
    what Trainer.train does: set_input copies them into the engine's buffers); copy them to keep them longer.  A slot is
    rewritten only behind an event recorded on the current stream at that later next().  next() also plans the batch that
    takes the freed slot, grows the slot's buffers if the batch needs it, waits until the slot's last upload has left the pinned
    staging and hands the batch's files to the workers — everything that allocates or synchronises happens on the consumer's
    thread, between steps.  close() (and garbage collection) stops the threads.  Threads only: no other process opens the GPU."""

    def __init__(self, n_rows, n_frames, n_maps, dims, mean, stddev, device, workers, prefetch, timing, window):
        if prefetch < 1:
            raise ValueError("prefetch must be at least 1")
        self.device = _device(device)
        self.dims, self.prefetch = tuple(dims), prefetch
        _lib.lib()                                  # a missing library is an error here, not in the producer thread
        self._pipe = _Pipeline(self.device, self.dims, mean, stddev, workers, bool(timing), window)
        self._inflight = collections.deque()
        self._held = None                           # the slot whose tensors the consumer holds
        self._exhausted = False                     # a finite input: the planner has no further batch
        self.stage_times = collections.deque(maxlen=64)     # timing=True: per-batch dicts, filled by next()
        self._timed = collections.deque()
        try:
            with torch.cuda.device(self.device):
                slots = [_Slot(n_rows, n_frames, n_maps, self.dims[0], self.dims[1], self.device) for _ in range(prefetch + 1)]
            # (slot, event on the current stream behind which the side stream may write it)
            self._free = collections.deque((s, self._mark()) for s in slots)
            for _ in range(prefetch):
                self._schedule()
        except BaseException:
            self._pipe.close()
            raise

    def _plan(self):
        raise NotImplementedError

    def _result(self, job):
        raise NotImplementedError

    def _mark(self):
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(self.device))
        return e

    def _schedule(self):
        if self._exhausted:
            return False
        planned = self._plan()
        if planned is None:
            self._exhausted = True
            return False
        slot, free_event = self._free[0]
        job = _Job(slot, *planned)
        self._free.popleft()
        if slot.uploaded is not None:
            slot.uploaded.synchronize()             # the slot's previous batch has left the pinned buffers: workers may write them
        with torch.cuda.device(self.device):
            if slot.reserve(job.n_raw, job.n_dec, self.device):
                free_event = self._mark()           # memory new to the side stream: behind whatever the current stream did with it
        job.free_event = free_event
        # the workers start now, so the frames of every batch in flight share the pool; the producer thread takes the batches in order
        stage = slot.staging.numpy()
        job.submitted = time.perf_counter()
        job.futures = [self._pipe.pool.submit(_read_flo_into if f[2] == FLO else _inflate_into, f[0], f[1], stage[o:o + n])
                       for f, (o, n) in zip(job.files, job.spans)]
        self._inflight.append(job)
        self._pipe.jobs.put(job)
        return True

    def __iter__(self):
        return self

    def __next__(self):
        if self._pipe.closed and not (self._exhausted and not self._inflight):
            raise RuntimeError("%s is closed" % type(self).__name__)
        if not self._inflight:                      # a finite input, fully handed out
            self.close()
            raise StopIteration
        job = self._inflight.popleft()
        job.done.wait()
        if job.error is not None:
            self.close()
            raise job.error
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(job.ready)
        if self._held is not None:
            self._free.append((self._held, self._mark()))       # behind the mark: everything the consumer did with that batch
        self._held = job.slot
        try:
            while self._free and len(self._inflight) < self.prefetch and self._schedule():
                pass
        except BaseException:
            self.close()
            raise
        if self._pipe.timing:
            self._collect(job)
        return self._result(job)

    def _collect(self, job):
        self._timed.append(job)
        while self._timed and self._timed[0].marks[4].query():
            j = self._timed.popleft()
            m = j.marks
            t = dict(j.times, upload_ms=m[0].elapsed_time(m[1]), unfilter_ms=m[1].elapsed_time(m[2]),
                     to_batch_ms=m[2].elapsed_time(m[3]))
            if j.n_gt or j.n_flo:
                t['flow_gt_ms'] = m[3].elapsed_time(m[4])
            self.stage_times.append(t)

    def close(self):
        self._pipe.close()

    def __del__(self):
        try:
            self._pipe.close()
        except Exception:
            pass


def _norm(normalize, mean, stddev):
    return (np.asarray(mean, dtype=np.float32), np.float32(stddev)) if normalize else (None, None)


class DevicePairBatches(_DeviceBatches):
    """The device twin of RawPairBatches: an iterator of (image_1, image_2), two float32 DEVICE tensors [B,H,W,3] that equal what
    RawPairBatches.__next__ returns for the same files and seed, bit for bit (pair order and crop draws: PairPlanner; the ring,
    the threads and the lifetime of the tensors: _DeviceBatches)."""

    def __init__(self, pairs, batch_size, dims, needs_crop, normalize, mean, stddev, seed, device=None, workers=8, prefetch=2,
                 timing=False):
        self.planner = PairPlanner(pairs, batch_size, dims, needs_crop, seed)
        self.batch_size = batch_size
        mean, stddev = _norm(normalize, mean, stddev)
        super().__init__(2 * batch_size, 2 * batch_size, 0, dims, mean, stddev, device, workers, prefetch, timing, window=False)

    def _plan(self):
        examples = self.planner.next_batch()
        files = [(fn1, m1, FRAME, oy, ox) for fn1, _, m1, _, oy, ox in examples] + \
                [(fn2, m2, FRAME, oy, ox) for _, fn2, _, m2, oy, ox in examples]
        return files, examples

    def _result(self, job):
        B = self.batch_size
        return job.slot.out[:B], job.slot.out[B:]


class DeviceGTBatches(_DeviceBatches):
    """The device twin of the input_train_gt iterators (KITTIInput, and with gt_kind 'flo' / 'sintel' ChairsInput / SintelInput):
    an endless iterator of (im1, im2, flow_gt, mask_gt), float32 DEVICE tensors
    [B,h,w,3] x 2, [B,h,w,2], [B,h,w,1], bit-identical to the host iterator for the same file list, seed and shift (GTPlanner).
    A window that leaves one of an example's files, or a KITTI ground-truth file that is not 16-bit RGB, raises ValueError
    naming the file (from the constructor or from next(), whichever plans the batch).  gt_map (gt_kind 'sintel'): 0 = the
    occluded map (flow, 1 - invalid), 1 = the non-occluded one (unflow_sintel_gt composes both)."""

    def __init__(self, files, batch_size, dims, normalize, mean, stddev, seed=0, shift=0, device=None, workers=8, prefetch=2,
                 timing=False, gt_kind='kitti', gt_map=0):
        self.planner = GTPlanner(files, batch_size, dims, seed, shift, gt_kind)
        if not 0 <= int(gt_map) < self.planner.n_maps:
            raise ValueError("gt_map %r: gt_kind %r has %d map(s)" % (gt_map, gt_kind, self.planner.n_maps))
        self.batch_size, self.gt_map = batch_size, int(gt_map)
        mean, stddev = _norm(normalize, mean, stddev)
        super().__init__((2 + len(self.planner.gt_roles)) * batch_size, 2 * batch_size, self.planner.n_maps * batch_size, dims, mean,
                         stddev, device, workers, prefetch, timing, window=True)

    def _plan(self):
        examples = self.planner.next_batch()
        return self.planner.files(examples), examples

    def _result(self, job):
        B, s, g = self.batch_size, job.slot, self.gt_map
        return s.out[:B], s.out[B:], s.flow[g * B:(g + 1) * B], s.mask[g * B:(g + 1) * B]


class DeviceEvalBatches(_DeviceBatches):
    """The device twin of KITTIInput._input_train (gt_lists = the flow_occ and flow_noc files) and Input.input_test (no ground
    truth): one pass, a short last batch, the host iterator's tuples — im1, im2 [n,Hs,Ws,3] on the device, input_shape [n,3]
    int32 on the HOST (from im1's IHDR) and per ground-truth list flow [n,Hs,Ws,2], mask [n,Hs,Ws,1] — every tensor equal to the
    host's bit for bit (crop or zero padding per file as resize_image_with_crop_or_pad, normalisation after the padding).
    gt_kind (EvalPlanner): None with no lists is a test split (3-tuples), 'flo' is the twin of ChairsInput.input_test /
    MiddleburyInput.input_train (gt_lists = the .flo files; 5-tuples), 'sintel' of SintelInput.input_train_* (gt_lists = the .flo, invalid and occlusion files; 7-tuples: flow_occ,
    mask_occ, flow_noc, mask_noc)."""

    def __init__(self, pairs, batch_size, dims, normalize, mean, stddev, gt_lists=(), device=None, workers=8, prefetch=2,
                 timing=False, gt_kind=None):
        self.planner = EvalPlanner(pairs, batch_size, dims, gt_lists, gt_kind)
        self.batch_size = batch_size
        mean, stddev = _norm(normalize, mean, stddev)
        super().__init__((2 + len(self.planner.gt_lists)) * batch_size, 2 * batch_size, self.planner.n_maps * batch_size, dims, mean,
                         stddev, device, workers, prefetch, timing, window=True)

    def _plan(self):
        examples = self.planner.next_batch()
        return None if examples is None else (self.planner.table_files(examples), examples)

    def _result(self, job):
        n, s = len(job.plan), job.slot
        shapes = np.asarray([(ex[0][1][0], ex[0][1][1], 3) for ex in job.plan], dtype=np.int32)
        out = [s.out[:n], s.out[n:2 * n], shapes]
        for g in range(self.planner.n_maps):
            out += [s.flow[g * n:(g + 1) * n], s.mask[g * n:(g + 1) * n]]
        return tuple(out)


# ------------------------------------------------------------------------------------------------------------ PNG encode
# The output side of the same split (csrc/png_encode.hip): the GPU chooses and applies the row filters
# (unflow_png_filter: finished scanlines, filter byte included, for a list of images in one launch), the host deflates them, on a
# pool — zlib.compress and zlib.crc32 release the GIL — and writes the files.
_CTYPE_OF_CHANNELS = {1: 0, 2: 4, 3: 2, 4: 6}
PNG_LEVELS = range(0, 10)


def check_level(level):
    if isinstance(level, bool) or int(level) != level or int(level) not in PNG_LEVELS:
        raise ValueError("a deflate level is an integer in [0, 9], got %r" % (level,))
    return int(level)


def _chunk(typ, body):
    return struct.pack('>I', len(body)) + typ + body + struct.pack('>I', zlib.crc32(body, zlib.crc32(typ)) & 0xffffffff)


def assemble_png(h, w, depth, ctype, scanlines, level=6, compress=zlib.compress):
    """Finished scanlines (h rows of 1 + w * bpp bytes, the filter byte first) -> PNG file bytes: IHDR, one IDAT, IEND.  Host
    only; `scanlines` is anything with the buffer protocol."""
    _check_variant(depth, ctype, 0)
    scan = memoryview(scanlines).cast('B')
    if len(scan) != h * (1 + w * _bpp(depth, ctype)):
        raise ValueError("%d bytes of scanlines for a %d x %d image of %d bytes per pixel" % (len(scan), h, w, _bpp(depth, ctype)))
    return b''.join((PNG_SIGNATURE, _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, 0)),
                     _chunk(b'IDAT', compress(scan, level)), _chunk(b'IEND', b'')))


class PngSurface:
    """Where unflow_png_filter reads images from (unflow_png_surface of include/unflow_hip.h): `images` allocations of (H, W)
    pixels of `channels` samples in the device tensor `tensor`, strides in elements; kind = _lib.PNG_U8 / PNG_U8X255 / PNG_U16BE."""

    def __init__(self, tensor, images, H, W, channels, kind, image_stride=None, row_stride=None):
        self.tensor, self.images, self.H, self.W, self.channels, self.kind = tensor, int(images), int(H), int(W), int(channels), kind
        self.row_stride = self.W * self.channels if row_stride is None else int(row_stride)
        self.image_stride = self.H * self.row_stride if image_stride is None else int(image_stride)
        self.depth = 16 if kind == _lib.PNG_U16BE else 8
        self.bpp = self.channels * self.depth // 8
        self.ctype = _CTYPE_OF_CHANNELS[self.channels]
        want = 2 if kind == _lib.PNG_U16BE else 1
        if tensor.element_size() != want or not tensor.is_cuda:
            raise ValueError("a PNG surface of kind %d takes a device tensor of %d-byte elements" % (kind, want))
        last = (self.images - 1) * self.image_stride + (self.H - 1) * self.row_stride + self.W * self.channels
        if self.row_stride < self.W * self.channels or last > tensor.numel() or not tensor.is_contiguous() or \
                self.image_stride < (self.H - 1) * self.row_stride + self.W * self.channels:
            raise ValueError("a PNG surface of %d x (%d, %d, %d) with strides (%d, %d) leaves its tensor of %d elements"
                             % (self.images, self.H, self.W, self.channels, self.image_stride, self.row_stride, tensor.numel()))

    def c(self):
        return _lib.PngSurface(self.tensor.data_ptr(), self.image_stride, self.row_stride, self.images, self.H, self.W,
                               self.channels, self.kind)


def plan_scanlines(surfaces, entries, first=0):
    """Host packing of unflow_png_filter's table.  entries: [(surface index, image, h, w), ...] -> (rows int64 [n][8], spans
    [(offset, bytes, h, w, depth, ctype)], end offset, max h, max row bytes): image k's scanlines lie at [offset, offset +
    bytes) of the output buffer, back to back from `first`.  Everything the kernel would skip raises ValueError here."""
    rows = np.zeros((len(entries), _lib.PNG_FILTER_FIELDS), dtype=np.int64)
    spans, off, max_h, max_row = [], int(first), 1, 1
    for k, (si, image, h, w) in enumerate(entries):
        if not 0 <= si < len(surfaces):
            raise ValueError("entry %d names surface %d of %d" % (k, si, len(surfaces)))
        s = surfaces[si]
        if not (0 <= image < s.images and 1 <= h <= s.H and 1 <= w <= s.W):
            raise ValueError("entry %d: image %d of %d x %d leaves its surface (%d images of %d x %d)"
                             % (k, image, h, w, s.images, s.H, s.W))
        if w * s.bpp > _lib.PNG_FILTER_MAX_ROW_BYTES:
            raise ValueError("entry %d: a row of %d bytes (the filter kernel takes %d)" % (k, w * s.bpp, _lib.PNG_FILTER_MAX_ROW_BYTES))
        n = h * (1 + w * s.bpp)
        rows[k, :5] = (si, image, h, w, off)
        spans.append((off, n, h, w, s.depth, s.ctype))
        off, max_h, max_row = off + n, max(max_h, h), max(max_row, w * s.bpp)
    return rows, spans, off, max_h, max_row


def filter_scanlines(surfaces, table_dev, n, max_h, max_row, out_dev, stream):
    """One unflow_png_filter launch on `stream`: the n entries of the device table -> scanlines in out_dev."""
    if len(surfaces) > _lib.PNG_SURFACES_MAX:
        raise ValueError("%d surfaces in one launch (at most %d)" % (len(surfaces), _lib.PNG_SURFACES_MAX))
    arr = (_lib.PngSurface * len(surfaces))(*[s.c() for s in surfaces])
    check(_lib.lib().unflow_png_filter(arr, len(surfaces), ptr(table_dev), int(n), int(max_h), int(max_row), ptr(out_dev),
                                       _lib.cl(out_dev.numel()), _stream_ptr(stream)), "png_filter")


def _surface_of(t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("encode_png_device takes device tensors")
    if t.ndim == 2 and t.dtype == torch.uint8:
        ch, kind = 1, _lib.PNG_U8
    elif t.ndim == 3 and t.shape[2] == 3 and t.dtype == torch.uint8:
        ch, kind = 3, _lib.PNG_U8
    elif t.ndim == 3 and t.shape[2] == 3 and t.dtype in (torch.int16, torch.uint16):
        ch, kind = 3, _lib.PNG_U16BE
    else:
        raise ValueError("encode_png_device: uint8 [h,w], uint8 [h,w,3] or uint16 / int16 [h,w,3], got %s %s" % (t.dtype, tuple(t.shape)))
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("encode_png_device: an empty image %s" % (tuple(t.shape),))
    t = t.contiguous()
    return PngSurface(t, 1, t.shape[0], t.shape[1], ch, kind)


def scanlines_device(images):
    """[device tensor, ...] -> (uint8 device tensor of all scanlines, spans as plan_scanlines'): the filter half of
    encode_png_device.  One launch serves up to 16 images (the kernel's surface list); a longer list takes one launch per 16."""
    surfaces = [_surface_of(t) for t in images]
    if not surfaces:
        return None, []
    dev = surfaces[0].tensor.device
    rows, spans, total, _, _ = plan_scanlines(surfaces, [(k, 0, s.H, s.W) for k, s in enumerate(surfaces)])
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        step = _lib.PNG_SURFACES_MAX
        for k0 in range(0, len(surfaces), step):
            part = surfaces[k0:k0 + step]
            r = rows[k0:k0 + step].copy()
            r[:, 0] -= k0
            table = torch.from_numpy(r).to(dev)
            filter_scanlines(part, table, len(part), max(s.H for s in part), max(s.W * s.bpp for s in part), out, stream)
    return out, spans


def assemble_png_z(h, w, depth, ctype, zstream):
    """A finished zlib stream of an image's scanlines (deflate_device's) -> PNG file bytes: IHDR, one IDAT, IEND.  Host only:
    the two chunk CRCs are all the work left."""
    _check_variant(depth, ctype, 0)
    return b''.join((PNG_SIGNATURE, _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, 0)),
                     _chunk(b'IDAT', bytes(zstream)), _chunk(b'IEND', b'')))


DEFLATE_MODES = ('host', 'device')


def check_deflate_mode(deflate, workers=None):
    """'host' or 'device'; the device coder feeds the writer pool, so it needs workers >= 1 (where `workers` is given)."""
    if deflate not in DEFLATE_MODES:
        raise ValueError("deflate must be one of %s, got %r" % (DEFLATE_MODES, deflate))
    if deflate == 'device' and workers is not None and int(workers) < 1:
        raise ValueError("deflate='device' writes through the pool of the device encode path: it needs workers >= 1")
    return deflate == 'device'


def check_chunk_bytes(chunk_bytes):
    """None -> the default; otherwise an integer in [1, 65535] (one stored block must cover a chunk)."""
    if chunk_bytes is None:
        return _lib.DEFLATE_CHUNK_DEFAULT
    if isinstance(chunk_bytes, bool) or int(chunk_bytes) != chunk_bytes or not 1 <= int(chunk_bytes) <= _lib.DEFLATE_CHUNK_MAX:
        raise ValueError("chunk_bytes is an integer in [1, %d], got %r" % (_lib.DEFLATE_CHUNK_MAX, chunk_bytes))
    return int(chunk_bytes)


def deflate_slot_bytes(chunk):
    """Scratch bytes per chunk (unflow_deflate_slot_bytes): the segment bound rounded to 16, and 16."""
    return ((chunk + 5 + 15) & ~15) + 16


class DeflatePlan:
    """Host packing of unflow_deflate's table for streams [(offset, bytes, ...), ...] of one input buffer: rows int64 [n][8],
    places [(dst, cap)], and the sizes of the buffers the launch needs (out_bytes, scratch_bytes, meta_chunks, max_chunks)."""

    def __init__(self, spans, chunk_bytes=None):
        self.chunk = check_chunk_bytes(chunk_bytes)
        self.n = len(spans)
        self.rows = np.zeros((self.n, _lib.DEFLATE_FIELDS), dtype=np.int64)
        self.places, dst, scratch, meta, self.max_chunks = [], 0, 0, 0, 1
        slot = deflate_slot_bytes(self.chunk)
        for k, sp in enumerate(spans):
            off, nb = int(sp[0]), int(sp[1])
            chunks = max(1, -(-nb // self.chunk))
            cap = 2 + nb + 5 * chunks + 4
            self.rows[k, :6] = (off, nb, dst, cap, scratch, meta)
            self.places.append((dst, cap))
            dst, scratch, meta = dst + (-(-cap // 16)) * 16, scratch + chunks * slot, meta + chunks
            self.max_chunks = max(self.max_chunks, chunks)
        self.out_bytes, self.scratch_bytes, self.meta_chunks = dst, scratch, meta


def check_deflate_table(rows, chunk, in_bytes, out_bytes, scratch_bytes, meta_chunks):
    """Everything unflow_deflate would skip raises ValueError here, before any launch: a stream, an output range, a scratch range
    or a meta range that leaves its buffer, a cap below the stream bound, output ranges that overlap."""
    slot, taken = deflate_slot_bytes(chunk), []
    for k, (src, nb, dst, cap, scratch, meta) in enumerate(np.asarray(rows)[:, :6].tolist()):
        if nb < 1 or src < 0 or src + nb > in_bytes:
            raise ValueError("deflate entry %d: bytes [%d, %d) leave the input buffer of %d bytes" % (k, src, src + nb, in_bytes))
        chunks = -(-nb // chunk)
        if cap < 2 + nb + 5 * chunks + 4:
            raise ValueError("deflate entry %d: %d bytes of output for a stream whose bound is %d" % (k, cap, 2 + nb + 5 * chunks + 4))
        if dst < 0 or dst + cap > out_bytes:
            raise ValueError("deflate entry %d: output [%d, %d) leaves the buffer of %d bytes" % (k, dst, dst + cap, out_bytes))
        if scratch < 0 or scratch % 16 or scratch + chunks * slot > scratch_bytes:
            raise ValueError("deflate entry %d: scratch [%d, %d) leaves the buffer of %d bytes (or is not a multiple of 16)"
                             % (k, scratch, scratch + chunks * slot, scratch_bytes))
        if meta < 0 or meta + chunks > meta_chunks:
            raise ValueError("deflate entry %d: meta entries [%d, %d) of %d" % (k, meta, meta + chunks, meta_chunks))
        taken.append((dst, dst + cap))
    taken.sort()
    for (_, e0), (s1, _) in zip(taken, taken[1:]):
        if s1 < e0:
            raise ValueError("deflate: output ranges overlap at byte %d" % s1)


def deflate_launch(in_dev, rows, table_dev, max_chunks, chunk, scratch_dev, meta_dev, out_dev, sizes_dev, stream):
    """One unflow_deflate call on `stream` for the table `rows` (host; validated here) whose copy is table_dev (device)."""
    chunk = check_chunk_bytes(chunk)
    n = len(rows)
    if n < 1 or table_dev.numel() < n * _lib.DEFLATE_FIELDS or sizes_dev.numel() < n:
        raise ValueError("deflate: %d entries for a table of %d and %d sizes" % (n, table_dev.numel() // _lib.DEFLATE_FIELDS,
                                                                              sizes_dev.numel()))
    check_deflate_table(rows, chunk, in_dev.numel(), out_dev.numel(), scratch_dev.numel(), meta_dev.numel() // _lib.DEFLATE_META)
    check(_lib.lib().unflow_deflate(ptr(in_dev), _lib.cl(in_dev.numel()), ptr(table_dev), n, int(max_chunks), chunk,
                                    ptr(scratch_dev), _lib.cl(scratch_dev.numel()), ptr(meta_dev),
                                    _lib.cl(meta_dev.numel() // _lib.DEFLATE_META), ptr(out_dev), _lib.cl(out_dev.numel()),
                                    ptr(sizes_dev), _stream_ptr(stream)), "deflate")


class DeviceDeflater:
    """The buffers of unflow_deflate for up to max_streams streams of max_bytes bytes in all, allocated once (the estimator keeps
    one beside its scanline buffer): the device table, scratch slots, chunk meta, the output and the sizes, and pinned twins of
    the table and the sizes.  launch() enqueues the table upload, the two kernels and the copy of the sizes; once the caller
    has synchronised behind it, fetch() enqueues one copy per stream of exactly its compressed bytes."""

    def __init__(self, dev, max_streams, max_bytes, chunk_bytes=None):
        self.chunk = check_chunk_bytes(chunk_bytes)
        self.dev, self.max_streams = dev, int(max_streams)
        chunks = int(max_bytes) // self.chunk + self.max_streams
        self.host_bytes = int(max_bytes) + 5 * chunks + 6 * self.max_streams                 # the most fetch() packs
        with torch.cuda.device(dev):
            self.table = torch.zeros(self.max_streams, _lib.DEFLATE_FIELDS, dtype=torch.int64, device=dev)
            self.sizes = torch.zeros(self.max_streams, dtype=torch.int64, device=dev)
            self.scratch = torch.empty(chunks * deflate_slot_bytes(self.chunk), dtype=torch.uint8, device=dev)
            self.meta = torch.zeros(chunks * _lib.DEFLATE_META, dtype=torch.int32, device=dev)
            self.out = torch.empty(self.host_bytes + 16 * self.max_streams, dtype=torch.uint8, device=dev)
        self.table_host = torch.zeros(self.max_streams, _lib.DEFLATE_FIELDS, dtype=torch.int64, pin_memory=True)
        self.sizes_host = torch.zeros(self.max_streams, dtype=torch.int64, pin_memory=True)

    def launch(self, in_dev, spans, stream):
        plan = DeflatePlan(spans, self.chunk)
        if plan.n > self.max_streams:
            raise ValueError("deflate: %d streams in one launch (this deflater takes %d)" % (plan.n, self.max_streams))
        self.table_host.numpy()[:plan.n] = plan.rows
        with torch.cuda.stream(stream):
            self.table[:plan.n].copy_(self.table_host[:plan.n], non_blocking=True)
            deflate_launch(in_dev, plan.rows, self.table, plan.max_chunks, self.chunk, self.scratch, self.meta, self.out,
                           self.sizes, stream)
            self.sizes_host[:plan.n].copy_(self.sizes[:plan.n], non_blocking=True)
        return plan

    def fetch(self, plan, host, stream):
        """Behind a synchronisation on launch(): the streams' bytes -> `host` (a pinned uint8 tensor) back to back; returns
        [(offset, bytes)] in it.  The copies are enqueued on `stream`."""
        sizes = self.sizes_host.numpy()[:plan.n].tolist()
        out, pos = [], 0
        with torch.cuda.stream(stream):
            for (dst, cap), size in zip(plan.places, sizes):
                if not 8 <= size <= cap:
                    raise RuntimeError("unflow_deflate reported a stream of %d bytes (bound %d)" % (size, cap))
                host[pos:pos + size].copy_(self.out[dst:dst + size], non_blocking=True)
                out.append((pos, size))
                pos += size
        return out


def deflate_device(scan_dev, spans, stream=None, chunk_bytes=None):
    """Streams [(offset, bytes, ...), ...] of the device byte buffer scan_dev (scanlines_device's pair) -> [zlib stream bytes]:
    one unflow_deflate launch pair on `stream` (default: the current one); only the compressed bytes are copied back.
    chunk_bytes: the bytes coded per workgroup (default 16384).  A stream that leaves the buffer or a bad
    chunk_bytes raises ValueError before anything is launched."""
    chunk = check_chunk_bytes(chunk_bytes)
    if not isinstance(scan_dev, torch.Tensor) or not scan_dev.is_cuda or scan_dev.dtype != torch.uint8 or not scan_dev.is_contiguous():
        raise ValueError("deflate_device takes a contiguous uint8 device tensor")
    spans = list(spans)
    if not spans:
        return []
    plan = DeflatePlan(spans, chunk)
    check_deflate_table(plan.rows, chunk, scan_dev.numel(), plan.out_bytes, plan.scratch_bytes, plan.meta_chunks)
    dev = scan_dev.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        d = DeviceDeflater(dev, plan.n, sum(int(sp[1]) for sp in spans), chunk)
        done = d.launch(scan_dev, spans, stream)
        stream.synchronize()
        host = torch.empty(d.host_bytes, dtype=torch.uint8).pin_memory()
        places = d.fetch(done, host, stream)
        stream.synchronize()
    buf = host.numpy()
    return [buf[o:o + n].tobytes() for o, n in places]


def encode_png_device(images, level=6, deflate='host', chunk_bytes=None):
    """[device tensor uint8 [h,w] / uint8 [h,w,3] / uint16 or int16 [h,w,3], ...] -> [PNG file bytes, ...]: the counterpart of
    decode_png_device — decode_png(encode_png_device([x])[0]) and decode_png_device(...) return x exactly (int16 as its uint16
    bit pattern).  The row filters are chosen and applied on the device (unflow_png_filter: least sum of absolute differences
    per row); deflate='host': the host deflates at `level` and assembles IHDR, one IDAT and IEND.  deflate='device': the
    scanlines are coded on the device too (deflate_device; `level` does not apply, chunk_bytes as there) and the host only
    wraps the stream."""
    level = check_level(level)
    on_device = check_deflate_mode(deflate)
    if on_device:
        check_chunk_bytes(chunk_bytes)
    out, spans = scanlines_device(images)
    if out is None:
        return []
    if on_device:
        streams = deflate_device(out, spans, None, chunk_bytes)
        return [assemble_png_z(h, w, depth, ctype, z) for (_, _, h, w, depth, ctype), z in zip(spans, streams)]
    host = out.cpu().numpy()
    return [assemble_png(h, w, depth, ctype, host[off:off + n], level) for off, n, h, w, depth, ctype in spans]


def flo_file_bytes(flow):
    """float32 [h,w,2] -> the bytes of a .flo file (write_flo's)."""
    flow = np.ascontiguousarray(flow, dtype='<f4')
    h, w, _ = flow.shape
    return struct.pack('<f', FLO_TAG) + struct.pack('<ii', w, h) + flow.tobytes()


class DeviceFileWriter:
    """The ordered writer pool of the device encode path: submit(path, kind, payload) queues one file and returns at once;
    a worker deflates, forms the chunk CRCs and writes it.

        kind 'png': payload = (h, w, depth, ctype, scanlines) — host bytes that are already filtered (assemble_png);
        kind 'png_z': payload = (h, w, depth, ctype, zlib stream) — scanlines the device has deflated already
                      (deflate_device): the worker only forms the chunk CRCs and writes (assemble_png_z);
        kind 'flo': payload = the file's bytes (flo_file_bytes), written as they are through the same pool.

    workers is capped by MAX_WORKERS (never sized from os.cpu_count()).  At most `bound` = 2 * workers files are pending
    (submitted and not yet written): a producer that gets ahead blocks in submit, so the memory behind the payloads stays
    bounded.  A payload must stay unchanged until its file is written; the estimator hands over copies.  close() / leaving the
    `with` block waits for every file and raises RuntimeError naming the path of the first (in submission order) file whose
    worker failed, chained to the worker's exception.  Workers receive host bytes only and never touch the GPU — neither a
    launch nor a sync nor a copy — so they may run while another thread captures a graph.  `paths` lists the submitted paths in
    order; `written` and `file_bytes` count what the workers finished."""

    KINDS = ('png', 'png_z', 'flo')

    def __init__(self, workers=8, level=6, compress=zlib.compress):
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.level = check_level(level)
        self.bound = 2 * self.workers
        self.compress = compress
        self.paths = []
        self.written = self.file_bytes = self.pending = self.max_pending = 0
        self._lock = threading.Lock()
        self._room = threading.BoundedSemaphore(self.bound)
        self._error = None                           # (submission number, path, exception) of the earliest failure
        self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="png-deflate")
        self._closed = False

    def submit(self, path, kind, payload):
        if self._closed:
            raise RuntimeError("DeviceFileWriter is closed")
        if kind not in self.KINDS:
            raise ValueError("kind must be one of %s, got %r" % (self.KINDS, kind))
        self._room.acquire()                         # blocks while `bound` files are pending
        with self._lock:
            seq = len(self.paths)
            self.paths.append(path)
            self.pending += 1
            self.max_pending = max(self.max_pending, self.pending)
        self._pool.submit(self._work, seq, path, kind, payload)

    def _work(self, seq, path, kind, payload):
        n = 0
        try:
            if kind == 'png':
                h, w, depth, ctype, scan = payload
                data = assemble_png(h, w, depth, ctype, scan, self.level, self.compress)
            elif kind == 'png_z':
                data = assemble_png_z(*payload)
            else:
                data = payload
            with open(path, 'wb') as f:
                f.write(data)
            n = len(data)
        except BaseException as e:
            with self._lock:
                if self._error is None or seq < self._error[0]:
                    self._error = (seq, path, e)
        finally:
            with self._lock:
                self.pending -= 1
                if n:
                    self.written += 1
                    self.file_bytes += n
            self._room.release()

    def close(self):
        """Wait for every submitted file; raise the first failure."""
        if not self._closed:
            self._closed = True
            self._pool.shutdown(wait=True)
        err, self._error = self._error, None
        if err is not None:
            raise RuntimeError("writing %s failed: %s: %s" % (err[1], type(err[2]).__name__, err[2])) from err[2]

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                        # the caller's exception wins; still leave no thread behind
            self._closed = True
            self._pool.shutdown(wait=True)
        return False
