"""PNG decode on the device: the training input that keeps up with the step.

core/input.py::decode_png reconstructs Average / Paeth scanlines one pixel at a time in the interpreter (seconds per KITTI
frame).  Here the host only parses chunks and inflates (zlib releases the GIL, so a thread pool scales), and the GPU does the
rest (csrc/png_decode.hip):

  * unflow_png_unfilter   the five PNG row filters for a whole batch of images in one launch;
  * unflow_png_to_batch   read_png_image's channel rule, the crop and the normalisation -> float32 [n,H,W,3].

png_scanlines / decode_png_device are the building blocks; DevicePairBatches is the device twin of RawPairBatches (same pair
order, same crop draws, bit-identical batches) with the next batches in flight on a side stream while the step runs.
There is no host fallback: without the library's kernels these raise."""
import collections
import ctypes
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

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
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
    dev = _device(device)
    metas, raws, rows, src, dst = [], [], [], 0, 0
    for data in datas:
        h, w, depth, ctype, raw = png_scanlines(data)
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


class _Slot:
    """Staging and output of one batch in flight.  Every buffer is allocated (and grown) on the CONSUMER's thread, see
    DevicePairBatches._schedule."""

    def __init__(self, n, H, W, dev):
        self.staging = None                       # pinned uint8: the batch's inflated streams, back to back
        self.table_host = torch.empty(n, _lib.PNG_DESC_FIELDS, dtype=torch.int64).pin_memory()
        self.table = torch.empty(n, _lib.PNG_DESC_FIELDS, dtype=torch.int64, device=dev)
        self.raw = self.dec = None                # device: inflated streams, decoded frames
        self.out = torch.empty(2, n // 2, H, W, 3, dtype=torch.float32, device=dev)
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
    """One batch: its slot, its frames [(file, header, oy, ox)] (first frames, then second frames), the kernels' table rows, each
    frame's span in the staging buffer, the byte totals, the workers' futures and the event behind which the slot may be
    rewritten."""

    def __init__(self, slot, examples):
        self.slot = slot
        self.frames = [(fn1, m1, oy, ox) for fn1, _, m1, _, oy, ox in examples] + \
                      [(fn2, m2, oy, ox) for _, fn2, _, m2, oy, ox in examples]
        self.rows, self.spans, src, dst = [], [], 0, 0
        for _, (h, w, depth, ctype), oy, ox in self.frames:
            n_in, n_out = h * (w * _bpp(depth, ctype) + 1), h * w * _bpp(depth, ctype)
            self.rows.append(_table_row(src, dst, h, w, depth, ctype, oy, ox))
            self.spans.append((src, n_in))
            src, dst = src + n_in, dst + n_out
        self.n_raw, self.n_dec = src, dst
        self.free_event = self.futures = self.submitted = None
        self.done = threading.Event()
        self.error = self.ready = self.marks = None
        self.times = {}


class _Pipeline:
    """What the producer thread owns: the worker pool, the side stream and the launches.  It does not refer to the iterator, so
    dropping the iterator stops it (DevicePairBatches.__del__).

    The producer thread only enqueues on the side stream (waits on events, asynchronous copies from pinned memory, the two
    kernels, event records): it never allocates and never synchronises, so it may run while the consumer's thread captures a
    hipGraph of the training step (allocations and synchronising calls of ANY thread are errors during a capture)."""

    def __init__(self, dev, dims, mean, stddev, workers, timing):
        self.dev, self.dims, self.mean, self.stddev, self.timing = dev, dims, mean, stddev, timing
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)), thread_name_prefix="png-inflate")
        self.side = torch.cuda.Stream(dev)
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
        slot.table_host.copy_(torch.tensor(job.rows, dtype=torch.int64))
        errors = [f.exception() for f in job.futures]         # waits for every worker: none is left writing into the slot
        job.times['inflate_s'] = time.perf_counter() - job.submitted          # submit -> last frame staged
        for e in errors:
            if e is not None:
                raise e
        job.times['worker_s'] = sum(f.result() for f in job.futures)          # thread-seconds of the batch's frames
        marks = [torch.cuda.Event(enable_timing=self.timing) for _ in range(4)]
        with torch.cuda.stream(self.side):
            self.side.wait_event(job.free_event)               # the consumer has passed the batch this slot held
            marks[0].record(self.side)
            slot.raw[:job.n_raw].copy_(slot.staging[:job.n_raw], non_blocking=True)
            slot.table.copy_(slot.table_host, non_blocking=True)
            marks[1].record(self.side)
            _unfilter(slot.raw, job.n_raw, slot.dec, job.n_dec, slot.table, len(job.rows), self.side)
            marks[2].record(self.side)
            _to_batch(slot.dec, job.n_dec, slot.table, len(job.rows), H, W, self.mean, self.stddev, slot.out, self.side)
            marks[3].record(self.side)
        slot.uploaded, job.marks, job.ready = marks[1], marks, marks[3]

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.jobs.put(None)
        if threading.current_thread() is not self.thread:
            self.thread.join()
        self.pool.shutdown(wait=True, cancel_futures=True)
        self.side.synchronize()


class DevicePairBatches:
    """The device twin of RawPairBatches: an iterator of (image_1, image_2), two float32 DEVICE tensors [B,H,W,3] that equal what
    RawPairBatches.__next__ returns for the same files and seed, bit for bit.

    Up to `workers` (at most 16) threads read the files and inflate them into pinned staging; the upload and the two kernels run
    on one side stream; `prefetch` batches are in flight while the consumer works.  next() makes the current stream wait for the
    batch's event, so kernels launched on the current stream afterwards (the engine's) see the batch.  The two tensors belong
    to a ring of prefetch + 1 slots: they stay valid for work enqueued on the current stream before the NEXT next() call (which is
    what Trainer.train does: set_input copies them into the engine's buffers); copy them to keep them longer.  A slot is
    rewritten only behind an event recorded on the current stream at that later next().  next() also plans the batch that
    takes the freed slot (pair order and crop draws: PairPlanner), grows the slot's buffers if the batch needs it, waits
    until the slot's last upload has left the pinned staging and hands the batch's files to the workers — everything that
    allocates or synchronises happens on the consumer's thread, between steps.  close() (and garbage collection) stops the
    threads.  Threads only: no other process opens the GPU."""

    def __init__(self, pairs, batch_size, dims, needs_crop, normalize, mean, stddev, seed, device=None, workers=8, prefetch=2,
                 timing=False):
        if prefetch < 1:
            raise ValueError("prefetch must be at least 1")
        self.device = _device(device)
        self.planner = PairPlanner(pairs, batch_size, dims, needs_crop, seed)
        self.batch_size, self.dims, self.prefetch = batch_size, tuple(dims), prefetch
        _lib.lib()                                  # a missing library is an error here, not in the producer thread
        mean = np.asarray(mean, dtype=np.float32) if normalize else None
        self._pipe = _Pipeline(self.device, self.dims, mean, np.float32(stddev) if normalize else None, workers, bool(timing))
        self._inflight = collections.deque()
        self._held = None                           # the slot whose tensors the consumer holds
        self.stage_times = collections.deque(maxlen=64)     # timing=True: per-batch dicts, filled by next()
        self._timed = collections.deque()
        try:
            with torch.cuda.device(self.device):
                slots = [_Slot(2 * batch_size, self.dims[0], self.dims[1], self.device) for _ in range(prefetch + 1)]
            # (slot, event on the current stream behind which the side stream may write it)
            self._free = collections.deque((s, self._mark()) for s in slots)
            for _ in range(prefetch):
                self._schedule()
        except BaseException:
            self._pipe.close()
            raise

    def _mark(self):
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(self.device))
        return e

    def _schedule(self):
        slot, free_event = self._free[0]
        job = _Job(slot, self.planner.next_batch())
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
        job.futures = [self._pipe.pool.submit(_inflate_into, fn, meta, stage[o:o + n])
                       for (fn, meta, _, _), (o, n) in zip(job.frames, job.spans)]
        self._inflight.append(job)
        self._pipe.jobs.put(job)

    def __iter__(self):
        return self

    def __next__(self):
        if self._pipe.closed:
            raise RuntimeError("DevicePairBatches is closed")
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
            while self._free and len(self._inflight) < self.prefetch:
                self._schedule()
        except BaseException:
            self.close()
            raise
        if self._pipe.timing:
            self._collect(job)
        return job.slot.out[0], job.slot.out[1]

    def _collect(self, job):
        self._timed.append(job)
        while self._timed and self._timed[0].marks[3].query():
            j = self._timed.popleft()
            m = j.marks
            self.stage_times.append(dict(j.times, upload_ms=m[0].elapsed_time(m[1]), unfilter_ms=m[1].elapsed_time(m[2]),
                                         to_batch_ms=m[2].elapsed_time(m[3])))

    def close(self):
        self._pipe.close()

    def __del__(self):
        try:
            self._pipe.close()
        except Exception:
            pass
