#!/usr/bin/env python3
"""The training input from PNG files: host decoder against the device decoder, and the step fed by it; one JSON line.

    python tools/loader_bench.py [--batches 60] [--steps 60] [--warmup 5] [--raw-batches 2] [--workers 16] [--prefetch 2]

Writes two sets of 16 KITTI-size frames (384 x 1242 RGB: KITTI's 375 x 1242 made 9 rows taller so that the benchmark's 384 x 512
crop exists; smooth signal plus noise; this tool's own PNG encoder with a filter choice per row) to a temporary directory — one
with every row Paeth, one with a mix of the five filters — and measures, with B = 4 pairs cropped to 384 x 512 (Input's
normalisation on):

  (a) raw      RawPairBatches (the pure-Python decoder), batches per second over --raw-batches batches: seconds per frame;
  (b) device   DevicePairBatches alone, batches per second over --batches batches behind --warmup (device drained at the end);
  (c) fed      Trainer.train-style FlowNetC steps (next(batches); train_step) fed by (b), steps per second, against the same
               steps fed from batches already on the device (the ceiling), and their ratio; and those pre-staged steps with the
               loader's threads and uploads running beside them but its two kernels stubbed out (beside_host_only, Paeth set):
               what the loader costs the step on the host, apart from what it costs on the GPU;
  (d) stages   per batch, from (b)'s own events and clocks: the inflate stage (inflate_ms: from handing the 2B files to the
               worker threads until the last is staged, `prefetch` batches share the pool; worker_thread_ms: the sum of the 2B
               workers' own times, read + inflate + filter check + copy), and upload, unflow_png_unfilter and
               unflow_png_to_batch from device events on the side stream.

(a) runs in this process without a GPU.  Every GPU measurement is a child process of its own under its own time limit; after a
child that failed or ran out of time nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME = (384, 1242)        # KITTI's 375 x 1242, 9 rows taller: the 384 x 512 crop of the benchmarked step must exist
DIMS = (384, 512)
B = 4
N_FRAMES = 16


# ------------------------------------------------------------------------------------------------------------- the encoder
def filter_rows(rows, bpp, filters):
    """uint8 [h, stride] + a filter type per row -> PNG scanlines uint8 [h, 1 + stride].  Vectorised: when encoding, every
    predictor (left, up, upper left) is a shifted copy of the image."""
    import numpy as np
    x = rows.astype(np.int32)
    h = x.shape[0]
    a, b = np.zeros_like(x), np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :-bpp]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, paeth])[np.asarray(filters), np.arange(h)]
    out = np.empty((h, 1 + x.shape[1]), dtype=np.uint8)
    out[:, 0] = filters
    out[:, 1:] = (x - pred) & 255
    return out


def encode_rgb8(arr, filters):
    def chunk(t, body):
        return struct.pack('>I', len(body)) + t + body + struct.pack('>I', zlib.crc32(t + body) & 0xffffffff)
    h, w, _ = arr.shape
    stream = filter_rows(arr.reshape(h, w * 3), 3, filters).tobytes()
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(stream, 6)) + chunk(b'IEND', b''))


def write_sets(root):
    """{'paeth': dir, 'mix': dir}: N_FRAMES frames each, smooth signal plus noise."""
    import numpy as np
    rs = np.random.RandomState(0)
    h, w = FRAME
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    out = {}
    for name in ('paeth', 'mix'):
        d = os.path.join(root, name)
        os.makedirs(d)
        for i in range(N_FRAMES):
            smooth = 128 + 90 * np.sin(xx / 37.0 + i) * np.cos(yy / 23.0 + 0.5 * i)
            img = np.clip(smooth[:, :, None] + np.array([0, 8, -8]) + rs.normal(0, 6, size=(h, w, 3)), 0, 255).astype(np.uint8)
            filters = np.full(h, 4) if name == 'paeth' else rs.randint(0, 5, size=h)
            with open(os.path.join(d, '%06d.png' % i), 'wb') as f:
                f.write(encode_rgb8(img, filters))
        out[name] = d
    return out


def make_input(d):
    from unflow_amd.core.input import Input

    class Data:
        def get_raw_dirs(self):
            return [d]
    return Input(Data(), B, DIMS, normalize=True)


# ------------------------------------------------------------------------------------------------------------- measurements
def raw_rate(d, n):
    it = make_input(d).input_raw(seed=0)
    t0 = time.perf_counter()
    for _ in range(n):
        next(it)
    dt = time.perf_counter() - t0
    return dict(batches=n, batches_per_s=round(n / dt, 5), s_per_frame=round(dt / (n * 2 * B), 4))


def _mean(xs):
    return round(statistics.mean(xs), 4) if xs else None


def _loader(d, a, dev):
    from unflow_amd.core.png_device import DevicePairBatches
    inp = make_input(d)
    return DevicePairBatches(inp.raw_pairs(seed=0), B, DIMS, True, True, inp.mean, inp.stddev, 0, device=dev, workers=a.workers,
                             prefetch=a.prefetch, timing=True)           # what inp.input_raw(seed=0, device=dev) builds, + timing


def _stages(it):
    st = list(it.stage_times)
    return dict(batches=len(st), inflate_ms=_mean([1e3 * s['inflate_s'] for s in st]),
                worker_thread_ms=_mean([1e3 * s['worker_s'] for s in st]), upload_ms=_mean([s['upload_ms'] for s in st]),
                unfilter_ms=_mean([s['unfilter_ms'] for s in st]), to_batch_ms=_mean([s['to_batch_ms'] for s in st]))


def child_device(d, a):
    """(b) and (d)."""
    import torch
    it = _loader(d, a, torch.device('cuda:0'))
    for _ in range(a.warmup):
        next(it)
    torch.cuda.synchronize()
    it.stage_times.clear()
    t0 = time.perf_counter()
    for _ in range(a.batches):
        next(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = dict(batches=a.batches, batches_per_s=round(a.batches / dt, 3), ms_per_batch=round(1e3 * dt / a.batches, 3),
               stages=_stages(it))
    it.close()
    print(json.dumps(out))


def child_steps(d, a, mode):
    """(c): `steps` Trainer.train-style steps behind `warmup`.  mode 'fed': fed by the device loader; 'ceiling': from batches
    already on the device; 'beside': from batches already on the device while a loader whose two kernels are stubbed out is
    driven at the same rate and its batches are dropped — the loader's threads and uploads without its GPU work, which tells
    the host side of the fed run's loss from the GPU side.  Beside the rate: the host time per step inside next() (waiting for a
    batch shows here) and inside train_step, and the loader's stage times while the step runs beside it."""
    import torch
    from unflow_amd.core.train import Trainer
    dev = torch.device('cuda:0')
    params = dict(flownet='C', learning_rate=1e-5, decay_interval=100000, save_interval=1000, display_interval=1000)
    tr = Trainer(B, DIMS[0], DIMS[1], params, device=dev, seed=1, augment=True)
    loader = None
    if mode == 'beside':
        from unflow_amd.core import png_device
        png_device._unfilter = png_device._to_batch = lambda *args: None
    if mode != 'ceiling':
        loader = _loader(d, a, dev)            # created before the first step, as Trainer.train does: the graph capture of the
    if mode == 'fed':                          # first step runs beside the loader's threads
        batches = loader
    else:
        g = torch.Generator().manual_seed(0)
        ring = [tuple((torch.rand(B, DIMS[0], DIMS[1], 3, generator=g) - 0.4).to(dev) for _ in range(2)) for _ in range(4)]

        def staged():
            for i in range(a.warmup + a.steps):
                if loader is not None:
                    next(loader)
                yield ring[i % 4]
        batches = staged()
    tr.iteration = 0
    for _ in range(a.warmup):
        loss = tr.train_step(*next(batches))
    torch.cuda.synchronize()
    if loader is not None:
        loader.stage_times.clear()
    t_next = t_step = 0.0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        t1 = time.perf_counter()
        batch = next(batches)
        t2 = time.perf_counter()
        loss = tr.train_step(*batch)
        t_next, t_step = t_next + t2 - t1, t_step + time.perf_counter() - t2
    loss = float(loss)
    dt = time.perf_counter() - t0
    out = dict(steps=a.steps, steps_per_s=round(a.steps / dt, 3), ms_per_step=round(1e3 * dt / a.steps, 3),
               host_ms_in_next=round(1e3 * t_next / a.steps, 3), host_ms_in_train_step=round(1e3 * t_step / a.steps, 3),
               last_loss_finite=bool(loss == loss and abs(loss) != float('inf')))
    if loader is not None:
        out['stages'] = _stages(loader)
        loader.close()
    print(json.dumps(out))


def run_child(args, limit):
    """One GPU measurement in a process of its own, under its own time limit -> (result or None, error or None)."""
    print("loader_bench: " + " ".join(args[:4]), file=sys.stderr, flush=True)
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, dict(error="time limit of %d s" % limit)
    if r.returncode != 0:
        return None, dict(error="exit %d" % r.returncode, tail=r.stderr.decode(errors='replace')[-600:])
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]
    return json.loads(lines[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=60)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--raw-batches', type=int, default=2)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--prefetch', type=int, default=2)
    ap.add_argument('--limit', type=int, default=240, help='time limit of each GPU child, seconds')
    ap.add_argument('--child', choices=('device', 'fed', 'ceiling', 'beside'), help=argparse.SUPPRESS)
    ap.add_argument('--dir', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == 'device':
        return child_device(a.dir, a)
    if a.child:
        return child_steps(a.dir, a, a.child)
    res = dict(metric='loader_batches_per_s_and_fed_step_fraction', frame=list(FRAME) + [3], dims=list(DIMS),
               B=B, frames_per_set=N_FRAMES, workers=min(a.workers, 16), prefetch=a.prefetch, warmup=a.warmup, sets={})
    common = ['--batches', str(a.batches), '--steps', str(a.steps), '--warmup', str(a.warmup), '--workers', str(a.workers),
              '--prefetch', str(a.prefetch)]
    with tempfile.TemporaryDirectory(prefix='loader_bench_') as root:
        sets = write_sets(root)
        gpu_ok = True
        for name, d in sets.items():
            print("loader_bench: host decoder, set " + name, file=sys.stderr, flush=True)
            out = res['sets'][name] = dict(raw=raw_rate(d, a.raw_batches))
            for key, child in (('device', 'device'), ('ceiling', 'ceiling'), ('fed', 'fed'), ('beside_host_only', 'beside')):
                if name == 'mix' and key in ('ceiling', 'beside_host_only'):
                    if key == 'ceiling':
                        out[key] = res['sets']['paeth'].get('ceiling')     # the same steps: measured once
                    continue
                if not gpu_ok:
                    out[key] = dict(error="not run: an earlier GPU step failed")
                    continue
                r, err = run_child(['--child', child, '--dir', d] + common, a.limit)
                out[key] = r if err is None else err
                gpu_ok = err is None
            if isinstance(out.get('device'), dict) and 'batches_per_s' in out['device']:
                out['device_over_raw'] = round(out['device']['batches_per_s'] / out['raw']['batches_per_s'], 1)
            if all(isinstance(out.get(k), dict) and 'steps_per_s' in out[k] for k in ('fed', 'ceiling')):
                out['fed_over_ceiling'] = round(out['fed']['steps_per_s'] / out['ceiling']['steps_per_s'], 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
