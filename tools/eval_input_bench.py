#!/usr/bin/env python3
"""The evaluation and fine-tuning input from PNG files: the host readers against the device readers, and the consumers fed by
them; one JSON line.

    python tools/eval_input_bench.py [--examples 64] [--steps 40] [--warmup 4] [--host-examples 1] [--workers 16] [--prefetch 2]

Writes two KITTI trees of 8 examples per dataset (375 x 1242: 8-bit RGB frames, smooth signal plus noise; 16-bit RGB flow_occ /
flow_noc maps, a smooth flow field with a random validity channel; this tool's PNG encoder with a filter choice per row) to a
temporary directory — one with every row Paeth, one with a mix of the five filters — and measures per tree:

  (a) reader    examples per second of KITTIInput.input_train_2015 (four files per example), batch 4, dims 384 x 1280: the host
                iterator over --host-examples examples, the device iterator (DeviceEvalBatches) over --examples behind --warmup
                batches, the device drained at the end;
  (b) evaluate  FlowEstimator.evaluate (FlowNetC, batch 4, 384 x 1280) examples per second fed by either, and the time of the
                replayed batch alone (the ceiling: what tools/inference_bench.py measures);
  (c) finetune  supervised FlowNetC steps (B = 4, 320 x 768, Trainer.train's loop) fed by DeviceGTBatches, against the same steps
                from batches already on the device (the ceiling), and against steps fed by the host iterator (one step);
  (d) stages    per batch, from the device iterators' own events and clocks, alone (a) and beside the step (c): inflate (files
                handed to the pool -> last staged; the sum of the workers' own times), upload, unflow_png_unfilter,
                unflow_png_to_window and unflow_png_to_flow_gt.

--dataset sintel measures the .flo input instead: a Sintel tree of two scenes of five frames (436 x 1024: 8-bit RGB
frames in both passes, a mix of the five filters per row; .flo flow files; 8-bit grey invalid and occlusion maps), and
SintelInput.input_train_clean at dims 512 x 1024, batch 4 — batches per second of the host iterator (over --host-examples examples,
at least one batch) and of the device iterator (over --examples behind --warmup batches, the device drained at the end), with the
device iterator's stage times (the .flo bodies count under inflate: they are read, not inflated).  One JSON line, no threshold.

The host figures of (a) run in this process without a GPU.  Every GPU measurement is a child process of its own under its own time
limit; after a child that failed or ran out of time nothing more is started on the GPU.  The host-fed evaluate reads batches of
one example, so that its clock covers exactly the examples it counts."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loader_bench import _mean, filter_rows      # noqa: E402  (the vectorised filter step of that tool's encoder)

FRAME = (375, 1242)
EVAL_DIMS = (384, 1280)
TRAIN_DIMS = (320, 768)
B = 4
N_EXAMPLES = 8             # per dataset
LAYOUTS = (('data_scene_flow/training', 'image_2'), ('data_stereo_flow/training', 'colored_0'))


# ------------------------------------------------------------------------------------------------------------- the files
def encode(arr, filters):
    """uint8 [h, w, 3] -> 8-bit RGB PNG, uint16 [h, w, 3] -> 16-bit RGB PNG (big-endian samples), row y filtered by filters[y]."""
    import numpy as np

    def chunk(t, body):
        return struct.pack('>I', len(body)) + t + body + struct.pack('>I', zlib.crc32(t + body) & 0xffffffff)
    h, w, _ = arr.shape
    depth = 8 * arr.dtype.itemsize
    rows = np.ascontiguousarray(arr.astype('>u2') if depth == 16 else arr).view(np.uint8).reshape(h, -1)
    stream = filter_rows(rows, 3 * depth // 8, filters).tobytes()
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(stream, 6)) + chunk(b'IEND', b''))


def write_trees(root):
    """{'paeth': tree, 'mix': tree}: both training layouts, N_EXAMPLES examples each."""
    import numpy as np
    rs = np.random.RandomState(0)
    h, w = FRAME
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    out = {}
    for name in ('paeth', 'mix'):
        filt = (lambda: np.full(h, 4)) if name == 'paeth' else (lambda: rs.randint(0, 5, size=h))

        def put(path, arr):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'wb') as f:
                f.write(encode(arr, filt()))
        for base, img in LAYOUTS:
            for i in range(N_EXAMPLES):
                for k in (10, 11):
                    smooth = 128 + 90 * np.sin(xx / 37.0 + i + 0.1 * k) * np.cos(yy / 23.0 + 0.5 * i)
                    frame = np.clip(smooth[:, :, None] + np.array([0, 8, -8]) + rs.normal(0, 6, size=(h, w, 3)), 0, 255)
                    put(os.path.join(root, name, base, img, '%06d_%d.png' % (i, k)), frame.astype(np.uint8))
                u = 3.0 + 2.0 * np.sin(xx / 97.0 + i) + 0.02 * rs.normal(0, 1, size=(h, w))
                v = -1.0 + 1.5 * np.cos(yy / 53.0)
                for sub, p in (('flow_occ', 0.35), ('flow_noc', 0.28)):
                    valid = rs.rand(h, w) < p
                    u16 = np.zeros((h, w, 3), np.uint16)
                    u16[..., 0], u16[..., 1] = np.round(u * 64.0 + 2 ** 15) * valid, np.round(v * 64.0 + 2 ** 15) * valid
                    u16[..., 2] = valid
                    put(os.path.join(root, name, base, sub, '%06d_10.png' % i), u16)
        out[name] = os.path.join(root, name)
    return out


class Data:
    def __init__(self, root):
        self.current_dir = root


# ------------------------------------------------------------------------------------------------------------- sintel
SINTEL_FRAME = (436, 1024)
SINTEL_DIMS = (512, 1024)
SINTEL_SCENES = (5, 5)     # frames per scene: 8 pairs


def encode_grey(arr, filters):
    """uint8 [h, w] -> 8-bit greyscale PNG, row y filtered by filters[y]."""
    def chunk(t, body):
        return struct.pack('>I', len(body)) + t + body + struct.pack('>I', zlib.crc32(t + body) & 0xffffffff)
    h, w = arr.shape
    stream = filter_rows(arr, 1, filters).tobytes()
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(stream, 6)) + chunk(b'IEND', b''))


def write_sintel_tree(root):
    import numpy as np
    from unflow_amd.core.input import write_flo
    rs = np.random.RandomState(0)
    h, w = SINTEL_FRAME
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')

    def put(path, data):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(data)
    tr = os.path.join(root, 'sintel', 'training')
    for s, n in enumerate(SINTEL_SCENES):
        scene = 'scene_%d' % s
        for i in range(n):
            name = 'frame_%04d' % (i + 1)
            for p, noise in (('clean', 3), ('final', 8)):
                smooth = 128 + 90 * np.sin(xx / 41.0 + i + s) * np.cos(yy / 29.0 + 0.5 * i)
                frame = np.clip(smooth[:, :, None] + np.array([0, 8, -8]) + rs.normal(0, noise, size=(h, w, 3)), 0, 255)
                put(os.path.join(tr, p, scene, name + '.png'), encode(frame.astype(np.uint8), rs.randint(0, 5, size=h)))
            blobs = (np.sin(xx / 53.0 + i) * np.cos(yy / 31.0 + s) > 0.8)
            put(os.path.join(tr, 'invalid', scene, name + '.png'),
                encode_grey((blobs & (xx < 64)).astype(np.uint8) * 255, rs.randint(0, 5, size=h)))
            if i == n - 1:
                continue
            flow = np.stack([3.0 + 2.0 * np.sin(xx / 97.0 + i), -1.0 + 1.5 * np.cos(yy / 53.0)], axis=2).astype(np.float32)
            os.makedirs(os.path.join(tr, 'flow', scene), exist_ok=True)
            write_flo(os.path.join(tr, 'flow', scene, name + '.flo'), flow)
            put(os.path.join(tr, 'occlusions', scene, name + '.png'), encode_grey(blobs.astype(np.uint8) * 255, rs.randint(0, 5, size=h)))
    return root


def sintel_input(tree):
    from unflow_amd.sintel.input import SintelInput
    return SintelInput(Data(tree), B, SINTEL_DIMS, normalize=False)


def child_sintel_reader(tree, a):
    import torch
    from unflow_amd.core.png_device import DeviceEvalBatches
    sin = sintel_input(tree)
    pairs, gt = sin.train_files('sintel/training/clean')
    examples = a.examples + a.warmup * B
    rep = -(-examples // len(pairs))
    cut = lambda x: (x * rep)[:examples]          # noqa: E731
    it = DeviceEvalBatches(cut(pairs), B, SINTEL_DIMS, False, sin.mean, sin.stddev, gt_lists=[cut(g) for g in gt], gt_kind='sintel',
                           device=torch.device('cuda:0'), workers=a.workers, prefetch=a.prefetch, timing=True)
    for _ in range(a.warmup):
        next(it)
    torch.cuda.synchronize()
    it.stage_times.clear()
    t0, n = time.perf_counter(), 0
    for _batch in it:
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = stages(it)
    st['sintel_gt_ms'] = st.pop('to_flow_gt_ms')
    print(json.dumps(dict(batches=n, batches_per_s=round(n / dt, 3), ms_per_batch=round(1e3 * dt / n, 3), stages=st)))


def main_sintel(a):
    res = dict(metric='sintel_input_host_vs_device', frame=list(SINTEL_FRAME) + [3], dims=list(SINTEL_DIMS), B=B,
               pairs=sum(n - 1 for n in SINTEL_SCENES), files_per_example=5, workers=min(a.workers, 16), prefetch=a.prefetch,
               warmup=a.warmup)
    with tempfile.TemporaryDirectory(prefix='eval_input_bench_') as root:
        tree = write_sintel_tree(root)
        print("eval_input_bench: sintel host reader", file=sys.stderr, flush=True)
        n = max(1, -(-a.host_examples // B))
        t0 = time.perf_counter()
        for _, _batch in zip(range(n), sintel_input(tree).input_train_clean()):
            pass
        dt = time.perf_counter() - t0
        res['host'] = dict(batches=n, batches_per_s=round(n / dt, 5), s_per_batch=round(dt / n, 3))
        r, err = run_child(['--child', 'sintel_reader', '--dir', tree, '--examples', str(a.examples), '--warmup', str(a.warmup),
                            '--workers', str(a.workers), '--prefetch', str(a.prefetch)], a.limit)
        res['device'] = r if err is None else err
        if err is None:
            res['device_over_host'] = round(r['batches_per_s'] / res['host']['batches_per_s'], 1)
    print(json.dumps(res))


def kitti_input(tree, dims, normalize):
    from unflow_amd.kitti.input import KITTIInput
    return KITTIInput(Data(tree), B, dims, normalize=normalize)


def eval_loader(tree, a, dev, examples):
    """input_train_2015(device=dev) over the tree's pairs repeated up to `examples` examples, with timing."""
    from unflow_amd.core.png_device import DeviceEvalBatches
    kin = kitti_input(tree, EVAL_DIMS, False)
    pairs = kin.test_pairs('data_scene_flow/training/image_2')
    occ, noc = kin._flow_files('data_scene_flow/training', None)
    rep = -(-examples // len(pairs))
    cut = lambda x: (x * rep)[:examples]          # noqa: E731
    return DeviceEvalBatches(cut(pairs), B, EVAL_DIMS, False, kin.mean, kin.stddev, gt_lists=(cut(occ), cut(noc)), device=dev,
                             workers=a.workers, prefetch=a.prefetch, timing=True)


def gt_loader(tree, a, dev):
    from unflow_amd.core.png_device import DeviceGTBatches
    kin = kitti_input(tree, TRAIN_DIMS, True)
    return DeviceGTBatches(kin.train_gt_files(0), B, TRAIN_DIMS, True, kin.mean, kin.stddev, seed=0, device=dev,
                           workers=a.workers, prefetch=a.prefetch, timing=True)


def stages(it):
    st = list(it.stage_times)
    return dict(batches=len(st), inflate_ms=_mean([1e3 * s['inflate_s'] for s in st]),
                worker_thread_ms=_mean([1e3 * s['worker_s'] for s in st]), upload_ms=_mean([s['upload_ms'] for s in st]),
                unfilter_ms=_mean([s['unfilter_ms'] for s in st]), to_window_ms=_mean([s['to_batch_ms'] for s in st]),
                to_flow_gt_ms=_mean([s['flow_gt_ms'] for s in st if 'flow_gt_ms' in s]))


# ------------------------------------------------------------------------------------------------------------- measurements
def host_reader_rate(tree, n):
    it = kitti_input(tree, EVAL_DIMS, False)
    it.batch_size = 1
    t0 = time.perf_counter()
    for _, _batch in zip(range(n), it.input_train_2015()):
        pass
    dt = time.perf_counter() - t0
    return dict(examples=n, examples_per_s=round(n / dt, 5), s_per_example=round(dt / n, 3))


def child_reader(tree, a):
    """(a) device, (d) alone."""
    import torch
    it = eval_loader(tree, a, torch.device('cuda:0'), a.examples + a.warmup * B)
    for _ in range(a.warmup):
        next(it)
    torch.cuda.synchronize()
    it.stage_times.clear()
    t0, n = time.perf_counter(), 0
    for batch in it:
        n += batch[0].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(examples=n, examples_per_s=round(n / dt, 2), ms_per_batch=round(1e3 * dt * B / n, 3), stages=stages(it))))


def child_evaluate(tree, a, mode):
    """(b): FlowEstimator.evaluate fed by the device iterator ('device') or the host iterator ('host'), and the replay alone."""
    import torch
    from unflow_amd.core.inference import FlowEstimator
    dev = torch.device('cuda:0')
    est = FlowEstimator(dict(flownet='C'), B, net_size=EVAL_DIMS, device=dev)
    est.load_tf_params(est.engine.init_params(seed=1))
    est.evaluate(eval_loader(tree, a, dev, B))                  # builds the graph
    torch.cuda.synchronize()
    n = a.examples if mode == 'device' else a.host_examples
    kin = kitti_input(tree, EVAL_DIMS, False)
    kin.batch_size = 1          # the host generator decodes a whole batch before it yields: batches of one, so that exactly n are read
    batches = eval_loader(tree, a, dev, n) if mode == 'device' else kin.input_train_2015()
    t0 = time.perf_counter()
    res = est.evaluate(batches, num=n)
    dt = time.perf_counter() - t0
    out = dict(examples=res['num_examples'], examples_per_s=round(res['num_examples'] / dt, 4),
               ms_per_example=round(1e3 * dt / res['num_examples'], 3))
    if mode == 'device':
        t0 = time.perf_counter()
        for _ in range(50):
            est._run()
        torch.cuda.synchronize()
        out['replay_ms_per_batch'] = round(1e3 * (time.perf_counter() - t0) / 50, 3)
    print(json.dumps(out))


def child_steps(tree, a, mode):
    """(c): supervised steps.  'fed': DeviceGTBatches; 'ceiling': batches already on the device; 'host': the host iterator
    (--host-examples steps behind one pre-staged step that builds the graph)."""
    import torch
    from unflow_amd.core.train import Trainer
    dev = torch.device('cuda:0')
    params = dict(flownet='C', learning_rate=1e-5, decay_interval=100000, save_interval=1000, display_interval=1000)
    tr = Trainer(B, TRAIN_DIMS[0], TRAIN_DIMS[1], params, device=dev, seed=1, augment=True, supervised=True)
    loader = gt_loader(tree, a, dev) if mode == 'fed' else None
    g = torch.Generator().manual_seed(0)
    H, W = TRAIN_DIMS
    ring = [((torch.rand(B, H, W, 3, generator=g) - 0.4).to(dev), (torch.rand(B, H, W, 3, generator=g) - 0.4).to(dev),
             torch.randn(B, H, W, 2, generator=g).to(dev), (torch.rand(B, H, W, 1, generator=g) < 0.3).float().to(dev))
            for _ in range(4)]
    warmup, steps = (a.warmup, a.steps) if mode != 'host' else (1, a.host_examples)
    if mode == 'fed':
        batches = loader
    elif mode == 'ceiling':
        batches = (ring[i % 4] for i in range(warmup + steps))
    else:
        host = kitti_input(tree, TRAIN_DIMS, True).input_train_gt(0, seed=0)
        batches = (ring[0] if i < warmup else next(host) for i in range(warmup + steps))
    tr.iteration = 0
    step = lambda b: tr.train_step(b[0], b[1], target=(b[2], b[3]))      # noqa: E731
    for _ in range(warmup):
        loss = step(next(batches))
    torch.cuda.synchronize()
    if loader is not None:
        loader.stage_times.clear()
    t_next = t_step = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        batch = next(batches)
        t2 = time.perf_counter()
        loss = step(batch)
        t_next, t_step = t_next + t2 - t1, t_step + time.perf_counter() - t2
    loss = float(loss)
    dt = time.perf_counter() - t0
    out = dict(steps=steps, steps_per_s=round(steps / dt, 4), ms_per_step=round(1e3 * dt / steps, 3),
               host_ms_in_next=round(1e3 * t_next / steps, 3), host_ms_in_train_step=round(1e3 * t_step / steps, 3),
               last_loss_finite=bool(loss == loss and abs(loss) != float('inf')))
    if loader is not None:
        out['stages'] = stages(loader)
        loader.close()
    print(json.dumps(out))


def child_limit(child, a, host_s_per_example):
    """The time limit of a GPU child: --limit, plus — for the two children that decode on the host — three times what the
    host reader just took for the same files (host_fed decodes B examples of three files per step, the reader four files)."""
    host_examples = dict(evaluate_host=a.host_examples, host_fed=B * a.host_examples).get(child, 0)
    return a.limit + int(3 * host_s_per_example * host_examples)


def run_child(args, limit):
    """One GPU measurement in a process of its own, under its own time limit -> (result or None, error or None)."""
    print("eval_input_bench: " + " ".join(args[:4]), file=sys.stderr, flush=True)
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, dict(error="time limit of %d s" % limit)
    if r.returncode != 0:
        return None, dict(error="exit %d" % r.returncode, tail=r.stderr.decode(errors='replace')[-600:])
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]
    return json.loads(lines[-1]), None


CHILDREN = ('reader', 'evaluate_device', 'evaluate_host', 'ceiling', 'fed', 'host_fed')       # of --dataset kitti


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--examples', type=int, default=64)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--host-examples', type=int, default=1)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--prefetch', type=int, default=2)
    ap.add_argument('--limit', type=int, default=240, help='time limit of each GPU child, seconds (the host-fed children get their measured decode time on top)')
    ap.add_argument('--dataset', choices=('kitti', 'sintel'), default='kitti', help='sintel: the .flo input alone (see above)')
    ap.add_argument('--child', choices=CHILDREN + ('sintel_reader',), help=argparse.SUPPRESS)
    ap.add_argument('--dir', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == 'sintel_reader':
        return child_sintel_reader(a.dir, a)
    if a.dataset == 'sintel' and not a.child:
        return main_sintel(a)
    if a.child == 'reader':
        return child_reader(a.dir, a)
    if a.child in ('evaluate_device', 'evaluate_host'):
        return child_evaluate(a.dir, a, a.child.split('_')[1])
    if a.child:
        return child_steps(a.dir, a, dict(ceiling='ceiling', fed='fed', host_fed='host')[a.child])
    res = dict(metric='eval_and_finetune_input_host_vs_device', frame=list(FRAME) + [3], eval_dims=list(EVAL_DIMS),
               train_dims=list(TRAIN_DIMS), B=B, examples_per_dataset=N_EXAMPLES, workers=min(a.workers, 16), prefetch=a.prefetch,
               warmup=a.warmup, sets={})
    common = ['--examples', str(a.examples), '--steps', str(a.steps), '--warmup', str(a.warmup), '--host-examples',
              str(a.host_examples), '--workers', str(a.workers), '--prefetch', str(a.prefetch)]
    with tempfile.TemporaryDirectory(prefix='eval_input_bench_') as root:
        trees = write_trees(root)
        gpu_ok = True
        for name, tree in trees.items():
            print("eval_input_bench: host reader, set " + name, file=sys.stderr, flush=True)
            out = res['sets'][name] = dict(reader_host=host_reader_rate(tree, a.host_examples))
            for child in CHILDREN:
                key = 'reader_device' if child == 'reader' else child
                if name == 'mix' and child == 'ceiling':
                    out[key] = res['sets']['paeth'].get('ceiling')         # the same steps: measured once
                    continue
                if not gpu_ok:
                    out[key] = dict(error="not run: an earlier GPU step failed")
                    continue
                r, err = run_child(['--child', child, '--dir', tree] + common,
                                   child_limit(child, a, out['reader_host']['s_per_example']))
                out[key] = r if err is None else err
                gpu_ok = err is None
            ok = lambda k, f: isinstance(out.get(k), dict) and f in out[k]          # noqa: E731
            if ok('reader_device', 'examples_per_s'):
                out['reader_device_over_host'] = round(out['reader_device']['examples_per_s'] / out['reader_host']['examples_per_s'], 1)
            if ok('evaluate_device', 'examples_per_s') and ok('evaluate_host', 'examples_per_s'):
                out['evaluate_device_over_host'] = round(out['evaluate_device']['examples_per_s'] /
                                                         out['evaluate_host']['examples_per_s'], 1)
            if ok('fed', 'steps_per_s') and ok('ceiling', 'steps_per_s'):
                out['fed_over_ceiling'] = round(out['fed']['steps_per_s'] / out['ceiling']['steps_per_s'], 4)
            if ok('fed', 'steps_per_s') and ok('host_fed', 'steps_per_s'):
                out['fed_over_host_fed'] = round(out['fed']['steps_per_s'] / out['host_fed']['steps_per_s'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
