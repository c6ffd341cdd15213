#!/usr/bin/env python3
"""Flow files from the inference graph: the host PNG writers against the device encode path; one JSON line.

    python tools/export_bench.py [--frames 17] [--rounds 3] [--kernel-reps 50] [--out FILE]

One process, FlowNetC, B = 4, network 384 x 1280, a clip of --frames uint8 frames of 375 x 1242 with real motion (every frame is
the one before shifted, attenuated, plus noise on a smooth structure — tests/test_sequence_gpu.py::clip), random weights with
the last flow head scaled up so that the flow is not flat.  FlowEstimator(sequence=True).export_sequence writes the clip's
frames - 1 KITTI 16-bit flow PNGs to a temporary directory with

  (a) workers=0            the host writers (filter 0 on every row, zlib level 6, one file after another): the baseline;
  (b) workers=1, 4, 8      unflow_png_filter behind each replay, a writer pool of that many threads, level 6;
  (c) workers=8, level=1
  (d) workers=1, 4, 8, deflate='device'   unflow_deflate behind the filter launch: the pool only forms the CRCs and writes;

--rounds times each, a round being (a), (b) x 3, (c), (d) x 3 in that order, so every figure alternates with the baseline and
with (c), the yardstick of (d): files per
second of each run (all values, not a mean) and bytes per file (the same flows in every configuration).  Beside them: the
replay of the captured graph per pair, and unflow_png_filter on one replay's B flow maps, by device events (median and
minimum of --kernel-reps), with the bytes it must move (the int16 samples read once, the scanlines written once) and the
rate that gives; unflow_deflate on the same B maps' scanlines at every chunk size of CHUNKS (the A/B behind the default:
device events, median and minimum, and the compressed bytes), zlib's own sizes of those scanlines for comparison, and what a
writer thread and the copy back still cost per file in (d): the two chunk CRCs (assemble_png_z), the file write, and the
device-to-host copy of one compressed stream."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 4
NET = (384, 1280)
FRAME = (375, 1242)
CONFIGS = [('host_w0_l6', 0, 6, 'host'), ('pool_w1_l6', 1, 6, 'host'), ('pool_w4_l6', 4, 6, 'host'), ('pool_w8_l6', 8, 6, 'host'),
           ('pool_w8_l1', 8, 1, 'host'), ('dev_w1', 1, 6, 'device'), ('dev_w4', 4, 6, 'device'), ('dev_w8', 8, 6, 'device')]
YARDSTICK = 'pool_w8_l1'
CHUNKS = (8192, 16384, 32768, 65535)


def clip(T, h, w, seed):
    """tests/test_sequence_gpu.py::clip on a smooth structure: uint8 frames, each the one before shifted by (2, -3), attenuated,
    plus noise."""
    import numpy as np
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    smooth = 128 + 90 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    f = np.clip(smooth[:, :, None] + np.array([0, 8, -8]) + rs.normal(0, 20, size=(h, w, 3)), 0, 255)
    out = [f]
    for _ in range(T - 1):
        out.append(np.roll(out[-1], shift=(2, -3), axis=(0, 1)) * 0.9 + rs.rand(h, w, 3) * 25)
    return [np.clip(np.rint(f), 0, 255).astype(np.uint8) for f in out]


def event_ms(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=17)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-reps', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    import torch
    from unflow_amd.core import png_device as P
    from unflow_amd.core.inference import FlowEstimator
    dev = torch.device('cuda:0')
    est = FlowEstimator(dict(flownet='C'), B, net_size=NET, max_frame=FRAME, device=dev, sequence=True)
    tfp = est.engine.init_params(seed=31)
    est.load_tf_params({k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()})
    frames = clip(a.frames, FRAME[0], FRAME[1], 0)
    n_files = a.frames - 1
    flows = est.estimate_sequence(frames)                          # warm-up: builds the graph
    res = dict(metric='export_files_per_s', B=B, net=list(NET), frame=list(FRAME), files_per_run=n_files, rounds=a.rounds,
               flow_abs_max=round(max(float(abs(f).max()) for f in flows), 3), configs={})
    runs = {name: dict(workers=w, level=lv, deflate=df, files_per_s=[], bytes_per_file=None) for name, w, lv, df in CONFIGS}
    with tempfile.TemporaryDirectory(prefix='export_bench_') as root:
        for r in range(a.rounds):
            for name, w, lv, df in CONFIGS:
                d = os.path.join(root, '%s_%d' % (name, r))
                t0 = time.perf_counter()
                paths = est.export_sequence(frames, d, fmt='png', workers=w, level=lv, deflate=df)
                dt = time.perf_counter() - t0
                assert len(paths) == n_files
                runs[name]['files_per_s'].append(round(n_files / dt, 3))
                runs[name]['bytes_per_file'] = round(sum(os.path.getsize(p) for p in paths) / n_files)
                print("export_bench: round %d %s %.2f files/s" % (r, name, n_files / dt), file=sys.stderr, flush=True)
    res['configs'] = runs
    base = runs['host_w0_l6']['files_per_s']
    for name, _, _, df in CONFIGS[1:]:
        runs[name]['faster_than_host'] = min(runs[name]['files_per_s']) > max(base)      # slowest run against the baseline's fastest
        if df == 'device':                                                               # and against (c)'s fastest
            runs[name]['faster_than_' + YARDSTICK] = min(runs[name]['files_per_s']) > max(runs[YARDSTICK]['files_per_s'])
    # the replay per pair, and the filter kernel on one replay's B flow maps
    rep = event_ms(est.graph.replay, 20)
    res['replay_ms_per_pair'] = dict(median=round(statistics.median(rep) / B, 4), min=round(min(rep) / B, 4))
    h, w = FRAME
    surf = [P.PngSurface(est.out_u16, B, FRAME[0], FRAME[1], 3, 2)]
    rows, spans, total, max_h, max_row = P.plan_scanlines(surf, [(0, i, h, w) for i in range(B)])
    table = torch.from_numpy(rows).to(dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    launch = lambda: P.filter_scanlines(surf, table, B, max_h, max_row, out, stream)      # noqa: E731
    launch()
    torch.cuda.synchronize()
    ms = event_ms(launch, a.kernel_reps)
    moved = B * h * w * 6 + total
    res['filter_kernel'] = dict(images=B, ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4),
                                bytes_read=B * h * w * 6, bytes_written=total,
                                tb_per_s_median=round(moved / (statistics.median(ms) * 1e-3) / 1e12, 4))
    filt = out.cpu().numpy()
    hist = [0] * 5
    for off, n, hh, _, _, _ in spans:
        for f in filt[off:off + n].reshape(hh, n // hh)[:, 0].tolist():
            hist[f] += 1
    res['filter_histogram'] = hist
    # unflow_deflate on those scanlines, per chunk size; the sizes against zlib's
    import zlib
    from unflow_amd import _lib
    res['deflate_kernel'] = {}
    streams = None
    for chunk in CHUNKS:
        plan = P.DeflatePlan(spans, chunk)
        bufs = dict(table=torch.from_numpy(plan.rows).to(dev), sizes=torch.zeros(B, dtype=torch.int64, device=dev),
                    scratch=torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev),
                    meta=torch.zeros(plan.meta_chunks * _lib.DEFLATE_META, dtype=torch.int32, device=dev),
                    z=torch.empty(plan.out_bytes, dtype=torch.uint8, device=dev))
        launch = lambda: P.deflate_launch(out, plan.rows, bufs['table'], plan.max_chunks, chunk, bufs['scratch'], bufs['meta'],   # noqa: E731
                                          bufs['z'], bufs['sizes'], stream)
        launch()
        torch.cuda.synchronize()
        ms = event_ms(launch, a.kernel_reps)
        sizes = bufs['sizes'].cpu().numpy().tolist()
        codings = bufs['meta'].cpu().numpy().reshape(-1, _lib.DEFLATE_META)[:, 3]
        res['deflate_kernel'][str(chunk)] = dict(
            images=B, chunks=int(plan.meta_chunks), ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4),
            bytes_in=total, bytes_out=int(sum(sizes)), codings=[int((codings == k).sum()) for k in range(3)],
            gb_per_s_median=round(total / (statistics.median(ms) * 1e-3) / 1e9, 2))
        if chunk == _lib.DEFLATE_CHUNK_DEFAULT:
            z = bufs['z'].cpu().numpy()
            streams = [z[dst:dst + n].tobytes() for (dst, _), n in zip(plan.places, sizes)]
            for (off, n, _, _, _, _), zs in zip(spans, streams):
                assert zlib.decompress(zs) == filt[off:off + n].tobytes()
    res['deflate_chunk_default'] = _lib.DEFLATE_CHUNK_DEFAULT
    maps = [filt[off:off + n].tobytes() for off, n, _, _, _, _ in spans]

    def zsize(**kw):
        total_z = 0
        for one in maps:
            c = zlib.compressobj(**kw)
            total_z += len(c.compress(one)) + len(c.flush())
        return total_z
    res['bytes_of_the_maps'] = dict(scanlines=total, device=sum(len(z) for z in streams), zlib_l6=zsize(level=6), zlib_l1=zsize(level=1),
                                    zlib_huffman_only=zsize(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
                                    zlib_rle=zsize(level=6, strategy=zlib.Z_RLE))
    # what is left per file in (d): the CRCs, the write, the copy back of one stream
    with tempfile.TemporaryDirectory(prefix='export_bench_') as root:
        crc, wr = [], []
        for k in range(12):
            t0 = time.perf_counter()
            data = P.assemble_png_z(h, w, 16, 2, streams[k % B])
            t1 = time.perf_counter()
            with open(os.path.join(root, '%d.png' % k), 'wb') as f:
                f.write(data)
            t2 = time.perf_counter()
            crc.append((t1 - t0) * 1e3)
            wr.append((t2 - t1) * 1e3)
    pinned = torch.empty(len(streams[0]), dtype=torch.uint8).pin_memory()
    import numpy as np
    zdev = torch.from_numpy(np.frombuffer(streams[0], dtype=np.uint8).copy()).to(dev)
    cp = event_ms(lambda: pinned.copy_(zdev, non_blocking=True), 20)
    res['per_file_ms'] = dict(crc_and_assemble=round(statistics.median(crc), 3), write=round(statistics.median(wr), 3),
                              copy_back=round(statistics.median(cp), 4), tobytes_of_pinned=None)
    t = []
    for _ in range(12):
        t0 = time.perf_counter()
        pinned.numpy().tobytes()
        t.append((time.perf_counter() - t0) * 1e3)
    res['per_file_ms']['tobytes_of_pinned'] = round(statistics.median(t), 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
