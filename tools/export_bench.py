#!/usr/bin/env python3
"""Flow files from the inference graph: the host PNG writers against the device encode path; one JSON line.

    python tools/export_bench.py [--frames 17] [--rounds 3] [--kernel-reps 50]

One process, FlowNetC, B = 4, network 384 x 1280, a clip of --frames uint8 frames of 375 x 1242 with real motion (every frame is
the one before shifted, attenuated, plus noise on a smooth structure — tests/test_sequence_gpu.py::clip), random weights with
the last flow head scaled up so that the flow is not flat.  FlowEstimator(sequence=True).export_sequence writes the clip's
frames - 1 KITTI 16-bit flow PNGs to a temporary directory with

  (a) workers=0            the host writers (filter 0 on every row, zlib level 6, one file after another): the baseline;
  (b) workers=1, 4, 8      unflow_png_filter behind each replay, a writer pool of that many threads, level 6;
  (c) workers=8, level=1

--rounds times each, a round being (a), (b) x 3, (c) in that order, so every figure alternates with the baseline: files per
second of each run (all values, not a mean) and bytes per file (the same flows in every configuration).  Beside them: the
replay of the captured graph per pair, and unflow_png_filter on one replay's B flow maps, by device events (median and
minimum of --kernel-reps), with the bytes it must move (the int16 samples read once, the scanlines written once) and the
rate that gives."""
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
CONFIGS = [('host_w0_l6', 0, 6), ('pool_w1_l6', 1, 6), ('pool_w4_l6', 4, 6), ('pool_w8_l6', 8, 6), ('pool_w8_l1', 8, 1)]


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
    runs = {name: dict(workers=w, level=lv, files_per_s=[], bytes_per_file=None) for name, w, lv in CONFIGS}
    with tempfile.TemporaryDirectory(prefix='export_bench_') as root:
        for r in range(a.rounds):
            for name, w, lv in CONFIGS:
                d = os.path.join(root, '%s_%d' % (name, r))
                t0 = time.perf_counter()
                paths = est.export_sequence(frames, d, fmt='png', workers=w, level=lv)
                dt = time.perf_counter() - t0
                assert len(paths) == n_files
                runs[name]['files_per_s'].append(round(n_files / dt, 3))
                runs[name]['bytes_per_file'] = round(sum(os.path.getsize(p) for p in paths) / n_files)
                print("export_bench: round %d %s %.2f files/s" % (r, name, n_files / dt), file=sys.stderr, flush=True)
    res['configs'] = runs
    base = runs['host_w0_l6']['files_per_s']
    for name, _, _ in CONFIGS[1:]:
        runs[name]['faster_than_host'] = min(runs[name]['files_per_s']) > max(base)      # slowest run against the baseline's fastest
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
    print(json.dumps(res))


if __name__ == '__main__':
    main()
