#!/usr/bin/env python3
"""Throughput of the forward-only estimator (core/inference.FlowEstimator) at the KITTI evaluation shape; one JSON line.

    python tools/inference_bench.py [--iters 20] [--warmup 5] [--rocprof] [--bidirectional] [--visual]

For FlowNetC and CSS at 384 x 1280, B in {1, 4, 8}, math modes bf16x3 and f16: ms per batch of the replayed graph (input
kernel + forward + output kernel, device events around `iters` replays after `warmup`, staging excluded) and pairs/s.  Beside
them: the unsupervised training step (StepRunner, FlowNetC, B = 4, bf16x3) at the same shape, and the device memory of the
estimator against FlowNetEngine(supervised=True) at B = 8.  --rocprof: a separate child run under `rocprofv3 --kernel-trace
--stats` of the two inference kernels alone (B = 8, uint8 KITTI frames, both GT maps) gives their kernel times and the fraction of 8 TB/s
their bytes moved reach.  --bidirectional: also FlowEstimator(..., bidirectional=True) for C and CSS at B in {1, 4, 8}, bf16x3
(both directions, the second output kernel and the occlusion kernel in the graph), and under --rocprof the occlusion kernel's time
and the fraction of 8 TB/s its compulsory bytes reach (two frame-size flows read, two masks written, two GT maps read).
--visual: also FlowEstimator(..., visual=True) for C at B in {1, 4, 8}, bf16x3 (the two visual kernels in the graph), each beside
the plain estimator measured right before it, and under --rocprof the visual kernels' times and the fraction of 8 TB/s their
compulsory bytes reach; --visual-only: nothing but those."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 384, 1280
KITTI = [(375, 1242), (370, 1226), (376, 1241)]
HBM = 8e12


def _estimator(spec, B, math, bidirectional=False, visual=False):
    import torch
    os.environ['UNFLOW_CONV_MATH'] = math
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator(dict(flownet=spec), B, net_size=(H, W), device=torch.device('cuda:0'), bidirectional=bidirectional,
                        **(dict(visual=True) if visual else {}))
    est.engine.init_params(seed=1)
    est._params_changed()
    return est


def _stage_once(est, B):
    """One batch of KITTI-layout uint8 frames through the estimator (stages it, captures the graph)."""
    est.estimate([e[0][:e[2][0], :e[2][1]] for e in _raw(B)], [e[1][:e[2][0], :e[2][1]] for e in _raw(B)])


def _raw(B):
    import numpy as np
    rs = np.random.RandomState(0)
    out = []
    for i in range(B):
        h, w = KITTI[i % 3]
        a = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        out.append((a, np.roll(a, 2, 1), (h, w)))
    return out


def time_replays(est, iters, warmup):
    import torch
    for _ in range(warmup):
        est.graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        est.graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def estimator_case(spec, B, math, iters, warmup, bidirectional=False, visual=False):
    import torch
    est = _estimator(spec, B, math, bidirectional, visual)
    _stage_once(est, B)
    ms = time_replays(est, iters, warmup)
    del est
    torch.cuda.empty_cache()
    out = dict(spec=spec, B=B, math=math, ms_per_batch=round(ms, 4), pairs_per_s=round(B * 1000.0 / ms, 2))
    if bidirectional:
        out['bidirectional'] = True
    if visual:
        out['visual'] = True
    return out


def visual_cases(iters, warmup):
    """C, bf16x3, B in {1, 4, 8}: the plain estimator and the visual one, one after the other in the same process."""
    out = []
    for B in (1, 4, 8):
        plain = estimator_case('C', B, 'bf16x3', iters, warmup)
        vis = estimator_case('C', B, 'bf16x3', iters, warmup, visual=True)
        vis['plain_ms_per_batch'] = plain['ms_per_batch']
        vis['visual_over_plain'] = round(vis['ms_per_batch'] / plain['ms_per_batch'], 4)
        out.append(vis)
    return out


def memory_case():
    import torch
    os.environ['UNFLOW_CONV_MATH'] = 'bf16x3'
    from unflow_amd.core.engine import FlowNetEngine
    from unflow_amd.core.inference import FlowEstimator
    dev = torch.device('cuda:0')
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated(dev)
    est = FlowEstimator(dict(flownet='C'), 8, net_size=(H, W), device=dev)
    torch.cuda.synchronize()
    m_est = torch.cuda.memory_allocated(dev) - m0
    del est
    torch.cuda.empty_cache()
    m0 = torch.cuda.memory_allocated(dev)
    eng = FlowNetEngine(8, H, W, params=dict(flownet='C'), device=dev, seed=None, supervised=True)
    torch.cuda.synchronize()
    m_sup = torch.cuda.memory_allocated(dev) - m0
    del eng
    torch.cuda.empty_cache()
    return dict(estimator_MB=round(m_est / 1e6, 1), supervised_engine_MB=round(m_sup / 1e6, 1),
                ratio=round(m_est / m_sup, 3))


def step_case(iters, warmup):
    import torch
    os.environ['UNFLOW_CONV_MATH'] = 'bf16x3'
    from unflow_amd.core.engine import FlowNetEngine
    from unflow_amd.core.train import StepRunner
    dev = torch.device('cuda:0')
    B = 4
    eng = FlowNetEngine(B, H, W, params=dict(flownet='C', pyramid_loss=True, border_mask=True, ternary_weight=1.0,
                                             smooth_2nd_weight=3.0), device=dev, seed=0)
    run = StepRunner(eng, 1, use_graph=True)
    g = torch.Generator().manual_seed(0)
    im1 = (torch.rand(B, H, W, 3, generator=g) * 255).to(dev)
    im2 = torch.roll(im1, 2, 2)
    for _ in range(warmup):
        run.step(im1, im2, 1e-5)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        run.step(im1, im2, 1e-5)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / iters
    del run, eng
    torch.cuda.empty_cache()
    return dict(spec='C', B=B, math='bf16x3', ms_per_step=round(ms, 3), pairs_per_s=round(B * 1000.0 / ms, 2))


def kernel_bytes(B):
    """Bytes each kernel must move at B, uint8 KITTI frames (what one replay of the bench batch moves)."""
    px_frames = sum(KITTI[i % 3][0] * KITTI[i % 3][1] for i in range(B))
    inp = 2 * px_frames * 3 + 2 * B * H * W * (16 + 3 * 4 * 2)       # frames read; x0 + bf16x3 planes written
    out = B * (H // 4) * (W // 4) * 8 + px_frames * (8 + 6 + 2 * (8 + 4))   # flow2 read; flow + u16 written; 2 GT maps read
    occ = px_frames * (2 * 8 + 2 * 1 + 2 * 4)          # both frame-size flows read; both uint8 masks written; 2 GT masks read
    return inp, out, occ


def visual_kernel_bytes(B):
    """Compulsory bytes of the two visual kernels at B, uint8 KITTI frames, both GT maps (tap re-reads go through the caches
    and are not counted).  frames kernel: both frames, the flow, flow_occ and mask_occ read (the two maxima); the shown frames
    written as float4.  images kernel: the shown frames, the flow, flow_occ and both masks read; five byte images written."""
    px = sum(KITTI[i % 3][0] * KITTI[i % 3][1] for i in range(B))
    return px * (2 * 3 + 8 + 8 + 4 + 2 * 16), px * (2 * 16 + 8 + 8 + 2 * 4 + 5 * 3)


def kernels_only(iters, bidirectional=False, visual=False):
    """The child of --rocprof: the two inference kernels of a B = 8 batch with both GT maps staged, `iters` times each
    (bidirectional: and the occlusion kernel on the two frame-size flows)."""
    import torch
    from unflow_amd import _lib
    from unflow_amd.core.inference import pack_desc
    est = _estimator('C', 8, 'bf16x3', bidirectional, visual)
    desc = pack_desc([KITTI[i % 3] for i in range(8)], 8, staged=(H, W), nmaps=2, u8=True)
    est.desc.copy_(torch.from_numpy(desc))
    est.frames.random_(0, 255)
    est.gt_mask.fill_(1.0)
    torch.cuda.synchronize()
    e = est.engine
    L = _lib.lib()
    f = est.flow_src
    for _ in range(iters):
        _lib.check(L.unflow_inference_input(_lib.ptr(est.frames), _lib.ptr(est.desc), 8, H, W, H, W, _lib.ptr(e.x0), e.mean_host,
                                            _lib.planes_of(est.in_planes), e.stream()), "input")
        _lib.check(L.unflow_inference_output(_lib.ptr(f), f.shape[1], f.shape[2], _lib.cf(20.0), H, W, _lib.ptr(est.desc), 8, H, W,
                                             _lib.ptr(est.out_flow), _lib.ptr(est.out_u16), _lib.ptr(est.gt_flow),
                                             _lib.ptr(est.gt_mask), _lib.ptr(est.partial), _lib.ptr(est.ticket),
                                             _lib.ptr(est.sums), _lib.ptr(est.counts), e.stream()), "output")
        if bidirectional:
            _lib.check(L.unflow_inference_occlusion(_lib.ptr(est.out_flow), _lib.ptr(est.out_flow_bw), _lib.ptr(est.desc), 8, H, W,
                                                    _lib.ptr(est.gt_mask), _lib.ptr(est.occ[0]), _lib.ptr(est.occ[1]),
                                                    _lib.ptr(est.occ_counts), e.stream()), "occlusion")
        if visual:
            _lib.check(L.unflow_inference_visual(_lib.ptr(est.frames), _lib.ptr(est.desc), 8, H, W, H, W, _lib.ptr(est.out_flow),
                                                 _lib.ptr(est.gt_flow), _lib.ptr(est.gt_mask), _lib.ptr(est.vis_shown),
                                                 _lib.ptr(est.vis_max), _lib.ptr(est.vis), None, e.stream()), "visual")
    torch.cuda.synchronize()


def rocprof_case(iters, bidirectional=False, visual=False):
    d = tempfile.mkdtemp(prefix='infprof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--', sys.executable, os.path.abspath(__file__),
           '--kernels-only', '--iters', str(iters)] + (['--bidirectional'] if bidirectional else []) + (['--visual'] if visual else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    if r.returncode != 0:
        return dict(error="rocprofv3 exit %d" % r.returncode, tail=r.stdout.decode(errors='replace')[-400:])
    stats = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not stats:
        return dict(error="no kernel_stats.csv")
    avg = {}
    for row in csv.DictReader(open(stats[0])):
        for k in ('inference_input_kernel', 'inference_output_kernel', 'inference_occlusion_kernel', 'visual_frames_kernel',
                  'visual_images_kernel'):
            if k in row['Name']:
                avg[k] = float(row['AverageNs'])
    bi, bo, bocc = kernel_bytes(8)
    bvf, bvi = visual_kernel_bytes(8)
    out = {}
    for k, b in (('inference_input_kernel', bi), ('inference_output_kernel', bo), ('inference_occlusion_kernel', bocc),
                 ('visual_frames_kernel', bvf), ('visual_images_kernel', bvi)):
        if k in avg:
            out[k] = dict(us=round(avg[k] / 1e3, 2), MB=round(b / 1e6, 2), TBps=round(b / avg[k] / 1e3, 3),
                          frac_of_8TBps=round(b / (avg[k] * 1e-9) / HBM, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rocprof', action='store_true')
    ap.add_argument('--bidirectional', action='store_true', help='also the bidirectional estimator (bf16x3) and its occlusion kernel')
    ap.add_argument('--visual', action='store_true', help='also the visual estimator (C, bf16x3) and its two kernels')
    ap.add_argument('--visual-only', action='store_true', help='only the --visual cases (and, with --rocprof, the kernel times)')
    ap.add_argument('--rocprof-only', action='store_true', help='only the kernel times of the rocprofv3 child run')
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.iters, a.bidirectional, a.visual)
        return
    if a.rocprof_only:
        print(json.dumps(dict(kernels_B8=rocprof_case(a.iters, a.bidirectional, a.visual))))
        return
    if a.visual_only:
        res = dict(metric='inference_ms_per_batch', shape=[H, W], visual=visual_cases(a.iters, a.warmup))
        if a.rocprof:
            res['kernels_B8'] = rocprof_case(a.iters, a.bidirectional, True)
        print(json.dumps(res))
        return
    res = dict(metric='inference_pairs_per_s', shape=[H, W], frames='KITTI uint8 (375x1242, 370x1226, 376x1241)', cases=[])
    for math in ('bf16x3', 'f16'):
        for spec in ('C', 'CSS'):
            for B in (1, 4, 8):
                res['cases'].append(estimator_case(spec, B, math, a.iters, a.warmup))
    if a.bidirectional:
        for spec in ('C', 'CSS'):
            for B in (1, 4, 8):
                res['cases'].append(estimator_case(spec, B, 'bf16x3', a.iters, a.warmup, bidirectional=True))
    if a.visual:
        res['visual'] = visual_cases(a.iters, a.warmup)
    os.environ['UNFLOW_CONV_MATH'] = 'bf16x3'
    res['train_step_unsupervised'] = step_case(a.iters, a.warmup)
    res['memory_B8'] = memory_case()
    if a.rocprof:
        res['kernels_B8'] = rocprof_case(a.iters, a.bidirectional, a.visual)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
