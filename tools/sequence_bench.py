#!/usr/bin/env python3
"""Sequence inference against pair mode at the KITTI evaluation shape; one JSON line.

    python tools/sequence_bench.py [--iters 20] [--warmup 5] [--rocprof] [--bidirectional | --visual | --track | --stabilise | --denoise | --interpolate N [--order K | --held_out] |
                                    --ground_truth [--track]]

For FlowNetC and CSS at 384 x 1280 and B in {1, 4, 8} (bf16x3, 375 x 1242 uint8 frames), in ONE process on one GPU: ms per pair
of the replayed graph of FlowEstimator(..., sequence=True) in its steady state (a carried frame and B new frames: B pairs per
replay) and of the pair-mode estimator (B pairs per replay) — device events around every one of `iters` replays after `warmup`,
staging excluded; mean, standard deviation, minimum and maximum over the replays, and the ratio sequence / pair mode of the
means.  Beside them the device memory of both estimators.  --rocprof: child runs under `rocprofv3 --kernel-trace --stats` give the
times of the two sequence kernels at B = 8 (with the bytes they must move) and, for FlowNetC at B = 4, the kernels of ten
replays of either graph, heaviest first — where the time of a replay goes in each mode.

--bidirectional: the same table for FlowEstimator(..., sequence='bidirectional') against the pair-mode bidirectional
estimator (both directions and the occlusion masks of B pairs per replay either way), the prediction made before the first run
beside it, and — from a child run under rocprofv3 of ten replays of the FlowNetC graph at B = 4 — the time of
unflow_sequence_mirror where it runs, behind conv2, with the bytes it must move.

--visual: FlowNetC at B in {1, 4, 8}, the pair-mode visual estimator, then the sequence visual estimator (and the
sequence estimator without pictures): ms per pair of each replayed graph.  With --rocprof, from one kernel-trace child run per
mode, the picture kernels alone at B = 8 — the last `iters` dispatches of each, with the bytes they must move.

--track: FlowNetC at B = 4, both sequence modes, dense tracks of stride 1: ms per pair of the replayed graph of the
tracking estimator, of the same estimator without tracks, and of the host alternative — the plain graph followed by B image_warp
launches and B adds outside it (no visibility) — the three taken in turn, `--rounds` times, in one process; the flow heads are
scaled down so that the tracks stay alive and the kernel does its whole work in every replay (the share alive is reported).  Beside
them the track kernel alone (device events around 50 launches) with the bytes it must move, and the parent commit's recorded
lines for the same estimators without tracks (profiles/sequence_bench_line.json, profiles/sequence_bidir_bench_line.json).

--interpolate N: FlowNetC at B = 4, both sequence modes, N in-between frames per pair: ms per pair of the replayed
graph of the interpolating estimator against the same run's estimator without the option (the two take turns), and alone — device
events around 50 launches — unflow_sequence_interpolate and the replay's output kernels (unflow_inference_output, with both
directions twice and unflow_inference_occlusion), with the atomic bytes the splat issues.  Recorded, one line per N, in
profiles/sequence_interpolate_bench_line.json.

--interpolate N --order K: the estimator with the consistency-ordered splat against the SAME RUN's unordered
interpolating estimator, the two taking turns; and the two entries alone on one set of buffers (device events around 50 launches),
taking turns as well.  One line per N in profiles/sequence_interpolate_order_bench_line.json.

--interpolate N --held_out: the estimator that also scores its in-between frames against held-out frames, against
the SAME RUN's interpolating estimator without the option, the two taking turns; and unflow_sequence_interpolate_score alone (device
events around 50 back-to-back calls) beside the bytes it reads.  One line per N in profiles/sequence_mid_score_bench_line.json.

--ground_truth [--track]: FlowNetC at B = 4, both sequence modes: ms per pair of the replayed graph of the scoring
estimator (two-map ground truth staged, every pair scored; with --track dense tracks of stride 1 and unflow_sequence_track_score)
against the SAME RUN's estimator without ground_truth (with --track: the plain tracking estimator), the two taking turns; with
--track the new kernel alone (device events around 50 launches) with the bytes it must move; and the wall time per pair of
evaluate_sequence against pair-mode evaluate on the same synthetic clip from host arrays.  Recorded in
profiles/sequence_gt_bench_line.json.

--stabilise: FlowNetC at B = 4, both sequence modes: ms per pair of the replayed graph of the stabilising estimator
(the defaults: tol 2, iters 3, follow 0) against the SAME RUN's plain estimator, the two taking turns; and
unflow_sequence_stabilise alone (device events around 50 calls, nine launches each) with the bytes it must move.  One line per mode
in profiles/sequence_stabilise_bench_line.json.

--denoise: FlowNetC at B = 4, sequence='bidirectional': ms per pair of the replayed graph of the denoising estimator
(the defaults: tol 'auto', depth 8) against the SAME RUN's plain bidirectional estimator, the two taking turns; and
unflow_sequence_denoise alone (device events around 50 calls, 2 B + 2 launches each) with the bytes it must move and the HBM
bandwidth they imply.  One line in profiles/sequence_denoise_bench_line.json."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 384, 1280
FRAME = (375, 1242)


def _frames(n):
    import numpy as np
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, size=FRAME + (3,)).astype(np.uint8)
    return [np.roll(a, 2 * i, 1) for i in range(n)]


def _estimator(spec, B, sequence, bidirectional=False, visual=False, track=False, head_scale=None, interpolate=None,
               ground_truth=False, held_out=False, interpolate_order=None, stabilise=None, denoise=None):
    """sequence: False, True or 'bidirectional'; bidirectional: the pair-mode estimator of both directions; visual: with the
    pictures at the end of the graph; track: FlowEstimator's; head_scale: the flow heads' weights times this."""
    import torch
    os.environ['UNFLOW_CONV_MATH'] = 'bf16x3'
    from unflow_amd.core.inference import FlowEstimator
    import gc
    dev = torch.device('cuda:0')
    gc.collect()                               # an earlier case's estimator is freed now, not inside this measurement
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated(dev)
    kw = dict(visual='sequence' if sequence else True) if visual else {}
    if track is not False:
        kw['track'] = track
    if interpolate:
        kw['interpolate'] = interpolate
    if interpolate_order:
        kw['interpolate_order'] = interpolate_order
    if ground_truth:
        kw['ground_truth'] = True
    if held_out:
        kw['held_out'] = True
    if stabilise:
        kw['stabilise'] = stabilise
    if denoise:
        kw['denoise'] = denoise
    est = FlowEstimator(dict(flownet=spec), B, net_size=(H, W), device=dev, sequence=sequence, bidirectional=bidirectional, **kw)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated(dev) - m0
    tfp = est.engine.init_params(seed=1)
    if head_scale is not None:
        est.load_tf_params({k: (v * head_scale if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                            for k, v in tfp.items()})
    est._params_changed()
    fr = _frames(3 * B + 1)
    if sequence == 'bidirectional':
        est.estimate_sequence_bidirectional(fr[:3 * B])
    elif sequence:
        est.estimate_sequence(fr[:3 * B])      # the last replay: a carried frame and B new ones, every pair slot valid
    elif bidirectional:
        est.estimate_bidirectional(fr[:B], fr[1:B + 1])
    else:
        est.estimate(fr[:B], fr[1:B + 1])
    return est, mem


def time_replays(est, iters, warmup):
    """ms of each of `iters` replays (device events between consecutive replays)."""
    import torch
    for _ in range(warmup):
        est.graph.replay()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        est.graph.replay()
        ev[i + 1].record()
    ev[-1].synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]


def _stats(ms, B):
    return dict(ms_per_pair=round(statistics.mean(ms) / B, 4), std=round(statistics.pstdev(ms) / B, 4),
                min=round(min(ms) / B, 4), max=round(max(ms) / B, 4))


def case(spec, B, iters, warmup, bidirectional=False):
    import gc
    import torch
    out = dict(spec=spec, B=B)
    for name, seq in (('pair', False), ('sequence', 'bidirectional' if bidirectional else True)):
        est, mem = _estimator(spec, B, seq, bidirectional and not seq)
        out[name] = _stats(time_replays(est, iters, warmup), B)
        out[name]['estimator_MB'] = round(mem / 1e6, 1)
        del est
        gc.collect()
        torch.cuda.empty_cache()
    out['sequence_over_pair'] = round(out['sequence']['ms_per_pair'] / out['pair']['ms_per_pair'], 4)
    return out


# ------------------------------------------------------------------------------------------------- rocprofv3 children
def kernels_only(iters):
    """Child: the two sequence kernels of a FlowNetC estimator at B = 8, `iters` times each (carry source B)."""
    import torch
    est, _ = _estimator('C', 8, True)
    e = est.engine
    for _ in range(iters):
        e.sequence_carry(est.tab[16 * 8:])
        e.sequence_input(est.frames, est.tab, est.Hmax, est.Wmax)
    torch.cuda.synchronize()


def graph_only(sequence, iters, bidirectional=False):
    """Child: `iters` replays of the FlowNetC graph at B = 4 in one mode."""
    import torch
    est, _ = _estimator('C', 4, sequence, bidirectional)
    for _ in range(iters):
        est.graph.replay()
    torch.cuda.synchronize()


def _rocprof(args):
    d = tempfile.mkdtemp(prefix='seqprof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--', sys.executable,
           os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    if r.returncode != 0:
        return None, dict(error="rocprofv3 exit %d" % r.returncode, tail=r.stdout.decode(errors='replace')[-400:])
    stats = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not stats:
        return None, dict(error="no kernel_stats.csv")
    return list(csv.DictReader(open(stats[0]))), None


def carry_bytes(B=8):
    """Bytes unflow_sequence_carry reads plus writes for FlowNetC at (H, W), bf16x3: one row of x0, of c3 and of the conv2
    segment of cat2, fp32 and three planes each (x0: fp32 only)."""
    x0 = H * W * 16
    c3 = (H // 8) * (W // 8) * 256 * (4 + 3 * 2)
    cat2 = (H // 4) * (W // 4) * 128 * (4 + 3 * 2)
    return 2 * (x0 + c3 + cat2)


def mirror_bytes(B=4):
    """Bytes unflow_sequence_mirror reads plus writes for FlowNetC at (H, W), bf16x3: B rows of the conv2 segment of cat2, fp32
    and three planes."""
    return 2 * B * (H // 4) * (W // 4) * 128 * (4 + 3 * 2)


def mirror_case(iters=10):
    """The mirror kernel inside the replayed FlowNetC graph at B = 4 (a rocprofv3 child run)."""
    rows, err = _rocprof(['--graph-only', 'bidir', '--iters', str(iters)])
    if err:
        return err
    for row in rows:
        if 'sequence_mirror_kernel' in row['Name']:
            ns, nbytes = float(row['AverageNs']), mirror_bytes(4)
            return dict(B=4, calls=int(row['Calls']), us=round(ns / 1e3, 2), MB=round(nbytes / 1e6, 2),
                        TBps=round(nbytes / ns / 1e3, 3), where='inside the replayed graph, behind conv2')
    return dict(error='no sequence_mirror_kernel in the trace')


def input_bytes(B=8):
    """Bytes unflow_inference_input_frames must move: B uint8 frames read, B rows of x0 and of its three planes written."""
    return B * FRAME[0] * FRAME[1] * 3 + B * H * W * (16 + 3 * 4 * 2)


def rocprof_cases(iters):
    out = {}
    rows, err = _rocprof(['--kernels-only', '--iters', str(iters)])
    if err:
        out['kernels_B8'] = err
    else:
        k = {}
        for name, nbytes in (('sequence_carry_kernel', carry_bytes()), ('inference_input_frames_kernel', input_bytes())):
            for row in rows:
                if name in row['Name']:
                    ns = float(row['AverageNs'])
                    k[name] = dict(us=round(ns / 1e3, 2), MB=round(nbytes / 1e6, 2), TBps=round(nbytes / ns / 1e3, 3))
        out['kernels_B8'] = k
    for mode in ('pair', 'sequence'):
        rows, err = _rocprof(['--graph-only', mode, '--iters', '10'])
        if err:
            out['graph_C_B4_' + mode] = err
            continue
        rows.sort(key=lambda r: -float(r['TotalDurationNs']))
        total = sum(float(r['TotalDurationNs']) for r in rows)
        out['graph_C_B4_' + mode] = dict(
            note='whole child run: 10 timed replays plus set-up (one eager pass, the capture pass, two replays)',
            total_ms=round(total / 1e6, 3),
            top=[dict(kernel=r['Name'][:72], calls=int(r['Calls']), total_ms=round(float(r['TotalDurationNs']) / 1e6, 3),
                      avg_us=round(float(r['AverageNs']) / 1e3, 2)) for r in rows[:14]])
    return out


# ------------------------------------------------------------------------------------------------- --visual
def visual_case(B, iters, warmup):
    """FlowNetC at B: ms per pair of the pair-mode visual estimator, then of the sequence visual estimator (and of the sequence
    estimator without pictures, for what the pictures add), each in its steady state."""
    import gc
    import torch
    out = dict(spec='C', B=B)
    for name, seq, vis in (('pair_visual', False, True), ('sequence_visual', True, True), ('sequence', True, False)):
        est, mem = _estimator('C', B, seq, visual=vis)
        out[name] = _stats(time_replays(est, iters, warmup), B)
        out[name]['estimator_MB'] = round(mem / 1e6, 1)
        del est
        gc.collect()
        torch.cuda.empty_cache()
    out['sequence_visual_over_pair_visual'] = round(out['sequence_visual']['ms_per_pair'] / out['pair_visual']['ms_per_pair'], 4)
    out['pictures_ms_per_pair_in_sequence'] = round(out['sequence_visual']['ms_per_pair'] - out['sequence']['ms_per_pair'], 4)
    return out


def visual_kernels_only(mode, iters, B=8):
    """Child: the picture launches alone on a set-up FlowNetC visual estimator at B = 8, `iters` times — unflow_inference_visual
    ('pair') or unflow_sequence_visual ('sequence': carry source B, every frame and pair slot valid)."""
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    est, _ = _estimator('C', B, mode == 'sequence', visual=True)
    L, st = _lib.lib(), est.engine.stream()
    torch.cuda.synchronize()
    for _ in range(iters):
        if mode == 'sequence':
            check(L.unflow_sequence_visual(ptr(est.frames), ptr(est.tab), B, est.Hmax, est.Wmax, H, W, ptr(est.out_flow), None, None,
                                           ptr(est.vis_shown), ptr(est.vis_max), ptr(est.vis), None, st), "sequence_visual")
        else:
            check(L.unflow_inference_visual(ptr(est.frames), ptr(est.desc), B, est.Hmax, est.Wmax, H, W, ptr(est.out_flow),
                                            ptr(est.gt_flow), ptr(est.gt_mask), ptr(est.vis_shown), ptr(est.vis_max), ptr(est.vis),
                                            None, st), "inference_visual")
    torch.cuda.synchronize()


def _last_dispatches(d, names, iters):
    """Mean duration in ns of the LAST `iters` dispatches of every kernel in `names` (the child's own loop; what its set-up ran
    before is left out), from the kernel trace of a rocprofv3 run in folder d; None when the trace cannot be read."""
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        return None
    rows = list(csv.DictReader(open(files[0])))
    if not rows or not {'Kernel_Name', 'Start_Timestamp', 'End_Timestamp'} <= set(rows[0]):
        return None
    out = {}
    for name in names:
        mine = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in rows
                      if name in r['Kernel_Name'] and ('sequence_' + name) not in r['Kernel_Name'])
        if len(mine) >= iters:
            out[name] = sum(e - s for s, e in mine[-iters:]) / float(iters)
    return out


def visual_bytes(B=8):
    """Compulsory bytes per kernel at B (uint8 frames of FRAME, no ground truth; tap re-reads go through the caches): per frame
    pixel — pair frames kernel 6 (two frames) + 8 (flow) read, 32 (two float4 frames) written; sequence frames kernel 3 + 8 read,
    16 written; either images kernel 32 + 8 read, 9 (three byte images) written; the carry 16 + 16 per pixel of ONE (H, W)
    staging row per replay."""
    px = FRAME[0] * FRAME[1]
    return {'visual_frames_kernel': (46, B * px * 46), 'visual_images_kernel': (49, B * px * 49),
            'sequence_visual_frames_kernel': (27, B * px * 27), 'sequence_visual_images_kernel': (49, B * px * 49),
            'sequence_carry_kernel': (32, H * W * 32)}


def visual_rocprof(iters, B=8):
    """Per-kernel times of the picture launches at B = 8, pair mode and sequence mode, one counters-free kernel-trace child each."""
    nbytes = visual_bytes(B)
    out = {}
    for mode, names in (('pair', ('visual_frames_kernel', 'visual_images_kernel')),
                        ('sequence', ('sequence_carry_kernel', 'sequence_visual_frames_kernel', 'sequence_visual_images_kernel'))):
        d = tempfile.mkdtemp(prefix='seqvisprof_')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--', sys.executable,
               os.path.abspath(__file__), '--visual-kernels-only', mode, '--iters', str(iters)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if r.returncode != 0:
            out[mode] = dict(error="rocprofv3 exit %d" % r.returncode, tail=r.stdout.decode(errors='replace')[-400:])
            continue
        ns = _last_dispatches(d, names, iters)
        if ns is None:
            out[mode] = dict(error="no readable kernel trace")
            continue
        k = {n: dict(us=round(ns[n] / 1e3, 2), B_per_px=nbytes[n][0], MB=round(nbytes[n][1] / 1e6, 2),
                     TBps=round(nbytes[n][1] / ns[n] / 1e3, 3)) for n in names if n in ns}
        k['total_us'] = round(sum(v['us'] for v in k.values()), 2)
        out[mode] = k
    return out


# ------------------------------------------------------------------------------------------------- --track
TRACK_HEAD_SCALE = 0.01          # flows of a few hundredths of a pixel: every track but the border's stays alive


def track_bytes(B=4, occ=False):
    """Compulsory bytes of unflow_sequence_track per replay, dense stride 1 on FRAME: per track the state read and written (9 + 9),
    and per pair the flow map read once (8; tap re-reads go through the caches), the mask with both directions (1) and the
    outputs written (9)."""
    px = FRAME[0] * FRAME[1]
    per = 18 + B * (8 + 9 + (1 if occ else 0))
    return per, px * per


def _host_chain(est, disp):
    """The alternative without the kernel: B image_warp launches and B adds behind the replay, outside the graph, on the whole
    buffers (no crop to the frame, no visibility)."""
    from unflow_amd.core.image_warp import image_warp
    for i in range(est.B):
        disp = disp + image_warp(est.out_flow[i:i + 1], disp)
    return disp


def _time(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    ev[-1].synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]


def _recorded(path, B=4):
    """ms per pair of the FlowNetC sequence estimator at B in a recorded bench line of profiles/, or None."""
    try:
        with open(os.path.join(ROOT, 'profiles', path)) as f:
            line = json.loads(f.read().strip().splitlines()[-1])
        return [c['sequence']['ms_per_pair'] for c in line['cases'] if c['spec'] == 'C' and c['B'] == B][0]
    except (OSError, ValueError, KeyError, IndexError):
        return None


def track_case(seq, iters, warmup, rounds, B=4):
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    plain, _ = _estimator('C', B, seq, head_scale=TRACK_HEAD_SCALE)
    tracked, mem = _estimator('C', B, seq, track=True, head_scale=TRACK_HEAD_SCALE)
    tracked.track_sequence(_frames(3 * B))                 # the tables of the last replay: a carried frame, B pairs, S = 1, N
    disp0 = torch.zeros(1, plain.Hmax, plain.Wmax, 2, device=plain.dev)

    def host():
        plain.graph.replay()
        _host_chain(plain, disp0)
    runs = {'plain': plain.graph.replay, 'track': tracked.graph.replay, 'host_chain': host}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # the three in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence=seq if seq is True else str(seq), tracks=FRAME[0] * FRAME[1], rounds=rounds)
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['track']['estimator_MB'] = round(mem / 1e6, 1)
    out['track_over_plain'] = round(out['track']['ms_per_pair'] / out['plain']['ms_per_pair'], 4)
    out['host_chain_over_plain'] = round(out['host_chain']['ms_per_pair'] / out['plain']['ms_per_pair'], 4)
    out['track_added_us_per_replay'] = round((out['track']['ms_per_pair'] - out['plain']['ms_per_pair']) * B * 1e3, 2)
    out['host_chain_added_us_per_replay'] = round((out['host_chain']['ms_per_pair'] - out['plain']['ms_per_pair']) * B * 1e3, 2)
    # the kernel alone: 50 launches between two events (its launch gaps included), the tables of the last replay
    L, e = _lib.lib(), tracked

    def kernel():
        check(L.unflow_sequence_track(ptr(e.out_flow), ptr(e.occ[0]) if e.seq_bidir else None, ptr(e.tab), B, e.Hmax, e.Wmax,
                                      ptr(e.track_anchors), e.track_cap, ptr(e.track_disp), ptr(e.track_alive),
                                      ptr(e.out_track_disp), ptr(e.out_track_alive), e.engine.stream()), "sequence_track")
    with torch.cuda.device(e.dev):
        for _ in range(10):
            kernel()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            kernel()
        b.record()
        b.synchronize()
    us = a.elapsed_time(b) * 1e3 / 50
    per, nbytes = track_bytes(B, e.seq_bidir)
    out['kernel'] = dict(us=round(us, 2), B_per_track=per, MB=round(nbytes / 1e6, 2), TBps=round(nbytes / us / 1e6, 3),
                         how='device events around 50 back-to-back launches, launch gaps included')
    out['alive_share'] = round(float(e.track_alive[:FRAME[0] * FRAME[1]].float().mean().item()), 4)
    out['parent_recorded_ms_per_pair'] = _recorded('sequence_bidir_bench_line.json' if e.seq_bidir else 'sequence_bench_line.json', B)
    del plain, tracked
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------- --interpolate
def _launches_us(fn, dev, n=50, warm=10):
    """us per call of fn: device events around n back-to-back calls, launch gaps included."""
    import torch
    with torch.cuda.device(dev):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def interpolate_case(seq, n, iters, warmup, rounds, B=4):
    import gc
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    plain, _ = _estimator('C', B, seq)
    mid, mem = _estimator('C', B, seq, interpolate=n)
    mid.interpolate_sequence(_frames(3 * B))               # the tables of the last replay: a carried frame, B pairs
    runs = {'plain': plain.graph.replay, 'interpolate': mid.graph.replay}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence=seq if seq is True else str(seq), n=n, rounds=rounds)
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['interpolate']['estimator_MB'] = round(mem / 1e6, 1)
    out['interpolate_over_plain'] = round(out['interpolate']['ms_per_pair'] / out['plain']['ms_per_pair'], 4)
    out['interpolate_added_us_per_replay'] = round((out['interpolate']['ms_per_pair'] - out['plain']['ms_per_pair']) * B * 1e3, 2)
    L, e = _lib.lib(), mid
    bw, ofw, obw = (e.out_flow_bw, e.occ[0], e.occ[1]) if e.seq_bidir else (None, None, None)

    def kernel():
        check(L.unflow_sequence_interpolate(ptr(e.frames), ptr(e.tab), B, e.Hmax, e.Wmax, n, ptr(e.out_flow), ptr(bw), ptr(ofw),
                                            ptr(obw), ptr(e.mid_prev), ptr(e.mid_sums), ptr(e.out_mid), ptr(e.out_mid_holes),
                                            e.engine.stream()), "sequence_interpolate")

    def outputs():
        pairs = e.tab[8 * B:]
        if e.seq_bidir:
            fw_rows, bw_rows = e.engine.fw_bw(e.flow_src)
            e._output(fw_rows, pairs, e.out_flow, e.out_u16)
            e._output(bw_rows, pairs, e.out_flow_bw, e.out_u16_bw)
            e._occlusion(pairs)
        else:
            e._output(e.flow_src, pairs, e.out_flow, e.out_u16)
    us, us_out = _launches_us(kernel, e.dev), _launches_us(outputs, e.dev)
    px, dirs = FRAME[0] * FRAME[1] * B, 2 if e.seq_bidir else 1
    atomic_bytes = px * n * dirs * 128                     # 4 targets x 4 sums x 8 bytes per source pixel, j and direction, at most
    out['kernel'] = dict(us=round(us, 2), launches=3, atomic_MB=round(atomic_bytes / 1e6, 1),
                         atomic_TBps_if_all_of_it=round(atomic_bytes / us / 1e6, 3),
                         how='device events around 50 back-to-back calls of the entry (three launches each), launch gaps included')
    out['output_kernels'] = dict(us=round(us_out, 2), how='the same, unflow_inference_output (x 2 and unflow_inference_occlusion with '
                                                          'both directions)')
    out['kernel_over_output_kernels'] = round(us / us_out, 3)
    out['holes_share'] = round(float(e.out_mid_holes.float().sum().item()) / (px * n), 5)
    del plain, mid
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------- --interpolate N --order K (7.19)
def order_case(seq, n, order, iters, warmup, rounds, B=4):
    """The ordered estimator against the SAME RUN's unordered interpolating estimator, the two taking turns; and the two entries
    alone on the ordered estimator's buffers, taking turns as well."""
    import gc
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    mid, _ = _estimator('C', B, seq, interpolate=n)
    mid.interpolate_sequence(_frames(3 * B))               # the tables of the last replay: a carried frame, B pairs
    ordered, mem = _estimator('C', B, seq, interpolate=n, interpolate_order=order)
    ordered.interpolate_sequence(_frames(3 * B))
    runs = {'interpolate': mid.graph.replay, 'ordered': ordered.graph.replay}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence=seq if seq is True else str(seq), n=n, order=order, rounds=rounds)
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['ordered']['estimator_MB'] = round(mem / 1e6, 1)
    out['ordered_over_interpolate'] = round(out['ordered']['ms_per_pair'] / out['interpolate']['ms_per_pair'], 4)
    out['ordered_added_us_per_replay'] = round((out['ordered']['ms_per_pair'] - out['interpolate']['ms_per_pair']) * B * 1e3, 2)
    L, e = _lib.lib(), ordered
    bw, ofw, obw = (e.out_flow_bw, e.occ[0], e.occ[1]) if e.seq_bidir else (None, None, None)
    args = (ptr(e.frames), ptr(e.tab), B, e.Hmax, e.Wmax, n, ptr(e.out_flow), ptr(bw), ptr(ofw), ptr(obw), ptr(e.mid_prev),
            ptr(e.mid_sums), ptr(e.out_mid), ptr(e.out_mid_holes))
    entries = {'interpolate': lambda: check(L.unflow_sequence_interpolate(*args, e.engine.stream()), "sequence_interpolate"),
               'ordered': lambda: check(L.unflow_sequence_interpolate_ordered(*args, order, e.engine.stream()),
                                        "sequence_interpolate_ordered")}
    us = {k: [] for k in entries}
    for _ in range(rounds):
        for k, fn in entries.items():
            us[k].append(_launches_us(fn, e.dev))
    px, dirs = FRAME[0] * FRAME[1] * B, 2 if e.seq_bidir else 1
    atomic_bytes = px * n * dirs * 128                     # 4 targets x 4 sums x 8 bytes per source pixel, j and direction, at most
    out['kernel'] = {k: dict(us=round(statistics.mean(v), 2), rounds_us=[round(x, 2) for x in v],
                             atomic_TBps_if_all_of_it=round(atomic_bytes / statistics.mean(v) / 1e6, 3)) for k, v in us.items()}
    out['kernel']['atomic_MB'] = round(atomic_bytes / 1e6, 1)
    out['kernel']['how'] = 'device events around 50 back-to-back calls of either entry (three launches each), launch gaps included'
    out['kernel']['ordered_over_interpolate'] = round(statistics.mean(us['ordered']) / statistics.mean(us['interpolate']), 4)
    entries['ordered']()                                   # the outputs of the ordered entry, for the hole share
    out['holes_share'] = round(float(e.out_mid_holes.float().sum().item()) / (px * n), 5)
    assert not bool(e.mid_sums.any())
    del mid, ordered
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------- --interpolate N --held_out (7.18)
def held_out_case(seq, n, iters, warmup, rounds, B=4):
    """The scoring estimator against the SAME RUN's interpolating estimator without the option, the two taking turns; and the
    new entry alone, with the bytes it has to read."""
    import gc
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    mid, _ = _estimator('C', B, seq, interpolate=n)
    mid.interpolate_sequence(_frames(3 * B))
    held, mem = _estimator('C', B, seq, interpolate=n, held_out=True)
    scores = held.evaluate_interpolation([_frames((3 * B - 1) * (n + 1) + 1)])      # the last replay: a carried frame, B held pairs
    runs = {'interpolate': mid.graph.replay, 'held_out': held.graph.replay}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence=seq if seq is True else str(seq), n=n, rounds=rounds)
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['held_out']['estimator_MB'] = round(mem / 1e6, 1)
    out['held_out_over_interpolate'] = round(out['held_out']['ms_per_pair'] / out['interpolate']['ms_per_pair'], 4)
    out['held_out_added_us_per_replay'] = round((out['held_out']['ms_per_pair'] - out['interpolate']['ms_per_pair']) * B * 1e3, 2)
    L, e = _lib.lib(), held

    def kernel():
        check(L.unflow_sequence_interpolate_score(ptr(e.frames), ptr(e.tab), B, e.Hmax, e.Wmax, n, ptr(e.out_mid), ptr(e.mid_truth),
                                                  ptr(e.mid_score_prev), ptr(e.mid_score_ws), ptr(e.out_mid_sse),
                                                  ptr(e.out_mid_ssim), e.engine.stream()), "sequence_interpolate_score")
    us = _launches_us(kernel, e.dev)
    px = FRAME[0] * FRAME[1] * B
    # uint8 frames: per pixel the two frames' 3 bytes once per slot, truth and out_mid 3 bytes each per j; the 39 x 23 halo region
    # of a 32 x 16 tile reads 1.75 times the tile's own pixels
    own = px * (6 + 6 * n)
    out['kernel'] = dict(us=round(us, 2), launches=2, own_MB=round(own / 1e6, 2), with_halo_MB=round(own * 39 * 23 / 512 / 1e6, 2),
                         own_TBps=round(own / us / 1e6, 4), with_halo_TBps=round(own * 39 * 23 / 512 / us / 1e6, 4),
                         how='device events around 50 back-to-back calls of the entry (two launches each), launch gaps included')
    out['scores'] = {k: round(v, 4) for k, v in scores.items() if k.startswith(('psnr/', 'ssim/'))}
    out['holes_share'] = round(scores['holes'], 5)
    assert not bool(e.mid_score_ws.any())
    del mid, held
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------- --ground_truth
def _clip_gts(n):
    """A two-map ground truth per pair at FRAME: a flow of a hundredth of a pixel and masks of ones, so that every ground-truth
    track stays alive and the scoring kernel does its whole work in every replay."""
    import numpy as np
    flow = np.full(FRAME + (2,), 0.01, np.float32)
    ones = np.ones(FRAME, np.float32)
    return [(flow, ones, flow, ones)] * n


def track_score_bytes(B=4):
    """Compulsory bytes of unflow_sequence_track_score per replay, dense stride 1 on FRAME: per track the state read and written
    (9 + 9) and per pair the ground-truth flow and mask read once (8 + 4; tap re-reads go through the caches), the predicted track
    read (9) and the ground-truth track written (9)."""
    px = FRAME[0] * FRAME[1]
    per = 18 + B * 30
    return per, px * per


def gt_case(seq, track, iters, warmup, rounds, B=4):
    import gc
    import time
    import numpy as np
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    from unflow_amd.core.input import resize_image_with_crop_or_pad
    tr = True if track else False
    plain, _ = _estimator('C', B, seq, track=tr, head_scale=TRACK_HEAD_SCALE)
    scored, mem = _estimator('C', B, seq, track=tr, head_scale=TRACK_HEAD_SCALE, ground_truth=True)
    frames = _frames(3 * B + 1)
    gts = _clip_gts(3 * B)
    if track:
        plain.track_sequence(frames[:3 * B])               # the tables of the last replay: a carried frame, B pairs, S = 1, N
    res = scored.evaluate_sequence([(frames[:3 * B], gts[:3 * B - 1])])       # ... and their nmaps words, the maps staged
    runs = {'plain': plain.graph.replay, 'ground_truth': scored.graph.replay}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence=seq if seq is True else str(seq), track=bool(track), rounds=rounds)
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['ground_truth']['estimator_MB'] = round(mem / 1e6, 1)
    out['ground_truth_over_plain'] = round(out['ground_truth']['ms_per_pair'] / out['plain']['ms_per_pair'], 4)
    out['ground_truth_added_us_per_replay'] = round((out['ground_truth']['ms_per_pair'] - out['plain']['ms_per_pair']) * B * 1e3, 2)
    if track:
        L, e = _lib.lib(), scored

        def kernel():
            check(L.unflow_sequence_track_score(ptr(e.gt_flow), ptr(e.gt_mask), ptr(e.tab), B, e.Hmax, e.Wmax, ptr(e.track_anchors),
                                                e.track_cap, ptr(e.out_track_disp), ptr(e.out_track_alive), ptr(e.gt_track_disp),
                                                ptr(e.gt_track_alive), ptr(e.out_gt_track_disp), ptr(e.out_gt_track_alive),
                                                ptr(e.out_track_scores), ptr(e.out_track_err), ptr(e.track_score_ws),
                                                e.engine.stream()), "sequence_track_score")
        us = _launches_us(kernel, e.dev)
        per, nbytes = track_score_bytes(B)
        out['kernel'] = dict(us=round(us, 2), B_per_track=per, MB=round(nbytes / 1e6, 2), TBps=round(nbytes / us / 1e6, 3),
                             how='device events around 50 back-to-back launches, launch gaps included')
        out['gt_alive_share'] = round(float(e.gt_track_alive[:FRAME[0] * FRAME[1]].float().mean().item()), 4)
        out['track_scores_last_pair'] = [int(v) for v in e.out_track_scores[B - 1].cpu()]
    # evaluate_sequence against pair-mode evaluate on the same clip from host arrays: wall time per pair, the second of two passes
    n_pairs = 3 * B
    pair, _ = _estimator('C', B, False, bidirectional=seq == 'bidirectional', head_scale=TRACK_HEAD_SCALE)
    pad = lambda a: resize_image_with_crop_or_pad(a, H, W).reshape((H, W) + a.shape[2:])         # noqa: E731
    fp = [pad(f.astype(np.float32)) for f in frames]
    gp = [tuple(pad(a if a.ndim == 3 else a[..., None]) for a in g) for g in gts]
    shape = np.asarray(FRAME + (3,), np.int32)
    batches = [tuple(np.stack(c) for c in zip(*[(fp[i], fp[i + 1], shape) + gp[i] for i in range(b0, min(b0 + B, n_pairs))]))
               for b0 in range(0, n_pairs, B)]
    wall = {}
    for name, fn in (('evaluate_sequence', lambda: scored.evaluate_sequence([(frames, gts)])),
                     ('pair_evaluate', lambda: pair.evaluate(iter(batches)))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        wall[name] = dict(ms_per_pair=round((time.perf_counter() - t0) * 1e3 / n_pairs, 3), pairs=r['num_examples'])
    wall['evaluate_sequence_over_pair_evaluate'] = round(wall['evaluate_sequence']['ms_per_pair'] / wall['pair_evaluate']['ms_per_pair'], 4)
    out['wall'] = wall
    out['names'] = res['names']
    del plain, scored, pair
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------- --stabilise
def stabilise_bytes(iters, B=4):
    """Compulsory bytes of unflow_sequence_stabilise per replay on FRAME: the flow (8 bytes per pixel) is read iters + 2 times — once
    per fit and once for the residual map — the uint8 frame (3 bytes) once, and four bytes are written per pixel."""
    return FRAME[0] * FRAME[1] * B * (8 * (iters + 2) + 3 + 4)


def stabilise_kernels_only(mode, iters, B=4):
    """Child: unflow_sequence_stabilise alone on a set-up FlowNetC estimator, `iters` times (carry source B, every pair valid)."""
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    e, _ = _estimator('C', B, 'bidirectional' if mode == 'bidir' else True, stabilise=True)
    e.stabilise_sequence(_frames(3 * B))
    L, o = _lib.lib(), e.stabilise
    torch.cuda.synchronize()
    for _ in range(iters):
        check(L.unflow_sequence_stabilise(ptr(e.frames), ptr(e.tab), B, e.Hmax, e.Wmax, ptr(e.out_flow),
                                          ptr(e.occ[0]) if e.seq_bidir else None, o['tol'], o['iters'], o['follow'], ptr(e.stab_path),
                                          ptr(e.stab_ws), ptr(e.out_stab_motion), ptr(e.out_stab_path), ptr(e.out_stab_resid),
                                          ptr(e.out_stab), ptr(e.out_stab_counts), e.engine.stream()), "sequence_stabilise")
    torch.cuda.synchronize()


def stabilise_rocprof(seq, iters=50):
    """Per-kernel times of the entry from a counters-free kernel-trace child: {kernel: calls, mean us}, and the sum of one entry's
    nine launches (the estimator's own few replays are in the means too)."""
    rows, err = _rocprof(['--stabilise-kernels-only', 'bidir' if seq == 'bidirectional' else 'fw', '--iters', str(iters)])
    if err:
        return err
    out, R = {}, 3
    per_entry = {'st_accumulate_kernel': R + 1, 'st_solve_kernel': R + 1, 'st_apply_kernel': 1}
    for row in rows:
        for name in per_entry:
            if name in row['Name']:
                out[name] = dict(calls=int(row['Calls']), us=round(float(row['AverageNs']) / 1e3, 2))
    if len(out) == len(per_entry):
        out['kernels_us_per_entry'] = round(sum(out[n]['us'] * k for n, k in per_entry.items()), 2)
    return out


def stabilise_case(seq, iters, warmup, rounds, B=4, rocprof=False):
    """The stabilising estimator (defaults: tol 2, iters 3, follow 0) against the SAME RUN's plain estimator, the two taking turns;
    and the new entry alone, with the bytes it has to move."""
    import gc
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    plain, _ = _estimator('C', B, seq)
    stab, mem = _estimator('C', B, seq, stabilise=True)
    stab.stabilise_sequence(_frames(3 * B))                # the tables of the last replay: a carried frame, B pairs
    runs = {'plain': plain.graph.replay, 'stabilise': stab.graph.replay}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence=seq if seq is True else str(seq), rounds=rounds, options=dict(stab.stabilise))
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['stabilise']['estimator_MB'] = round(mem / 1e6, 1)
    out['stabilise_over_plain'] = round(out['stabilise']['ms_per_pair'] / out['plain']['ms_per_pair'], 4)
    out['stabilise_added_us_per_replay'] = round((out['stabilise']['ms_per_pair'] - out['plain']['ms_per_pair']) * B * 1e3, 2)
    L, e, o = _lib.lib(), stab, stab.stabilise

    def kernel():
        check(L.unflow_sequence_stabilise(ptr(e.frames), ptr(e.tab), B, e.Hmax, e.Wmax, ptr(e.out_flow),
                                          ptr(e.occ[0]) if e.seq_bidir else None, o['tol'], o['iters'], o['follow'], ptr(e.stab_path),
                                          ptr(e.stab_ws), ptr(e.out_stab_motion), ptr(e.out_stab_path), ptr(e.out_stab_resid),
                                          ptr(e.out_stab), ptr(e.out_stab_counts), e.engine.stream()), "sequence_stabilise")
    us = [_launches_us(kernel, e.dev) for _ in range(rounds)]
    nbytes = stabilise_bytes(o['iters'], B)
    launches = 2 * o['iters'] + 3
    out['kernel'] = dict(us=round(statistics.mean(us), 2), rounds_us=[round(x, 2) for x in us], launches=launches,
                         compulsory_MB=round(nbytes / 1e6, 2), TBps_of_compulsory=round(nbytes / statistics.mean(us) / 1e6, 3),
                         us_per_launch=round(statistics.mean(us) / launches, 2),
                         how='device events around 50 back-to-back calls of the entry (%d launches each), launch gaps included'
                             % launches)
    out['motion_last_pair'] = [int(v) for v in e.out_stab_motion[B - 1].cpu()]
    out['counts_last_pair'] = [int(v) for v in e.out_stab_counts[B - 1].cpu()]
    assert not bool(e.stab_ws.any())
    if rocprof:
        out['kernel']['rocprofv3'] = stabilise_rocprof(seq)
    del plain, stab
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------- --denoise
def denoise_bytes(B=4):
    """Compulsory bytes of unflow_sequence_denoise per replay on uint8 FRAMEs in (H, W) buffers: per slot and frame pixel the two
    passes each read the flow (8), the mask (1), the frame (3) and the history (8, every word once: neighbouring pixels share
    their taps), the second writes the new history (8) and the denoised pixel (3), and copies the history of the buffer's pixels
    outside the frame (8 + 8); the launches in front and behind copy the history of the whole buffer (16 each)."""
    px, plane = FRAME[0] * FRAME[1], H * W
    return B * (px * (20 + 20 + 8 + 3) + (plane - px) * 16) + plane * 32


def _denoise_call(e):
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr
    L, o = _lib.lib(), e.denoise

    def call():
        check(L.unflow_sequence_denoise(ptr(e.frames), ptr(e.tab), e.B, e.Hmax, e.Wmax, ptr(e.out_flow_bw), ptr(e.occ[1]),
                                        -1 if o['tol'] == 'auto' else o['tol'], o['depth'], ptr(e.den_state), ptr(e.den_ws),
                                        ptr(e.out_den), ptr(e.out_den_stats), e.engine.stream()), "sequence_denoise")
    return call


def _noisy_frames(n):
    """A static smooth picture with noise of its own per frame (sigma 8): the filter has something to average."""
    import numpy as np
    rs = np.random.RandomState(0)
    yy, xx = np.meshgrid(np.arange(FRAME[0]), np.arange(FRAME[1]), indexing='ij')
    base = np.stack([128 + 80 * np.sin(xx / (40.0 + 9 * c)) * np.cos(yy / (30.0 + 7 * c)) for c in range(3)], axis=-1)
    return [np.clip(np.rint(base + rs.randn(*base.shape) * 8.0), 0, 255).astype(np.uint8) for _ in range(n)]


def denoise_kernels_only(iters, B=4):
    """Child: unflow_sequence_denoise alone on a set-up FlowNetC estimator, `iters` times (carry source B, every pair valid)."""
    import torch
    e, _ = _estimator('C', B, 'bidirectional', denoise=True, head_scale=0.1)
    e.denoise_sequence(_noisy_frames(3 * B))
    call = _denoise_call(e)
    torch.cuda.synchronize()
    for _ in range(iters):
        call()
    torch.cuda.synchronize()


def denoise_rocprof(B=4, iters=50):
    """Per-kernel times of the entry from a counters-free kernel-trace child: {kernel: calls, mean us}, and the sum of one entry's
    2 B + 2 launches (the estimator's own few replays are in the means too)."""
    rows, err = _rocprof(['--denoise-kernels-only', '--iters', str(iters)])
    if err:
        return err
    out = {}
    per_entry = {'dn_begin_kernel': 1, 'dn_level_kernel': B, 'dn_filter_kernel': B, 'dn_end_kernel': 1}
    for row in rows:
        for name in per_entry:
            if name in row['Name']:
                out[name] = dict(calls=int(row['Calls']), us=round(float(row['AverageNs']) / 1e3, 2))
    if len(out) == len(per_entry):
        out['kernels_us_per_entry'] = round(sum(out[n]['us'] * k for n, k in per_entry.items()), 2)
    return out


def denoise_case(iters, warmup, rounds, B=4, rocprof=False):
    """The denoising estimator (defaults: tol 'auto', depth 8) against the SAME RUN's plain bidirectional estimator, the two taking
    turns; and the new entry alone, with the bytes it has to move."""
    import gc
    import torch
    plain, _ = _estimator('C', B, 'bidirectional', head_scale=0.1)
    den, mem = _estimator('C', B, 'bidirectional', denoise=True, head_scale=0.1)
    last = den.denoise_sequence(_noisy_frames(3 * B))[-1]    # the tables of the last replay: a carried frame, B pairs
    runs = {'plain': plain.graph.replay, 'denoise': den.graph.replay}
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                # in turn, so that drift of the box hits them alike
        for k, fn in runs.items():
            ms[k].append(_time(fn, iters, warmup))
    out = dict(spec='C', B=B, sequence='bidirectional', rounds=rounds, options=dict(den.denoise))
    for k in runs:
        out[k] = _stats([v for r in ms[k] for v in r], B)
        out[k]['round_means'] = [round(statistics.mean(r) / B, 4) for r in ms[k]]
    out['denoise']['estimator_MB'] = round(mem / 1e6, 1)
    out['denoise_over_plain'] = round(out['denoise']['ms_per_pair'] / out['plain']['ms_per_pair'], 4)
    out['denoise_added_us_per_replay'] = round((out['denoise']['ms_per_pair'] - out['plain']['ms_per_pair']) * B * 1e3, 2)
    us = [_launches_us(_denoise_call(den), den.dev) for _ in range(rounds)]
    nbytes = denoise_bytes(B)
    launches = 2 * B + 2
    out['kernel'] = dict(us=round(statistics.mean(us), 2), rounds_us=[round(x, 2) for x in us], launches=launches,
                         compulsory_MB=round(nbytes / 1e6, 2), TBps_of_compulsory=round(nbytes / statistics.mean(us) / 1e6, 3),
                         us_per_launch=round(statistics.mean(us) / launches, 2),
                         how='device events around 50 back-to-back calls of the entry (%d launches each), launch gaps included'
                             % launches)
    out['last_pair'] = dict(noise=last.noise, tol=last.tol, counts=last.counts)
    assert not bool(den.den_ws[:B * 256].any())
    if rocprof:
        out['kernel']['rocprofv3'] = denoise_rocprof(B)
    del plain, den
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rocprof', action='store_true', help='also the kernel times of rocprofv3 child runs')
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--bidirectional', action='store_true',
                    help="sequence='bidirectional' against the pair-mode bidirectional estimator (DESIGN 7.13)")
    ap.add_argument('--graph-only', choices=('pair', 'sequence', 'bidir', 'pair_bidir'), help=argparse.SUPPRESS)
    ap.add_argument('--visual', action='store_true',
                    help='the pair-mode visual estimator against the sequence visual estimator, FlowNetC (DESIGN 7.14)')
    ap.add_argument('--visual-kernels-only', choices=('pair', 'sequence'), help=argparse.SUPPRESS)
    ap.add_argument('--track', action='store_true',
                    help='the tracking estimator against the same one without tracks and against image_warp launches behind '
                         'the graph, FlowNetC at B = 4, both sequence modes (DESIGN 7.15)')
    ap.add_argument('--rounds', type=int, default=3, help='--track, --interpolate: how often the compared estimators take turns')
    ap.add_argument('--interpolate', type=int, default=None, metavar='N',
                    help='the estimator with N in-between frames per pair against the same one without, FlowNetC at B = 4, both '
                         'sequence modes, and the kernels alone (DESIGN 7.16)')
    ap.add_argument('--order', type=int, default=None, metavar='K',
                    help='with --interpolate N: the estimator with the consistency-ordered splat of steepness K (1..4) against the '
                         'same run\'s unordered interpolating estimator, and the two entries alone (DESIGN 7.19)')
    ap.add_argument('--held_out', action='store_true',
                    help='with --interpolate N: the estimator that scores its in-between frames against the same run\'s '
                         'interpolating estimator without the option, and the scoring entry alone (DESIGN 7.18)')
    ap.add_argument('--ground_truth', action='store_true',
                    help='the scoring estimator against the same one without ground_truth (with --track: both tracking), FlowNetC at '
                         'B = 4, both sequence modes, and evaluate_sequence against pair-mode evaluate (DESIGN 7.17)')
    ap.add_argument('--stabilise', action='store_true',
                    help='the stabilising estimator against the same run\'s plain estimator, FlowNetC at B = 4, both sequence modes, '
                         'and unflow_sequence_stabilise alone (DESIGN 7.20)')
    ap.add_argument('--stabilise-kernels-only', choices=('fw', 'bidir'), help=argparse.SUPPRESS)
    ap.add_argument('--denoise', action='store_true',
                    help='the denoising estimator against the same run\'s plain bidirectional estimator, FlowNetC at B = 4, and '
                         'unflow_sequence_denoise alone (DESIGN 7.21)')
    ap.add_argument('--denoise-kernels-only', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.denoise_kernels_only:
        return denoise_kernels_only(a.iters)
    if a.denoise:
        res = dict(metric='sequence_denoise_ms_per_pair_over_the_same_runs_plain_bidirectional_estimator', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup,
                   expected='no time or ratio was predicted: nobody had measured this entry.  From the bytes: two passes per slot '
                            'over flow, mask, frame and history, one history and one frame written, the history copied in and out '
                            '— %.1f MB per replay at B = 4, tens of microseconds at HBM rate; the entry is 2 B + 2 dependent '
                            'launches, so its launch gaps weigh as much' % (denoise_bytes(4) / 1e6),
                   note='one run on one box; box to box +- 3 %',
                   cases=[denoise_case(a.iters, a.warmup, a.rounds, rocprof=a.rocprof)])
        print(json.dumps(res), flush=True)
        return
    if a.stabilise_kernels_only:
        return stabilise_kernels_only(a.stabilise_kernels_only, a.iters)
    if a.stabilise:
        for seq in (True, 'bidirectional'):              # one line per mode
            res = dict(metric='sequence_stabilise_ms_per_pair_over_the_same_runs_plain_estimator', shape=[H, W],
                       frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup,
                       expected='no time or ratio was predicted: nobody had measured this entry.  From the bytes: the flow read '
                                'iters + 2 times, the frame once, four bytes written per pixel — %.1f MB per replay at the '
                                'defaults, microseconds at HBM rate; the entry is 2 iters + 3 dependent launches, so its launch '
                                'gaps weigh as much' % (stabilise_bytes(3) / 1e6),
                       note='one run on one box; box to box +- 3 %',
                       cases=[stabilise_case(seq, a.iters, a.warmup, a.rounds, rocprof=a.rocprof)])
            print(json.dumps(res), flush=True)
        return
    if a.ground_truth:
        res = dict(metric='sequence_ground_truth_ms_per_pair_over_the_same_estimator_without_it', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup, track=bool(a.track),
                   expected='no ratio was predicted: nobody had measured the scoring kernel; the track kernel of 7.15 (17.5 / 23.2 us '
                            'alone) is the yardstick beside it',
                   note='one run on one box; box to box +- 3 %',
                   cases=[gt_case(seq, a.track, a.iters, a.warmup, a.rounds) for seq in (True, 'bidirectional')])
        print(json.dumps(res))
        return
    if a.order is not None:
        if a.interpolate is None or a.held_out or not 1 <= a.order <= 4:
            ap.error("--order K, 1..4, needs --interpolate N (and no --held_out)")
        res = dict(metric='sequence_interpolate_ordered_ms_per_pair_over_the_same_runs_unordered_interpolating_estimator', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup, n=a.interpolate, order=a.order,
                   expected='from the code: the splat runs at the rate of its 64-bit atomics (0.33 - 0.39 TB/s, DESIGN 7.16) and the '
                            'ordered one adds a few VALU operations per source pixel, so inside the +- 3 % box-to-box spread',
                   note='one run on one box; box to box +- 3 %',
                   cases=[order_case(seq, a.interpolate, a.order, a.iters, a.warmup, a.rounds) for seq in (True, 'bidirectional')])
        print(json.dumps(res))
        return
    if a.held_out:
        if a.interpolate is None:
            ap.error("--held_out needs --interpolate N")
        res = dict(metric='sequence_held_out_ms_per_pair_over_the_same_interpolating_estimator_without_it', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup, n=a.interpolate,
                   expected='no time or ratio was predicted: nobody had measured this kernel; its bytes are about 12 B per pixel and j '
                            'plus the halo',
                   note='one run on one box; box to box +- 3 %',
                   cases=[held_out_case(seq, a.interpolate, a.iters, a.warmup, a.rounds) for seq in (True, 'bidirectional')])
        print(json.dumps(res))
        return
    if a.interpolate is not None:
        res = dict(metric='sequence_interpolate_ms_per_pair_over_the_same_estimator_without_it', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup, n=a.interpolate,
                   expected='no ratio was predicted: the rate of 64-bit integer global atomics on this part was unmeasured when the '
                            'kernel was written',
                   cases=[interpolate_case(seq, a.interpolate, a.iters, a.warmup, a.rounds) for seq in (True, 'bidirectional')])
        print(json.dumps(res))
        return
    if a.track:
        res = dict(metric='sequence_track_ms_per_pair_over_the_same_estimator_without_tracks', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup,
                   expected='no ratio was predicted; from the bytes the kernel is a few microseconds beside a replay of '
                            'milliseconds',
                   cases=[track_case(seq, a.iters, a.warmup, a.rounds) for seq in (True, 'bidirectional')])
        print(json.dumps(res))
        return
    if a.visual_kernels_only:
        return visual_kernels_only(a.visual_kernels_only, a.iters)
    if a.visual:
        res = dict(metric='sequence_visual_ms_per_pair_over_pair_mode_visual', shape=[H, W], frames='uint8 %dx%d' % FRAME,
                   math='bf16x3', iters=a.iters, warmup=a.warmup,
                   expected='from the code, unmeasured when written: the frames kernel does B frames\' work instead of 2B, plus '
                            'a 16-byte-per-pixel row copy', cases=[visual_case(B, a.iters, a.warmup) for B in (1, 4, 8)])
        if a.rocprof:
            res['kernels_B8'] = visual_rocprof(a.iters)
        print(json.dumps(res))
        return
    if a.kernels_only:
        return kernels_only(a.iters)
    if a.graph_only:
        seq = {'pair': False, 'sequence': True, 'bidir': 'bidirectional', 'pair_bidir': False}[a.graph_only]
        return graph_only(seq, a.iters, a.graph_only == 'pair_bidir')
    if a.bidirectional:
        # the prediction of the issue that asked for the mode, from DESIGN 7.3 / 7.5's measurements at FlowNetC, B = 4; printed
        # beside the measurement, never a threshold
        res = dict(metric='bidirectional_sequence_ms_per_pair_over_pair_mode_bidirectional', shape=[H, W],
                   frames='uint8 %dx%d' % FRAME, math='bf16x3', iters=a.iters, warmup=a.warmup,
                   predicted=dict(C_B4=0.9, basis='pair-bidirectional 1.51 x 0.792 = 1.20 ms/pair; one-direction sequence 0.649 '
                                  'ms/pair + the second direction behind the tower 0.51 x 0.792 = 0.40 ms -> 1.05 ms/pair + the '
                                  'mirror, assuming the costs add; unmeasured when it was made'), cases=[])
        for spec in ('C', 'CSS'):
            for B in (1, 4, 8):
                res['cases'].append(case(spec, B, a.iters, a.warmup, bidirectional=True))
        res['mirror_kernel_C'] = mirror_case()
        print(json.dumps(res))
        return
    res = dict(metric='sequence_ms_per_pair_over_pair_mode', shape=[H, W], frames='uint8 %dx%d' % FRAME, math='bf16x3',
               iters=a.iters, warmup=a.warmup, predicted=dict(C=0.75, CSS='closer to 1'), cases=[])
    for spec in ('C', 'CSS'):
        for B in (1, 4, 8):
            res['cases'].append(case(spec, B, a.iters, a.warmup))
    if a.rocprof:
        res.update(rocprof_cases(a.iters))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
