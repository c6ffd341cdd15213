#!/usr/bin/env python3
"""Time the supervised fine-tuning step (one-direction engine, FlowNetEngine(supervised=True)) against the unsupervised step of the
same configuration at the same shape: graph-captured StepRunner steps, device events around `--steps` steps after `--warmup`.
Default shape: [train_kitti_ft] (B = 4, 320 x 768).  Prints one JSON line.

    python tools/supervised_step_bench.py [--batch 4 --height 320 --width 768 --steps 20 --warmup 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_step(spec, train_all, supervised, B, H, W, steps, warmup):
    import torch
    from unflow_amd.core.engine import FlowNetEngine, DEFAULT_PARAMS
    from unflow_amd.core.train import StepRunner
    dev = torch.device('cuda:0')
    params = dict(DEFAULT_PARAMS, flownet=spec, train_all=train_all)
    eng = FlowNetEngine(B, H, W, params=params, device=dev, seed=0, supervised=supervised)
    run = StepRunner(eng)
    g = torch.Generator().manual_seed(1)
    im1 = (torch.rand(B, H, W, 3, generator=g) * 255).to(dev)
    im2 = (torch.rand(B, H, W, 3, generator=g) * 255).to(dev)
    target = ((torch.randn(B, H, W, 2, generator=g) * 5).to(dev), (torch.rand(B, H, W, 1, generator=g) > 0.5).float().to(dev)) \
        if supervised else None
    for _ in range(warmup):
        run.step(im1, im2, 1e-5, target=target)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        loss = run.step(im1, im2, 1e-5, target=target)
    b.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    eng.check_device_faults()
    ms = a.elapsed_time(b) / steps
    del run, eng
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=320)
    ap.add_argument('--width', type=int, default=768)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    B, H, W = args.batch, args.height, args.width
    out = dict(shape=[B, H, W], steps=args.steps, math=os.environ.get('UNFLOW_CONV_MATH', 'bf16x3'))
    for spec, train_all in (('C', False), ('CSS', True)):
        sup = time_step(spec, train_all, True, B, H, W, args.steps, args.warmup)
        uns = time_step(spec, train_all, False, B, H, W, args.steps, args.warmup)
        key = spec + ('_train_all' if train_all else '')
        out[key] = dict(supervised_ms=round(sup, 3), unsupervised_ms=round(uns, 3), ratio=round(sup / uns, 3),
                        supervised_pairs_per_s=round(B * 1000.0 / sup, 1))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
