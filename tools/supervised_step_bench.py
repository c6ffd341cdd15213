#!/usr/bin/env python3
"""Time the supervised fine-tuning step (one-direction engine, FlowNetEngine(supervised=True)) against the unsupervised step of the
same configuration at the same shape: graph-captured StepRunner steps, device events around `--steps` steps after `--warmup`.
Default shape: [train_kitti_ft] (B = 4, 320 x 768).  Prints one JSON line.

    python tools/supervised_step_bench.py [--batch 4 --height 320 --width 768 --steps 20 --warmup 5] [--geometric [--rounds 5 --reps 2000]]

--geometric adds two measurements for FlowNetC at the same shape, each alternated in one process, `--rounds` rounds
per side after a warm-up of both, device events around every round:
  geo_input   the fused unflow_supervised_geo_augment launch against the launches it replaces for the IMAGE part — the chain of
              engine.set_input for the unsupervised step (unflow_prepare_image_pair, transformer x 2, the copy, photometric; no
              flow, no mask: less work).  Means, the spread between rounds of the same code, and whether the fused launch is
              within that spread of the chain (the requirement) or faster.
  geo_step    the supervised step with augment_geometric draws against the photometric-only step, same engine.  Recorded only."""
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


def _rounds(sides, rounds, reps):
    """Alternate the callables of `sides` (name -> fn), `rounds` rounds of `reps` calls each, device events around every round.
    name -> per-call ms of every round."""
    import torch
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return out


def _summary(ms):
    return dict(mean_ms=round(sum(ms) / len(ms), 4), spread_ms=round(max(ms) - min(ms), 4), rounds_ms=[round(v, 4) for v in ms])


def time_geometric(B, H, W, steps, warmup, rounds, reps):
    import torch
    from unflow_amd import _lib
    from unflow_amd._lib import check, cl, ptr, stream
    from unflow_amd.core import augment as A
    from unflow_amd.core.engine import CHANNEL_MEAN, DEFAULT_PARAMS, FlowNetEngine
    from unflow_amd.core.train import StepRunner
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1)
    im1 = (torch.rand(B, H, W, 3, generator=g) * 255).to(dev)
    im2 = (torch.rand(B, H, W, 3, generator=g) * 255).to(dev)
    flow, mask = (torch.randn(B, H, W, 2, generator=g) * 5).to(dev), (torch.rand(B, H, W, 1, generator=g) > 0.1).float().to(dev)
    draws = A.draw_supervised_augmentation(B, g, geometric=True)
    ddev = {k: v.to(dev) for k, v in draws.items()}
    mats = A.affine_pixel_maps(draws['theta_global'], draws['theta_local'], H, W).to(dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    im01, x0, tmp, fo, mo = z(2 * B, H, W, 3), z(2 * B, H, W, 4), z(2 * B, H, W, 3), z(B, H, W, 2), z(B, H, W, 1)
    mean_host = (_lib.ctypes.c_float * 3)(*CHANNEL_MEAN)
    lib = _lib.lib()

    def chain():          # engine.set_input's launches for the unsupervised step, border mask off
        st = stream(dev)
        check(lib.unflow_prepare_image_pair(ptr(im1), ptr(im2), cl(B * H * W), ptr(x0), ptr(tmp), mean_host, None, st), "prepare")
        A.transformer(tmp, ddev['theta_global'], out=im01, n_samples=2 * B)
        A.transformer(im01[B:], ddev['theta_local'], out=tmp[B:], n_samples=B)
        check(lib.unflow_copy(ptr(im01[B:]), ptr(tmp[B:]), _lib.csz(B * H * W * 3 * 4), st), "copy")
        A.photometric(im01, ddev, out=x0, mean=CHANNEL_MEAN)

    def fused():
        A.supervised_geo_augment(im1, im2, flow, mask, mats, ddev, im01, x0, fo, mo, mean=CHANNEL_MEAN)

    for fn in (chain, fused):
        for _ in range(max(warmup, 3)):
            fn()
    torch.cuda.synchronize()
    r = _rounds(dict(chain=chain, fused=fused), rounds, reps)
    ch, fu = _summary(r['chain']), _summary(r['fused'])
    spread = max(ch['spread_ms'], fu['spread_ms'])
    geo_input = dict(calls_per_round=reps, chain=ch, fused=fu, fused_over_chain=round(fu['mean_ms'] / ch['mean_ms'], 3),
                     bytes_per_pixel_counted=100, fused_not_slower_than_spread=bool(fu['mean_ms'] - ch['mean_ms'] <= spread))

    eng = FlowNetEngine(B, H, W, params=dict(DEFAULT_PARAMS, flownet='C'), device=dev, seed=0, supervised=True)
    run = StepRunner(eng)
    photo = {k: v for k, v in draws.items() if not k.startswith('theta')}
    step = lambda aug: (lambda: run.step(im1, im2, 1e-5, augment=aug, target=(flow, mask)))      # noqa: E731
    sides = dict(photometric=step(photo), geometric=step(draws))
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    r = _rounds(sides, rounds, steps)
    eng.check_device_faults()
    ph, ge = _summary(r['photometric']), _summary(r['geometric'])
    geo_step = dict(photometric=ph, geometric=ge, geometric_over_photometric=round(ge['mean_ms'] / ph['mean_ms'], 4))
    del run, eng
    torch.cuda.empty_cache()
    return geo_input, geo_step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=320)
    ap.add_argument('--width', type=int, default=768)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--geometric', action='store_true', help='also time the geometric augmentation (see above)')
    ap.add_argument('--rounds', type=int, default=5, help='--geometric: alternated rounds per side (at least 3)')
    ap.add_argument('--reps', type=int, default=2000, help='--geometric: calls of the input launches per round (a round should last a good fraction of a second)')
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    B, H, W = args.batch, args.height, args.width
    out = dict(shape=[B, H, W], steps=args.steps, math=os.environ.get('UNFLOW_CONV_MATH', 'bf16x3'))
    for spec, train_all in (('C', False), ('CSS', True)):
        sup = time_step(spec, train_all, True, B, H, W, args.steps, args.warmup)
        uns = time_step(spec, train_all, False, B, H, W, args.steps, args.warmup)
        key = spec + ('_train_all' if train_all else '')
        out[key] = dict(supervised_ms=round(sup, 3), unsupervised_ms=round(uns, 3), ratio=round(sup / uns, 3),
                        supervised_pairs_per_s=round(B * 1000.0 / sup, 1))
    if args.geometric:
        out['geo_input'], out['geo_step'] = time_geometric(B, H, W, args.steps, args.warmup, args.rounds, args.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
