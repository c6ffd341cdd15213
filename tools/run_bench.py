#!/usr/bin/env python3
"""What the summaries of python -m unflow_amd.run cost: the Trainer.train loop without and with them.  A child process per
figure (fresh engine, fresh graph), FlowNetC, B = 4, 384 x 512, device batches from memory, `--warmup` steps then `--steps` timed
steps (host clock around Trainer.train, the stream drained at both ends; the checkpoint at the end of train() is switched off).

  a   on_display = None, display_interval 50 — the loop as it was before the summaries; `--repeats` children, alternated with
      the children of (b) and (c) (their spread is what (b) is held against)
  b   the command's on_display (loss_terms() + the event record) at display_interval 50
  c   the same at display_interval 1
  d   one loss_terms() call after a step, for the default terms and for [train_kitti]'s (fb_weight 0.2, mask_occlusion fb,
      occ_weight 12.4): mean and minimum over 20 calls (each ends with its host synchronisation)

Prints one JSON line; b_inside_a_spread says whether (b) lies inside [min, max] of the repeats of (a).

    python tools/run_bench.py [--steps 60 --warmup 5 --repeats 3] > profiles/run_bench_line.json"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 4, 384, 512
KITTI_TERMS = dict(fb_weight=0.2, mask_occlusion='fb', occ_weight=12.4)


def _trainer(extra, display):
    import torch
    from unflow_amd.core.engine import DEFAULT_PARAMS
    from unflow_amd.core.train import Trainer
    params = dict(DEFAULT_PARAMS, learning_rate=1e-5, display_interval=display, save_interval=1 << 30, **extra)
    tr = Trainer(B, H, W, params)
    tr.save = lambda *a, **k: None
    g = torch.Generator().manual_seed(1)
    pool = [tuple((torch.rand(B, H, W, 3, generator=g) * 255).to(tr.engine.dev) for _ in range(2)) for _ in range(4)]

    def batches(_offset):
        i = 0
        while True:
            yield pool[i % len(pool)]
            i += 1
    return tr, batches


def figure_loop(display, summaries, steps, warmup):
    import contextlib
    import io
    import torch
    from unflow_amd.core.summary import SummaryWriter
    from unflow_amd.run import train_scalars
    tr, batches = _trainer({}, display)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        writer = SummaryWriter(tmp)
        hook = (lambda i, loss, trainer: writer.add_scalars(i, train_scalars(loss, trainer))) if summaries else None
        tr.train(2, 1 + warmup, 0, batches, tmp, on_display=hook)          # from i = 2: no display at i == 1
        torch.cuda.synchronize()
        first = 2 + warmup              # display_interval 50, 60 steps from i = 7: one display step (i = 50) inside the timed steps
        t0 = time.perf_counter()
        tr.train(first, first + steps - 1, warmup, batches, tmp, on_display=hook)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1000.0 / steps
        writer.close()
    return dict(ms_per_step=round(ms, 4), pairs_per_s=round(B * 1000.0 / ms, 1),
                display_steps=sum(1 for i in range(first, first + steps) if i % display == 0))


def figure_terms(extra, calls=20):
    import contextlib
    import io
    tr, batches = _trainer(extra, 1 << 30)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        tr.train(2, 4, 0, batches, tmp)
    tr.engine.loss_terms()                                                  # allocates its scratch
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        tr.engine.loss_terms()
        ms.append((time.perf_counter() - t0) * 1000.0)
    return dict(mean_ms=round(sum(ms) / len(ms), 4), min_ms=round(min(ms), 4), calls=calls)


def child(name, steps, warmup):
    if name == 'a':
        return figure_loop(50, False, steps, warmup)
    if name == 'b':
        return figure_loop(50, True, steps, warmup)
    if name == 'c':
        return figure_loop(1, True, steps, warmup)
    return figure_terms(KITTI_TERMS if name == 'd_train_kitti' else {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3, help='children of figure (a)')
    ap.add_argument('--figure', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.figure:
        print('FIGURE ' + json.dumps(child(args.figure, args.steps, args.warmup)))
        return 0

    def run(name):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--figure', name, '--steps', str(args.steps), '--warmup',
                            str(args.warmup)], capture_output=True, text=True, timeout=600)
        lines = [l for l in r.stdout.splitlines() if l.startswith('FIGURE ')]
        if r.returncode != 0 or len(lines) != 1:
            raise SystemExit("figure %s failed (status %d):\n%s%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
        return json.loads(lines[0][len('FIGURE '):])

    a, b, c = [], None, None                  # alternated: a, b, a, c, a ... (the repeats of (a) bracket the other two)
    for k in range(args.repeats):
        a.append(run('a'))
        if k == 0:
            b = run('b')
        elif k == 1:
            c = run('c')
    b, c = b or run('b'), c or run('c')
    lo, hi = min(x['ms_per_step'] for x in a), max(x['ms_per_step'] for x in a)
    mean_a = sum(x['ms_per_step'] for x in a) / len(a)
    out = dict(shape=[B, H, W], net='C', steps=args.steps, warmup=args.warmup, math=os.environ.get('UNFLOW_CONV_MATH', 'bf16x3'),
               a_no_summaries=a, b_display_50=b, c_display_1=c, a_spread_ms=[lo, hi], b_over_a=round(b['ms_per_step'] / mean_a, 4),
               c_over_a=round(c['ms_per_step'] / mean_a, 4), b_inside_a_spread=bool(lo <= b['ms_per_step'] <= hi),
               b_not_slower_than_a_spread=bool(b['ms_per_step'] <= hi),
               d_loss_terms=dict(default=run('d_default'), train_kitti=run('d_train_kitti')))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
