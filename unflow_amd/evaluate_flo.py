"""python -m unflow_amd.evaluate_flo: score a trained experiment on Sintel, FlyingChairs or Middlebury, write benchmark files and
pictures — the rest of the reference's src/eval_gui.py (:303-322), beside python -m unflow_amd.evaluate (KITTI).

    python -m unflow_amd.evaluate_flo --dataset {sintel,chairs,mdb} --ex NAME [--variant ...] [--num 10] [--batch_size 4]
                                      [--occlusion] [--output_benchmark [--output_png] [--output_backward]]
                                      [--visual [--sheet]] [--host_decode] [--dims H W]
                                      [--sequence [--track [--track_stride S]]]

Variants: sintel train_clean (default), train_final, test_clean, test_final; chairs test; mdb train (default), test.  The
network input size defaults to eval_gui.py's: 512 x 1024, 384 x 512, 512 x 640.  The experiment, its config ([train] and
[train_<dataset>]) and its checkpoint are found as python -m unflow_amd.evaluate finds them.  The frames, the .flo ground truth
and Sintel's masks are decoded on the device (core/png_device.py) unless --host_decode.  On variants with ground truth the
scores are printed: AEE/<map> and outliers/<map> — occluded and non-occluded on Sintel, all on the one-map datasets — and, on
Sintel with --occlusion, this project's occlusion precision / recall / F1 of the forward-backward mask against Sintel's
occlusion maps.  --output_benchmark and --visual write through FlowEstimator.export to <--out>/NAME/: %06d_10.flo (or .png),
with --output_backward %06d_01, with --occlusion %06d_10_occ.png, with --visual the pictures of python -m unflow_amd.visualize
(--sheet: its contact sheets, too).

--sequence (Sintel's train_* variants): the scenes are evaluated as clips — FlowEstimator(..., sequence=...,
ground_truth=True).evaluate_sequence: every frame uploaded and encoded once, the frames decoded as python -m unflow_amd.sequence
decodes them, the ground truth composed at the files' own size (no crop, no padding).  The same score lines are printed; --track
follows every pixel of each scene's first frame (--track_stride S: every S-th pixel of every S-th row) and adds track/epe,
track/delta_avg, track/AJ and track/occ_acc against the chained ground-truth flow.  With --output_benchmark the files of
python -m unflow_amd.sequence go to <--out>/NAME/<scene>/."""
import argparse
import os
import shutil
import sys

from .evaluate import add_encode_flags, check_encode_flags, experiment_paths

DATASETS = {      # variants (the first is the default), eval_gui.py's dims
    'sintel': (('train_clean', 'train_final', 'test_clean', 'test_final'), (512, 1024)),
    'chairs': (('test',), (384, 512)),
    'mdb': (('train', 'test'), (512, 640)),
}
WITH_GT = {('sintel', 'train_clean'), ('sintel', 'train_final'), ('chairs', 'test'), ('mdb', 'train')}


def parser():
    ap = argparse.ArgumentParser(prog='python -m unflow_amd.evaluate_flo', description=__doc__.split('\n')[0])
    ap.add_argument('--ex', required=True, help='experiment name')
    ap.add_argument('--dataset', required=True, choices=sorted(DATASETS), help='kitti: python -m unflow_amd.evaluate')
    ap.add_argument('--variant', default=None, help='the split, see above (default: the first of the dataset)')
    ap.add_argument('--num', type=int, default=10, help='examples to evaluate; -1: all (eval_gui.py --num)')
    ap.add_argument('--num_vis', type=int, default=100, help='examples on the contact sheets (eval_gui.py --num_vis)')
    ap.add_argument('--output_benchmark', action='store_true', help='write the flow files')
    ap.add_argument('--output_png', action='store_true', help='KITTI 16-bit PNG files (default: .flo)')
    ap.add_argument('--output_backward', action='store_true', help='with --output_benchmark: also the backward flow (%%06d_01)')
    ap.add_argument('--occlusion', action='store_true',
                    help='forward-backward occlusion: scores on Sintel train_*, %%06d_10_occ.png with --output_benchmark')
    ap.add_argument('--visual', action='store_true', help='write the pictures (overlay, flow colours, errors) beside the flow files')
    ap.add_argument('--sheet', action='store_true', help='with --visual: also page_%%03d.png contact sheets, four examples per page')
    ap.add_argument('--batch_size', type=int, default=4, help='pairs per graph replay')
    ap.add_argument('--host_decode', action='store_true',
                    help="read the files with the host's decoders (slow) instead of the library's kernels")
    ap.add_argument('--sequence', action='store_true',
                    help='sintel train_*: evaluate scene by scene as clips, every frame encoded once (see above)')
    ap.add_argument('--track', action='store_true',
                    help='with --sequence: also score the tracks of every pixel of a scene\'s first frame')
    ap.add_argument('--track_stride', type=int, default=None, metavar='S',
                    help='like --track, for every S-th pixel of every S-th row')
    add_encode_flags(ap)
    ap.add_argument('--config', default='../config.ini', help='the project config.ini (dirs: data, log, checkpoints)')
    ap.add_argument('--out', default='../out', help='output root: files go to <out>/<ex>/')
    ap.add_argument('--dims', type=int, nargs=2, default=None, metavar=('H', 'W'), help="network input size (default: eval_gui.py's)")
    return ap


def parse_args(argv=None):
    """Parsed flags with the dataset's defaults filled in (variant, dims; num = None for all); refuses what this tool does not
    do with a clear message (SystemExit, status 2)."""
    ap = parser()
    a = ap.parse_args(argv)
    check_encode_flags(ap, a)
    variants, dims = DATASETS[a.dataset]
    if a.variant is None:
        a.variant = variants[0]
    if a.variant not in variants:
        ap.error("--variant %s: --dataset %s has %s" % (a.variant, a.dataset, ', '.join(variants)))
    a.dims = tuple(a.dims) if a.dims else dims
    a.num = None if a.num < 0 else a.num
    a.has_gt = (a.dataset, a.variant) in WITH_GT
    if a.output_backward and not a.output_benchmark:
        ap.error("--output_backward requires --output_benchmark")
    if a.sheet and not a.visual:
        ap.error("--sheet requires --visual")
    if a.batch_size <= 0:
        ap.error("--batch_size must be positive")
    if a.num_vis < 0:
        ap.error("--num_vis must not be negative")
    if a.sequence and a.dataset != 'sintel':
        ap.error("--sequence evaluates clips: --dataset %s is a training set of pairs (only sintel has scenes)" % a.dataset)
    if a.sequence and not a.has_gt:
        ap.error("--sequence scores clips against ground truth: --variant %s has none (python -m unflow_amd.sequence writes the "
                 "flow of a clip)" % a.variant)
    if a.sequence and (a.visual or a.sheet):
        ap.error("--sequence writes no pictures here: python -m unflow_amd.sequence --visual draws a clip")
    if (a.track or a.track_stride is not None) and not a.sequence:
        ap.error("--track / --track_stride score tracks along a clip: they need --sequence")
    if a.track_stride is not None and a.track_stride < 1:
        ap.error("--track_stride must be at least 1")
    a.track_option = (a.track_stride if a.track_stride is not None else True) if (a.track or a.track_stride is not None) else False
    return a


from .data import Data as _Data      # the data root alone (dirs.data)       # noqa: E402


def dataset_input(dataset, root, batch_size, dims):
    if dataset == 'sintel':
        from .sintel.input import SintelInput as cls
    elif dataset == 'chairs':
        from .chairs.input import ChairsInput as cls
    else:
        from .middlebury.input import MiddleburyInput as cls
    return cls(_Data(root), batch_size=batch_size, normalize=False, dims=tuple(dims))


def write_sheets(out_dir, n_examples, has_gt, num_vis):
    """The contact sheets of python -m unflow_amd.visualize --sheet over the first num_vis examples, put together from the
    picture files export(visual=True) has just written to out_dir (read back: no further pass over the input and the network);
    returns the written paths."""
    from .core.inference import VISUAL_IMAGES, visual_files
    from .core.input import decode_png, write_png_rgb8
    from .visualize import EXAMPLES_PER_PAGE, SHEET_COLUMNS, contact_sheet, sheet_name
    rows = []
    for n in range(min(n_examples, num_vis)):
        files = {VISUAL_IMAGES[k]: os.path.join(out_dir, name) for k, name in visual_files(n, has_gt)}
        row = []
        for column in SHEET_COLUMNS[has_gt]:
            with open(files[column], 'rb') as f:
                row.append(decode_png(f.read()))
        rows.append(row)
    paths = []
    for page, r0 in enumerate(range(0, len(rows), EXAMPLES_PER_PAGE)):
        paths.append(os.path.join(out_dir, sheet_name(page)))
        write_png_rgb8(paths[-1], contact_sheet(rows[r0:r0 + EXAMPLES_PER_PAGE]))
    return paths


TRACK_NAMES = ('track/epe', 'track/delta_avg', 'track/AJ', 'track/occ_acc')


def clip_stream(dinput, clips, batch, device, num=None):
    """(frames, gts) per clip for FlowEstimator.evaluate_sequence / export_sequence, cut behind `num` pairs: the frames as
    python -m unflow_amd.sequence decodes them — device tensors, or read_frame's arrays with device=None — and per pair the
    two-map ground truth at the files' own size: png_device.sintel_gt_device's tensors, or SintelInput.read_gt_full's arrays."""
    from .sequence import device_frames, read_frame
    left = None if num is None else int(num)
    for _, files, triples in clips:
        if left is not None:
            if left <= 0:
                return
            files, triples = files[:left + 1], triples[:left]
            left -= len(triples)
        if device is None:
            frames = (read_frame(p) for p in files)
            gts = [dinput.read_gt_full(*t) for t in triples]
        else:
            from .core.png_device import sintel_gt_device
            frames = device_frames(files, batch, device)
            flow, mask = sintel_gt_device(triples, device)
            gts = [(flow[0, i], mask[0, i], flow[1, i], mask[1, i]) for i in range(len(triples))]
        yield frames, gts


def main_sequence(a, ckpt_dir, cfg_path, params, dirs):
    """--sequence: Sintel's scenes as clips."""
    from .core.inference import OCC_NAMES, FlowEstimator
    from .sequence import png_size
    dinput = dataset_input(a.dataset, dirs.get('data', ''), a.batch_size, a.dims)
    clips = dinput.clips(a.variant.split('_')[1])
    if not clips:
        raise SystemExit("Error: no scenes under sintel/training/%s" % a.variant.split('_')[1])
    sizes = [png_size(files[0]) for _, files, _ in clips]
    est = FlowEstimator.from_checkpoint(ckpt_dir, params, a.batch_size, net_size=a.dims,
                                        max_frame=(max(s[0] for s in sizes), max(s[1] for s in sizes)),
                                        sequence='bidirectional' if (a.output_backward or a.occlusion) else True,
                                        track=a.track_option, ground_truth=True)
    dev = None if a.host_decode else est.dev
    print("-- evaluating %s (step %s) on %s %s, %d scenes as clips" % (a.ex, est.global_step, a.dataset, a.variant, len(clips)))
    try:
        res = est.evaluate_sequence(clip_stream(dinput, clips, a.batch_size, dev, a.num))
    except ValueError as err:
        raise SystemExit("Error: %s" % err)
    for k in res['names'] + [k for k in OCC_NAMES if a.occlusion and k in res] + [k for k in TRACK_NAMES if k in res]:
        print("%-24s %.4f" % (k, res[k]))
    print("examples: %d" % res['num_examples'])
    if a.output_benchmark:
        out_dir = os.path.join(a.out, a.ex)
        if os.path.isdir(out_dir):
            shutil.rmtree(out_dir)
        os.makedirs(out_dir)
        shutil.copyfile(cfg_path, os.path.join(out_dir, 'config.ini'))
        paths = []
        for (name, _, _), (frames, _) in zip(clips, clip_stream(dinput, clips, a.batch_size, dev, a.num)):
            paths += est.export_sequence(frames, os.path.join(out_dir, name), fmt='png' if a.output_png else 'flo',
                                         workers=a.encode_workers, level=a.level, deflate=a.deflate, backward=a.output_backward,
                                         occlusion=a.occlusion, tracks=a.track_option is not False)
        print("wrote %d files to %s" % (len(paths), out_dir))
    return 0


def main(argv=None):
    a = parse_args(argv)
    from .core.util import config_dict, convert_input_strings
    from .core.inference import OCC_NAMES, FlowEstimator
    cfg_path, ckpt_dir = experiment_paths(a.ex, a.config)
    config = config_dict(cfg_path)
    params = dict(config.get('train', {}))
    dirs = config_dict(a.config).get('dirs', {})
    convert_input_strings(params, dirs)
    params.update(config.get('train_' + a.dataset, {}))
    if a.sequence:
        return main_sequence(a, ckpt_dir, cfg_path, params, dirs)
    est = FlowEstimator.from_checkpoint(ckpt_dir, params, a.batch_size, net_size=a.dims,
                                        bidirectional=a.output_backward or a.occlusion, visual=a.visual)
    dinput = dataset_input(a.dataset, dirs.get('data', ''), a.batch_size, a.dims)
    dev = None if a.host_decode else est.dev
    batches = lambda: getattr(dinput, 'input_' + a.variant)(device=dev)            # noqa: E731
    print("-- evaluating %s (step %s) on %s %s" % (a.ex, est.global_step, a.dataset, a.variant))
    if a.has_gt:
        res = est.evaluate(batches(), num=a.num)
        for k in res['names'] + [k for k in OCC_NAMES if a.occlusion and k in res]:
            print("%-24s %.4f" % (k, res[k]))
        print("examples: %d" % res['num_examples'])
    if a.output_benchmark or a.visual:
        out_dir = os.path.join(a.out, a.ex)
        if os.path.isdir(out_dir):
            shutil.rmtree(out_dir)
        os.makedirs(out_dir)
        shutil.copyfile(cfg_path, os.path.join(out_dir, 'config.ini'))
        paths = est.export(batches(), out_dir, fmt='png' if a.output_png else 'flo', num=a.num, backward=a.output_backward,
                           occlusion=a.occlusion, visual=a.visual, workers=a.encode_workers, level=a.level,
                           deflate=a.deflate)
        if a.sheet:
            paths += write_sheets(out_dir, sum(p.endswith('_img.png') for p in paths), a.has_gt, a.num_vis)
        print("wrote %d files to %s" % (len(paths), out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
