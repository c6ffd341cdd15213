"""python -m unflow_amd.visualize: look at the flow of a trained experiment on KITTI — the GUI part of the reference's
src/eval_gui.py as image files, on core/inference.FlowEstimator(visual=True) (the pictures are made on the device, inside the
inference graph: csrc/visual.hip).

    python -m unflow_amd.visualize --ex NAME [--variant train_2012] [--num 10] [--num_vis 100] [--batch_size 4] [--sheet]

The experiment and its checkpoint are found as python -m unflow_amd.evaluate finds them.  For the k-th example, <--out>/NAME/
gets %06d_img.png (the overlay of both frames), %06d_flow.png (the flow's colour wheel), %06d_diff.png (the brightness error
|im1 - warp(im2, flow)|) and, on the train_* variants, %06d_err.png (the KITTI devkit's error map: blue correct, red wrong, dark
occluded) and %06d_gt.png (the ground truth's colour wheel).  eval_gui.py --output_visual (:248-254) writes the brightness error
into _flow.png and the flow colours into _err.png and never writes the error map; the names' evident meaning is followed.
--sheet: the pages of its window (e2eflow/gui.py: four examples each) as contact sheets page_%03d.png over the first --num_vis
examples: one row per example, one column per image slot of eval_gui.py:160-204, smaller frames padded with black.  There is
no window on screen, and only --dataset kitti (the other datasets: python -m unflow_amd.evaluate_flo --visual)."""
import argparse
import os
import sys

import numpy as np

from .evaluate import VARIANTS, _KITTIData, add_encode_flags, check_encode_flags, experiment_paths

EXAMPLES_PER_PAGE = 4                                   # eval_gui.py NUM_EXAMPLES_PER_PAGE
# the columns of a sheet: eval_gui.py's image slots on ground truth (:160-178, :190-194) and without (:199-204)
SHEET_COLUMNS = {True: ('overlay', 'warp_error', 'flow', 'gt', 'error'), False: ('overlay', 'warp_error', 'flow')}


def parser():
    ap = argparse.ArgumentParser(prog='python -m unflow_amd.visualize', description=__doc__.split('\n')[0])
    ap.add_argument('--ex', required=True, help='experiment name')
    ap.add_argument('--dataset', default='kitti', help="only 'kitti' (sintel / chairs / mdb: python -m unflow_amd.evaluate_flo)")
    ap.add_argument('--variant', default='train_2012', choices=VARIANTS)
    ap.add_argument('--num', type=int, default=10, help='examples to process; -1: all (eval_gui.py --num)')
    ap.add_argument('--num_vis', type=int, default=100, help='examples on the contact sheets (eval_gui.py --num_vis)')
    ap.add_argument('--sheet', action='store_true', help='also write page_%%03d.png contact sheets, four examples per page')
    ap.add_argument('--batch_size', type=int, default=4, help='pairs per graph replay')
    ap.add_argument('--host_decode', action='store_true',
                    help="decode the PNG files with the host's decoder (slow) instead of the library's PNG kernels")
    add_encode_flags(ap)
    ap.add_argument('--config', default='../config.ini', help='the project config.ini (dirs: data, log, checkpoints)')
    ap.add_argument('--out', default='../out', help='output root: files go to <out>/<ex>/')
    ap.add_argument('--dims', type=int, nargs=2, default=(384, 1280), metavar=('H', 'W'),
                    help='network input size (eval_gui.py: 384 1280)')
    return ap


def parse_args(argv=None):
    """Parsed flags; refuses what this tool does not do with a clear message (SystemExit, status 2)."""
    ap = parser()
    a = ap.parse_args(argv)
    check_encode_flags(ap, a)
    if a.dataset != 'kitti':
        ap.error("--dataset %s is not supported here (only kitti; python -m unflow_amd.evaluate_flo scores and draws sintel / "
                 "chairs / mdb)" % a.dataset)
    if a.batch_size <= 0:
        ap.error("--batch_size must be positive")
    if a.num_vis < 0:
        ap.error("--num_vis must not be negative")
    return a


def contact_sheet(rows):
    """rows: per example a list of uint8 [h, w, 3] images (sizes may differ, rows may be of unequal length) -> one uint8 image:
    a grid of cells of the largest height and width, each image at the top left of its cell, the rest black."""
    rows = [[np.asarray(im) for im in r] for r in rows]
    ims = [im for r in rows for im in r]
    if not ims:
        raise ValueError("contact_sheet: no images")
    for im in ims:
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("contact_sheet: expected uint8 [h,w,3] images, got %s %s" % (im.dtype, im.shape))
    ch, cw = max(im.shape[0] for im in ims), max(im.shape[1] for im in ims)
    sheet = np.zeros((ch * len(rows), cw * max(len(r) for r in rows), 3), np.uint8)
    for j, r in enumerate(rows):
        for i, im in enumerate(r):
            sheet[j * ch:j * ch + im.shape[0], i * cw:i * cw + im.shape[1]] = im
    return sheet


def sheet_name(page):
    return 'page_%03d.png' % page


def write_pictures(examples, out_dir, sheet=False, num_vis=100, workers=0, level=6):
    """Writes the picture files of every example (dicts of FlowEstimator.pictures) and, with sheet, the contact sheets of the
    first num_vis of them; returns the written paths.  workers >= 1: the per-example pictures go through a writer pool
    (png_device.DeviceFileWriter) from the examples' 'scanlines' (FlowEstimator.pictures(..., scanlines=True); zlib streams where
    'scanlines_kind' says 'png_z': pictures(..., deflate='device')); the contact sheets
    are composed and written on the host either way."""
    from .core.inference import VISUAL_IMAGES, visual_files
    from .core.input import write_png_rgb8
    paths, page_rows, page = [], [], 0
    pool = None
    if workers:
        from .core.png_device import DeviceFileWriter
        pool = DeviceFileWriter(workers, level)

    def flush():
        nonlocal page_rows, page
        if page_rows:
            p = os.path.join(out_dir, sheet_name(page))
            write_png_rgb8(p, contact_sheet(page_rows))
            paths.append(p)
            page_rows, page = [], page + 1
    try:
        for n, ex in enumerate(examples):
            for k, name in visual_files(n, 'error' in ex):
                p = os.path.join(out_dir, name)
                if pool is not None:
                    pool.submit(p, ex.get('scanlines_kind', 'png'), ex['scanlines'][VISUAL_IMAGES[k]])
                else:
                    write_png_rgb8(p, ex[VISUAL_IMAGES[k]])
                paths.append(p)
            if sheet and n < num_vis:
                page_rows.append([ex[c] for c in SHEET_COLUMNS['error' in ex]])
                if len(page_rows) == EXAMPLES_PER_PAGE:
                    flush()
        flush()
    except BaseException:
        if pool is not None:
            pool.__exit__(*sys.exc_info())
        raise
    if pool is not None:
        pool.close()
    return paths


def main(argv=None):
    a = parse_args(argv)
    import shutil
    from .core.util import config_dict, convert_input_strings
    from .core.inference import FlowEstimator
    from .kitti.input import KITTIInput
    cfg_path, ckpt_dir = experiment_paths(a.ex, a.config)
    config = config_dict(cfg_path)
    params = dict(config.get('train', {}))
    dirs = config_dict(a.config).get('dirs', {})
    convert_input_strings(params, dirs)
    params.update(config.get('train_' + a.dataset, {}))
    est = FlowEstimator.from_checkpoint(ckpt_dir, params, a.batch_size, net_size=tuple(a.dims), visual=True)
    kinput = KITTIInput(_KITTIData(dirs.get('data', '')), batch_size=a.batch_size, normalize=False, dims=tuple(a.dims))
    out_dir = os.path.join(a.out, a.ex)
    if os.path.isdir(out_dir):
        shutil.rmtree(out_dir)
    os.makedirs(out_dir)
    shutil.copyfile(cfg_path, os.path.join(out_dir, 'config.ini'))
    print("-- visualising %s (step %s) on kitti %s" % (a.ex, est.global_step, a.variant))
    batches = getattr(kinput, 'input_' + a.variant)(device=None if a.host_decode else est.dev)
    examples = est.pictures(batches, num=None if a.num < 0 else a.num, scanlines=a.encode_workers > 0, deflate=a.deflate)
    paths = write_pictures(examples, out_dir, sheet=a.sheet, num_vis=a.num_vis, workers=a.encode_workers, level=a.level)
    print("wrote %d files to %s" % (len(paths), out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
