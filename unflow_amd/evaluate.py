"""python -m unflow_amd.evaluate: score a trained experiment on KITTI and write benchmark files — the non-GUI part of the
reference's src/eval_gui.py, on core/inference.FlowEstimator (batched, graph-replayed, forward only).

    python -m unflow_amd.evaluate --ex NAME [--variant train_2012] [--num 10] [--occlusion] [--host_decode]
                                  [--output_benchmark [--output_png] [--output_backward]]

The experiment's config.ini (<dirs.log>/ex/NAME/config.ini, else --config) gives the network spec ([train] and
[train_kitti]); the checkpoint is the experiment's latest — its logs folder first, then <dirs.checkpoints>/NAME
(eval_gui.py:101-117).  Benchmark files go to <--out>/NAME/ beside a copy of the config: %06d_10.png (KITTI 16-bit) with
--output_png, else %06d_10.flo; with --output_backward also the backward flow, %06d_01.png / .flo (the file eval_gui.py's
--output_backward branch means to write).  --occlusion runs both directions and adds the forward-backward occlusion mask
(losses.occlusion): this project's occlusion precision / recall / F1 against KITTI's occluded pixels on train_* variants,
and %06d_10_occ.png (8-bit, 255 = occluded) with --output_benchmark.  The pictures (colour wheel, error map, overlay) are
python -m unflow_amd.visualize's; Sintel, FlyingChairs and Middlebury are python -m unflow_amd.evaluate_flo's.
--workers N (N >= 1) writes the files through the device encode path: PNG row filters on the GPU, N threads that
deflate at --level L (6) and write; the default and --host_encode: the host's writers, one file after another.
--device_deflate (with --workers N): the GPU deflates the scanlines too and the threads only write."""
import argparse
import os
import shutil
import sys

VARIANTS = ('train_2012', 'train_2015', 'test_2012', 'test_2015')
UNSUPPORTED = {'output_visual': "--output_visual is not supported here: python -m unflow_amd.visualize writes the colour-wheel / "
                                "error images"}


def parser():
    ap = argparse.ArgumentParser(prog='python -m unflow_amd.evaluate', description=__doc__.split('\n')[0])
    ap.add_argument('--ex', required=True, help='experiment name')
    ap.add_argument('--dataset', default='kitti', help="only 'kitti' (sintel / chairs / mdb: python -m unflow_amd.evaluate_flo)")
    ap.add_argument('--variant', default='train_2012', choices=VARIANTS)
    ap.add_argument('--num', type=int, default=10, help='examples to evaluate; -1: all (eval_gui.py --num)')
    ap.add_argument('--output_benchmark', action='store_true', help='write the benchmark flow files')
    ap.add_argument('--output_png', action='store_true', help='KITTI 16-bit PNG files (default: .flo)')
    ap.add_argument('--output_visual', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--output_backward', action='store_true',
                    help='with --output_benchmark: also write the backward flow (%%06d_01.png / .flo)')
    ap.add_argument('--occlusion', action='store_true',
                    help='forward-backward occlusion: scores on train_* variants, %%06d_10_occ.png with --output_benchmark')
    ap.add_argument('--batch_size', type=int, default=4, help='pairs per graph replay')
    ap.add_argument('--host_decode', action='store_true',
                    help="decode the PNG files with the host's decoder (slow) instead of the library's PNG kernels")
    add_encode_flags(ap)
    ap.add_argument('--config', default='../config.ini', help='the project config.ini (dirs: data, log, checkpoints)')
    ap.add_argument('--out', default='../out', help='output root: files go to <out>/<ex>/')
    ap.add_argument('--dims', type=int, nargs=2, default=(384, 1280), metavar=('H', 'W'),
                    help='network input size (eval_gui.py: 384 1280)')
    return ap


def add_encode_flags(ap):
    """The output flags the file-writing commands share (evaluate, evaluate_flo, visualize, sequence)."""
    ap.add_argument('--workers', type=int, default=0, metavar='N',
                    help='N >= 1: write the output files through the device encode path, the PNG filter kernel and N threads '
                         'that deflate and write (at most 16; 8 is a good value); 0, the default: the host writers')
    ap.add_argument('--level', type=int, default=6, metavar='L', help='deflate level of the PNG files, 0 .. 9')
    ap.add_argument('--host_encode', action='store_true',
                    help="write the files one after another with the host's PNG writers (filter 0), whatever --workers says")
    ap.add_argument('--device_deflate', action='store_true',
                    help='with --workers N >= 1: deflate the PNG scanlines on the GPU as well (DESIGN 7.12); the N threads only '
                         'form the chunk CRCs and write, and --level does not apply')


def check_encode_flags(ap, a):
    """Refuses a bad --workers / --level / --device_deflate (status 2); a.encode_workers: FlowEstimator.export's workers (0 with
    --host_encode), a.deflate: its deflate ('device' with --device_deflate)."""
    if a.workers < 0:
        ap.error("--workers must not be negative (0: the host's writers)")
    if not 0 <= a.level <= 9:
        ap.error("--level must be in 0 .. 9, got %d" % a.level)
    a.encode_workers = 0 if a.host_encode else a.workers
    if a.device_deflate and a.encode_workers < 1:
        ap.error("--device_deflate feeds the writer pool: it needs --workers N with N >= 1 (and no --host_encode)")
    a.deflate = 'device' if a.device_deflate else 'host'


def parse_args(argv=None):
    """Parsed flags; refuses what this tool does not do with a clear message (SystemExit, status 2)."""
    ap = parser()
    a = ap.parse_args(argv)
    check_encode_flags(ap, a)
    if a.dataset != 'kitti':
        ap.error("--dataset %s is not supported here (only kitti; python -m unflow_amd.evaluate_flo scores and draws sintel / "
                 "chairs / mdb)" % a.dataset)
    for k, msg in UNSUPPORTED.items():
        if getattr(a, k):
            ap.error(msg)
    if a.output_backward and not a.output_benchmark:      # eval_gui.py reads the flag inside its output_benchmark branch
        ap.error("--output_backward requires --output_benchmark")
    if a.batch_size <= 0:
        ap.error("--batch_size must be positive")
    return a


def experiment_paths(name, config_path):
    """(experiment config path, checkpoint directory) as eval_gui.py:101-117 finds them: the experiment's own config.ini when
    its logs folder has one (else the project config), and its logs folder when it holds a checkpoint (else
    <dirs.checkpoints>/<name>)."""
    from .core import tf_checkpoint as T
    from .core.util import config_dict
    dirs = config_dict(config_path).get('dirs', {})
    exp_dir = os.path.join(dirs.get('log', ''), 'ex', name)
    cfg = os.path.join(exp_dir, 'config.ini')
    if not os.path.isfile(cfg):
        cfg = config_path
    if not os.path.isdir(exp_dir) or T.latest_checkpoint(exp_dir) is None:
        exp_dir = os.path.join(dirs.get('checkpoints', ''), name)
    if T.latest_checkpoint(exp_dir) is None:
        raise SystemExit("Error: experiment must contain a checkpoint (looked in %s)" % exp_dir)
    return cfg, exp_dir


from .data import Data as _KITTIData      # the data root alone (dirs.data)       # noqa: E402


def main(argv=None):
    a = parse_args(argv)
    from .core.util import config_dict, convert_input_strings
    from .core.inference import OCC_NAMES, FlowEstimator
    from .kitti.input import KITTIInput
    cfg_path, ckpt_dir = experiment_paths(a.ex, a.config)
    config = config_dict(cfg_path)
    params = dict(config.get('train', {}))
    dirs = config_dict(a.config).get('dirs', {})
    convert_input_strings(params, dirs)
    params.update(config.get('train_' + a.dataset, {}))
    est = FlowEstimator.from_checkpoint(ckpt_dir, params, a.batch_size, net_size=tuple(a.dims),
                                        bidirectional=a.output_backward or a.occlusion)
    kinput = KITTIInput(_KITTIData(dirs.get('data', '')), batch_size=a.batch_size, normalize=False, dims=tuple(a.dims))
    dev = None if a.host_decode else est.dev          # the PNG files decoded by the library's kernels (core/png_device.py)
    batches = lambda: getattr(kinput, 'input_' + a.variant)(device=dev)            # noqa: E731
    num = None if a.num < 0 else a.num
    print("-- evaluating %s (step %s) on kitti %s" % (a.ex, est.global_step, a.variant))
    if a.variant.startswith('train'):
        res = est.evaluate(batches(), num=num)
        names = res['names'] + [k for k in OCC_NAMES if a.occlusion and k in res]
        for k in names:
            print("%-24s %.4f" % (k, res[k]))
        print("examples: %d" % res['num_examples'])
    if a.output_benchmark:
        out_dir = os.path.join(a.out, a.ex)
        if os.path.isdir(out_dir):
            shutil.rmtree(out_dir)
        os.makedirs(out_dir)
        shutil.copyfile(cfg_path, os.path.join(out_dir, 'config.ini'))
        paths = est.export(batches(), out_dir, fmt='png' if a.output_png else 'flo', num=num, backward=a.output_backward,
                           occlusion=a.occlusion, workers=a.encode_workers, level=a.level, deflate=a.deflate)
        print("wrote %d files to %s" % (len(paths), out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
