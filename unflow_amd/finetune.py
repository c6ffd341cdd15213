"""python -m unflow_amd.finetune: supervised fine-tuning of an experiment on ground-truth flow — the `kitti_ft` branch of the
reference's src/run.py (:175-190), and the same for the dense .flo datasets (this project's addition).

    python -m unflow_amd.finetune --ex NAME --dataset {kitti,sintel,chairs} [--variant clean|final] [--gt occ|noc]
                                  [--geometric] [--iters N] [--batch_size B] [--dims H W] [--host_decode] [--ow] [--config PATH]

Params = the experiment's [train] section updated by [train_<dataset>_ft] when the config has one ([train_kitti_ft] is the
reference's; finetune = <experiment names> there names the networks to start from).  Trainer(supervised=True) then runs from
step 0 to --iters (default: num_iters) in chunks of save_interval, a checkpoint after each chunk in <dirs.checkpoints>/NAME, and
resumes from the latest checkpoint found there, like the reference; the final checkpoint is kept with the experiment's logs.
  kitti   KITTIInput.input_train_gt(40): 2015 + 2012 pairs with their flow_occ maps (run.py:185)
  sintel  SintelInput.input_train_gt(--variant clean (default) | final, --gt occ (default) | noc)
  chairs  ChairsInput.input_train_gt(): flying_chairs/image with the .flo files of flying_chairs/train_flow
--geometric turns params['augment_geometric'] on: image pair and ground truth are transformed together (on kitti with
gt_sampling = 'nearest', the sparse maps; a [train_*_ft] gt_sampling key wins).  The batches are decoded on the device
(core/png_device.py) unless --host_decode.  The unsupervised datasets of run.py, summaries and evaluation during training are
python -m unflow_amd.run's (its kitti_ft branch takes this module's batches)."""
import argparse
import sys

DATASETS = ('kitti', 'sintel', 'chairs')
KITTI_HOLD_OUT = 40          # run.py:185


def parser():
    ap = argparse.ArgumentParser(prog='python -m unflow_amd.finetune', description=__doc__.split('\n')[0])
    ap.add_argument('--ex', required=True, help='experiment name')
    ap.add_argument('--dataset', required=True, choices=DATASETS)
    ap.add_argument('--variant', default=None, choices=('clean', 'final'), help='sintel: the pass (default clean)')
    ap.add_argument('--gt', default=None, choices=('occ', 'noc'), help='sintel: the ground-truth map (default occ)')
    ap.add_argument('--geometric', action='store_true', help='geometric augmentation of image pair and ground truth')
    ap.add_argument('--iters', type=int, default=None, help='train up to this step (default: num_iters of the config)')
    ap.add_argument('--batch_size', type=int, default=None, help='pairs per step (default: batch_size of [run], else 4)')
    ap.add_argument('--dims', type=int, nargs=2, default=None, metavar=('H', 'W'), help='crop size (default: height, width of the config)')
    ap.add_argument('--host_decode', action='store_true',
                    help="read the files with the host's decoders (slow) instead of the library's kernels")
    ap.add_argument('--ow', action='store_true', help='overwrite the experiment (run.py --ow)')
    ap.add_argument('--config', default='../config.ini', help='the project config.ini (dirs: data, log, checkpoints)')
    return ap


def parse_args(argv=None):
    """Parsed flags with the dataset's defaults filled in (sintel: variant clean, gt occ); refuses contradictions with a clear
    message (SystemExit, status 2)."""
    ap = parser()
    a = ap.parse_args(argv)
    if a.dataset == 'sintel':
        a.variant = a.variant or 'clean'
        a.gt = a.gt or 'occ'
    else:
        if a.variant is not None:
            ap.error("--variant is for --dataset sintel")
        if a.gt is not None:
            ap.error("--gt is for --dataset sintel (kitti trains on flow_occ, chairs has one map)")
    if a.iters is not None and a.iters <= 0:
        ap.error("--iters must be positive")
    if a.batch_size is not None and a.batch_size <= 0:
        ap.error("--batch_size must be positive")
    if a.dims is not None:
        a.dims = tuple(a.dims)
        if any(d <= 0 or d % 64 for d in a.dims):
            ap.error("--dims must be positive multiples of 64 (the network's input size)")
    return a


from .data import Data as _Data      # the data root alone (dirs.data)       # noqa: E402


def finetune_params(config, dataset, geometric):
    """[train] updated by [train_<dataset>_ft] (run.py:176-177), plus what --geometric sets."""
    params = dict(config.get('train', {}))
    params.update(config.get('train_%s_ft' % dataset, {}))
    if geometric:
        params['augment_geometric'] = True
        if dataset == 'kitti':
            params.setdefault('gt_sampling', 'nearest')
    return params


def dataset_batches(a, root, batch_size, dims):
    """shift -> the iterator of (im1, im2, flow_gt, mask_gt) batches, `shift` steps into the example list."""
    data = _Data(root)
    kw = dict(batch_size=batch_size, normalize=False, dims=tuple(dims))
    if a.dataset == 'kitti':
        from .kitti.input import KITTIInput
        inp = KITTIInput(data, **kw)
        return lambda shift, device: inp.input_train_gt(KITTI_HOLD_OUT, shift=shift * batch_size, device=device)
    if a.dataset == 'sintel':
        from .sintel.input import SintelInput
        inp = SintelInput(data, **kw)
        return lambda shift, device: inp.input_train_gt(variant=a.variant, gt=a.gt, shift=shift * batch_size, device=device)
    from .chairs.input import ChairsInput
    inp = ChairsInput(data, **kw)
    return lambda shift, device: inp.input_train_gt(shift=shift * batch_size, device=device)


def main(argv=None):
    a = parse_args(argv)
    from .core.train import Trainer
    from .core.util import config_dict, convert_input_strings
    from .experiment import Experiment
    experiment = Experiment(a.ex, overwrite=a.ow, config_path=a.config)
    dirs = config_dict(a.config).get('dirs', {})
    params = finetune_params(experiment.config, a.dataset, a.geometric)
    convert_input_strings(params, dirs)
    batch_size = a.batch_size or experiment.config.get('run', {}).get('batch_size') or 4
    dims = a.dims or (params['height'], params['width'])
    iters = a.iters or params.get('num_iters', 0)
    if iters <= 0:
        raise SystemExit("Error: nothing to do: give --iters or num_iters in the config")
    batches = dataset_batches(a, dirs.get('data', ''), batch_size, dims)
    tr = Trainer(batch_size, dims[0], dims[1], params, supervised=True)
    dev = None if a.host_decode else tr.engine.dev
    print("-- fine-tuning %s on %s%s: %d x %d, batch %d%s" % (a.ex, a.dataset, ' %s %s' % (a.variant, a.gt) if a.dataset == 'sintel' else '',
                                                           dims[0], dims[1], batch_size, ', geometric augmentation' if a.geometric else ''))
    tr.run(0, iters, lambda shift: batches(shift, dev), experiment.save_dir)
    experiment.conclude()
    return 0


if __name__ == '__main__':
    sys.exit(main())
