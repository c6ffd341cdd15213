"""python -m unflow_amd.run: train an experiment — the reference's src/run.py on core/train.Trainer, with the evaluation after
every chunk (train.py:142) and the TensorBoard summaries of core/summary.py.

    python -m unflow_amd.run --ex NAME [--dataset {chairs,kitti,cityscapes,synthia,kitti_ft}] [--ow] [--debug]
                             [--iters N] [--batch_size B] [--no_eval] [--kitti_excludes DIR] [--host_decode] [--config PATH]

--dataset defaults to [run] dataset of the experiment's config, else kitti (run.py:51).  Params = [train] updated by
[train_<dataset>], then convert_input_strings (run.py:63-65); --iters defaults to num_iters, --batch_size to [run] batch_size.
Per dataset (run.py:62-197; the frames' directories are unflow_amd/data.py's):
  chairs      ChairsInput(dims = (height, width), normalize = False).input_raw(swap_images = False, shift)
  kitti       KITTIInput(..., skipped_frames = True).input_raw(swap_images = False, center_crop = True, shift)
  cityscapes  KITTIInput(..., skipped_frames = False).input_raw(swap_images = False, center_crop = True, skip = [0, 1], shift)
  synthia     KITTIInput(...).input_raw(swap_images = False, shift)
  kitti_ft    Trainer(supervised = True) on finetune.py's KITTIInput.input_train_gt(40, shift) batches
with shift = (steps already trained) x batch_size.  Batches are decoded on the device (core/png_device.py) unless --host_decode.
Trainer.run trains from step 0 to --iters in chunks of save_interval, a checkpoint after each, and resumes from the latest
checkpoint of the experiment; the final checkpoint is kept with the experiment's logs (Experiment.conclude).

After every chunk the checkpoint is evaluated (Trainer.eval) on KITTIInput(batch_size = 1, normalize = False, dims = (384, 1280))
.input_train_2012() — kitti_ft: input_train_2015(40) — and AEE / outliers (occluded, non-occluded) and the averaged loss tags go
to <experiment>/eval.  When that KITTI tree is absent (the reference would download it) evaluation is skipped with one warning;
--no_eval skips it silently.  At i == 1 and every display_interval, where the loss is synchronised anyway, <experiment>/train gets
loss/combined, loss/<term> for all eight terms, loss<k>/<term> per level, weight/<term> and train/learning_rate (kitti_ft:
loss/combined and train/learning_rate), read with FlowNetEngine.loss_terms().

--kitti_excludes DIR: the benchmark frames named by the *.txt lists of DIR (the format of UnFlow's files/kitti_excludes, not
shipped) and their neighbours are left out of the kitti_raw listings (unflow_amd/data.py).  Without it --dataset kitti warns
once that benchmark frames are not excluded.

Deviation from the reference: --debug disables neither the checkpoints nor conclude(); it only adds the image summaries
train/augmented1/image/<n>, train/augmented2/image/<n> (n < min(B, 3): the network input with the channel mean added back,
x 255, clipped).  One process, one GPU: WORLD_SIZE > 1 is refused (sharding the example list over ranks is not built)."""
import argparse
import os
import sys

DATASETS = ('chairs', 'kitti', 'cityscapes', 'synthia', 'kitti_ft')
EVAL_DIMS = (384, 1280)      # run.py:57-60
FT_HOLD_OUT = 40             # run.py:185-186
NO_EXCLUDES_WARNING = ("Warning: --kitti_excludes not given: the frames of the KITTI 2012 / 2015 benchmark pairs are NOT excluded "
                       "from kitti_raw")


def parser():
    ap = argparse.ArgumentParser(prog='python -m unflow_amd.run', description=__doc__.split('\n')[0])
    ap.add_argument('--ex', required=True, help='experiment name; an existing experiment continues from its latest checkpoint')
    ap.add_argument('--dataset', default=None, choices=DATASETS, help='default: dataset of [run], else kitti')
    ap.add_argument('--ow', action='store_true', help='overwrite the experiment (run.py --ow)')
    ap.add_argument('--debug', action='store_true', help='add image summaries of the network input')
    ap.add_argument('--iters', type=int, default=None, help='train up to this step (default: num_iters of the config)')
    ap.add_argument('--batch_size', type=int, default=None, help='pairs per step (default: batch_size of [run])')
    ap.add_argument('--no_eval', action='store_true', help='no evaluation after the chunks')
    ap.add_argument('--kitti_excludes', default=None, metavar='DIR', help='folder of KITTI benchmark exclude lists (*.txt)')
    ap.add_argument('--host_decode', action='store_true',
                    help="read the files with the host's decoders (slow) instead of the library's kernels")
    ap.add_argument('--config', default='../config.ini', help='the project config.ini (dirs: data, log, checkpoints)')
    return ap


def parse_args(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.iters is not None and a.iters <= 0:
        ap.error("--iters must be positive")
    if a.batch_size is not None and a.batch_size <= 0:
        ap.error("--batch_size must be positive")
    return a


def refuse_multi_rank(environ=None):
    environ = os.environ if environ is None else environ
    if int(environ.get('WORLD_SIZE', '1') or 1) > 1:
        raise SystemExit("Error: python -m unflow_amd.run trains on one GPU; WORLD_SIZE = %s (sharding the example list over "
                         "ranks is not built)" % environ['WORLD_SIZE'])


def dataset_of(flag, config):
    """--dataset, else [run] dataset, else kitti (run.py:51)."""
    name = flag or config.get('run', {}).get('dataset', 'kitti')
    if name not in DATASETS:
        raise SystemExit("Error: invalid dataset %r: must be one of %s" % (name, ', '.join(DATASETS)))
    return name


def run_params(config, dataset):
    """[train] updated by [train_<dataset>] (run.py:63-64 and its four siblings)."""
    params = dict(config.get('train', {}))
    params.update(config.get('train_' + dataset, {}))
    return params


def dataset_data(dataset, root, kitti_excludes=None):
    from . import data as D
    if dataset in ('kitti', 'kitti_ft'):
        return D.KITTIData(root, exclude_lists_dir=kitti_excludes if dataset == 'kitti' else None)
    return {'chairs': D.ChairsData, 'cityscapes': D.CityscapesData, 'synthia': D.SynthiaData}[dataset](root)


def training_batches(dataset, data, batch_size, dims, kitti_input=None, chairs_input=None):
    """(shift in steps, device) -> the batch iterator of the dataset's run.py branch.  kitti_input / chairs_input: the input
    classes (default: the package's)."""
    kw = dict(batch_size=batch_size, normalize=False, dims=tuple(dims))
    if dataset == 'kitti_ft':
        from .finetune import dataset_batches
        return dataset_batches(argparse.Namespace(dataset='kitti'), data.current_dir, batch_size, dims)
    if dataset == 'chairs':
        if chairs_input is None:
            from .chairs.input import ChairsInput as chairs_input
        inp, ctor, raw, listing = chairs_input, {}, {}, dict(sequence=False)
    else:
        if kitti_input is None:
            from .kitti.input import KITTIInput as kitti_input
        inp = kitti_input
        ctor, raw = {'kitti': (dict(skipped_frames=True), dict(center_crop=True)),
                     'cityscapes': (dict(skipped_frames=False), dict(center_crop=True, skip=[0, 1])),
                     'synthia': ({}, {})}[dataset]
        listing = {k: v for k, v in raw.items() if k == 'skip'}
    inp = inp(data, **ctor, **kw)

    def batches(shift, device):
        return inp.input_raw(swap_images=False, shift=shift * batch_size, device=device, **raw)
    batches.pair_list = lambda: inp.raw_pairs(swap_images=False, **listing)       # the example list at shift 0
    return batches


def eval_batches(dataset, root):
    """device -> the evaluation batches of run.py:57-60,78,186, or None when the KITTI tree they read is absent."""
    from .data import KITTIData
    from .kitti.input import KITTIInput
    einput = KITTIInput(KITTIData(root), batch_size=1, normalize=False, dims=EVAL_DIMS)
    if dataset == 'kitti_ft':
        tree, fn = 'data_scene_flow/training', lambda device: einput.input_train_2015(FT_HOLD_OUT, device=device)
    else:
        tree, fn = 'data_stereo_flow/training', lambda device: einput.input_train_2012(device=device)
    return fn if os.path.isdir(os.path.join(root, tree)) else None


def network_input_images(engine, n_max=3):
    """{'train/augmented<1|2>/image/<n>': uint8 [H,W,3]} of the step's network input: mean added back, x 255, clipped."""
    import torch
    from .core.engine import CHANNEL_MEAN
    B = engine.B
    mean = torch.tensor(CHANNEL_MEAN, dtype=torch.float32, device=engine.dev) / 255.0
    out = {}
    for k, rows in ((1, engine.x0[:B]), (2, engine.x0[B:2 * B])):
        im = ((rows[:min(B, n_max), :, :, :3] + mean) * 255.0).clamp(0, 255).round().to(torch.uint8).cpu().numpy()
        out.update({'train/augmented%d/image/%d' % (k, n): im[n] for n in range(im.shape[0])})
    return out


def train_scalars(loss, trainer):
    """The scalars of one display step under the reference's tags (unsupervised.py:139-159, train.py:194)."""
    from .core.engine import LOSSES
    from .core.train import term_tags
    scalars = {'loss/combined': loss}
    if not trainer.supervised:
        scalars.update(term_tags(trainer.engine.loss_terms()))
        scalars.update({'weight/' + k: float(trainer.params[k + '_weight']) for k in LOSSES if trainer.params.get(k + '_weight')})
    scalars['train/learning_rate'] = trainer.last_lr
    return scalars


def main(argv=None):
    a = parse_args(argv)
    refuse_multi_rank()
    from .core.util import config_dict, convert_input_strings
    from .experiment import Experiment
    experiment = Experiment(a.ex, overwrite=a.ow, config_path=a.config)
    dirs = config_dict(a.config).get('dirs', {})
    run_config = experiment.config.get('run', {})
    dataset = dataset_of(a.dataset, experiment.config)
    params = run_params(experiment.config, dataset)
    convert_input_strings(params, dirs)
    batch_size = a.batch_size or run_config.get('batch_size')
    if not batch_size:
        raise SystemExit("Error: give --batch_size or batch_size in [run] of the config")
    iters = a.iters or params.get('num_iters', 0)
    if iters <= 0:
        raise SystemExit("Error: nothing to do: give --iters or num_iters in the config")
    dims = (params['height'], params['width'])
    root = dirs.get('data', '')
    if dataset == 'kitti' and not a.kitti_excludes:
        print(NO_EXCLUDES_WARNING)
    batches = training_batches(dataset, dataset_data(dataset, root, a.kitti_excludes), batch_size, dims)
    if hasattr(batches, 'pair_list'):
        # the example list the run walks (before `shift`), kept with the logs: which frames were trained on
        pairs = batches.pair_list()
        with open(os.path.join(experiment.log_dir, 'train_pairs.txt'), 'w') as f:
            f.writelines("%s %s\n" % pr for pr in pairs)
        print("-- %d frame pairs listed in %s" % (len(pairs), os.path.join(experiment.log_dir, 'train_pairs.txt')))
    evaluation = None if a.no_eval else eval_batches(dataset, root)
    if evaluation is None and not a.no_eval:
        print("Warning: no KITTI evaluation data under %s: the checkpoints are not evaluated" % root)

    from .core.summary import SummaryWriter
    from .core.train import Trainer
    tr = Trainer(batch_size, dims[0], dims[1], params, supervised=dataset == 'kitti_ft')
    dev = None if a.host_decode else tr.engine.dev
    print("-- training %s on %s: %d x %d, batch %d" % (a.ex, dataset, dims[0], dims[1], batch_size))
    train_writer = SummaryWriter(experiment.train_dir)
    eval_writer = SummaryWriter(experiment.eval_dir) if evaluation is not None else None

    def on_display(i, loss, trainer):
        train_writer.add_scalars(i, train_scalars(loss, trainer))
        if a.debug:
            train_writer.add_images(i, network_input_images(trainer.engine))

    def eval_fn(i):
        res = tr.eval(lambda: evaluation(dev), experiment.save_dir, terms=True)
        tags = [k for k in res['names'] if k != 'loss'] + list(res['term_names'])
        scalars = {k: res[k] for k in tags}
        scalars['loss/combined'] = res['loss']
        eval_writer.add_scalars(res['global_step'], scalars)
        print("-- eval: " + ", ".join("%s = %.4f" % (k, res[k]) for k in res['names']))

    try:
        tr.run(0, iters, lambda shift: batches(shift, dev), experiment.save_dir,
               eval_fn=eval_fn if evaluation is not None else None, on_display=on_display)
    finally:
        train_writer.close()
        if eval_writer is not None:
            eval_writer.close()
    experiment.conclude()
    return 0


if __name__ == '__main__':
    sys.exit(main())
