"""python -m unflow_amd.run without a GPU: the dataset directory conventions of unflow_amd/data.py, the KITTI benchmark exclusion,
parameter merging and the per-dataset input arguments (recorded through a stub input).  Trees of empty files: nothing is decoded."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXCLUDES = os.path.join(HERE, 'golden', 'kitti_excludes')


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'wb').close()


def _tree_state(root):
    return sorted((os.path.join(d, f), os.path.getsize(os.path.join(d, f))) for d, _, files in os.walk(str(root)) for f in files)


# ---------------------------------------------------------------------------------------------------- directory conventions
def test_raw_dirs_of_the_four_layouts_sorted(tmp_path):
    from unflow_amd import data as D
    root = str(tmp_path)
    for date, drive in (('2011_09_28', '2011_09_28_drive_0002_extract'), ('2011_09_26', '2011_09_26_drive_0009_sync'),
                        ('2011_09_26', '2011_09_26_drive_0001_extract')):
        for view in ('image_03', 'image_02'):
            _touch(os.path.join(root, 'kitti_raw', date, drive, view, 'data', '0000000000.png'))
    j = lambda *p: os.path.join(root, *p)
    assert D.KITTIData(root).get_raw_dirs() == [
        j('kitti_raw', '2011_09_26', '2011_09_26_drive_0001_extract', 'image_02', 'data'),
        j('kitti_raw', '2011_09_26', '2011_09_26_drive_0001_extract', 'image_03', 'data'),
        j('kitti_raw', '2011_09_26', '2011_09_26_drive_0009_sync', 'image_02', 'data'),
        j('kitti_raw', '2011_09_26', '2011_09_26_drive_0009_sync', 'image_03', 'data'),
        j('kitti_raw', '2011_09_28', '2011_09_28_drive_0002_extract', 'image_02', 'data'),
        j('kitti_raw', '2011_09_28', '2011_09_28_drive_0002_extract', 'image_03', 'data')]
    for seq, view in (('SEQS-02-SUMMER', 'Omni_R'), ('SEQS-02-SUMMER', 'Omni_B'), ('SEQS-01-DAWN', 'Omni_F')):
        _touch(j('synthia', seq, seq, 'RGB', 'Stereo_Left', view, '000000.png'))
    assert D.SynthiaData(root).get_raw_dirs() == [
        j('synthia', 'SEQS-01-DAWN', 'SEQS-01-DAWN', 'RGB', 'Stereo_Left', 'Omni_F'),
        j('synthia', 'SEQS-02-SUMMER', 'SEQS-02-SUMMER', 'RGB', 'Stereo_Left', 'Omni_B'),
        j('synthia', 'SEQS-02-SUMMER', 'SEQS-02-SUMMER', 'RGB', 'Stereo_Left', 'Omni_R')]
    for split, city in (('val', 'munster'), ('train', 'zurich'), ('train', 'aachen')):
        _touch(j('cs', 'leftImg8bit_sequence_trainvaltest', split, city, 'a_000000_000000_leftImg8bit.png'))
    top = j('cs', 'leftImg8bit_sequence_trainvaltest')
    assert D.CityscapesData(root).get_raw_dirs() == [os.path.join(top, 'train', 'aachen'), os.path.join(top, 'train', 'zurich'),
                                                     os.path.join(top, 'val', 'munster')]
    _touch(j('flying_chairs', 'image', '00001_img1.png'))
    assert D.ChairsData(root).get_raw_dirs() == [j('flying_chairs', 'image')]
    assert D.ChairsData(root).current_dir == root and D.Data(root).get_raw_dirs() == []


@pytest.mark.parametrize("cls,looked_for", [('KITTIData', 'kitti_raw'), ('SynthiaData', 'synthia'),
                                            ('CityscapesData', os.path.join('cs', 'leftImg8bit_sequence_trainvaltest')),
                                            ('ChairsData', os.path.join('flying_chairs', 'image'))])
def test_missing_root_names_the_directory(tmp_path, cls, looked_for):
    from unflow_amd import data as D
    with pytest.raises(RuntimeError) as err:
        getattr(D, cls)(str(tmp_path)).get_raw_dirs()
    assert os.path.join(str(tmp_path), looked_for) in str(err.value)


# ---------------------------------------------------------------------------------------------------- benchmark exclusion
def _kitti_raw(root, drives):
    """drives: {(date, drive dir): frame numbers}; image_02 and image_03 get the same frames."""
    for (date, drive), frames in drives.items():
        for view in ('image_02', 'image_03'):
            for n in frames:
                _touch(os.path.join(str(root), 'kitti_raw', date, drive, view, 'data', '%010d.png' % n))


def test_exclude_list_format():
    """The three-line list: a _10 line (counts), its _11 line (ignored), a _10 line of another date's drive."""
    from unflow_amd.data import read_kitti_excludes
    assert read_kitti_excludes(EXCLUDES) == {('2011_09_26', '2011_09_26_drive_0005'): [20], ('2011_09_29', '2011_09_29_drive_0071'): [3]}
    with pytest.raises(RuntimeError, match='nowhere'):
        read_kitti_excludes(os.path.join(EXCLUDES, 'nowhere'))


def test_exclusion_rule(tmp_path):
    from unflow_amd.core.input import Input, frame_name_to_num
    from unflow_amd.data import KITTIData
    gaps = [n for n in range(41) if n not in (5, 6, 36)]                 # a drive with dropped frames
    _kitti_raw(tmp_path, {('2011_09_26', '2011_09_26_drive_0005_extract'): gaps,
                          ('2011_09_26', '2011_09_26_drive_0011_extract'): range(41),
                          ('2011_09_29', '2011_09_29_drive_0071_sync'): range(20)})
    before = _tree_state(tmp_path)
    data = KITTIData(str(tmp_path), exclude_lists_dir=EXCLUDES)
    plain = KITTIData(str(tmp_path))
    dirs = data.get_raw_dirs()
    assert dirs == plain.get_raw_dirs() and len(dirs) == 6
    for folder in dirs:
        kept = [frame_name_to_num(f) for f in data.list_frames(folder)]
        everything = [frame_name_to_num(f) for f in plain.list_frames(folder)]
        if 'drive_0005' in folder:                                        # frame 20 named: [10, 32) gone, in both views
            assert kept == [n for n in gaps if n < 10 or n >= 32]
        elif 'drive_0071' in folder:                                      # the _sync directory is the one present: frame 3 named
            assert kept == list(range(15, 20))
        else:
            assert kept == everything == list(range(41))                  # other drives untouched (the _11 line names 0011's frame 21)
    pairs = Input(data, batch_size=1, dims=(8, 8), skipped_frames=True).raw_pairs(swap_images=False)
    for a, b in pairs:
        na, nb = frame_name_to_num(os.path.basename(a)), frame_name_to_num(os.path.basename(b))
        assert nb - na == 1 and os.path.dirname(a) == os.path.dirname(b)      # no pair straddles the hole (9 -> 32) or a gap
        if 'drive_0005' in a:
            assert not (10 <= na < 32 or 10 <= nb < 32)
    n_0005 = sum('drive_0005' in a and 'image_02' in a for a, _ in pairs)
    assert n_0005 == len([n for n in range(9) if n not in (4, 5, 6)]) + len([n for n in range(32, 40) if n not in (35, 36)])
    unfiltered = Input(plain, batch_size=1, dims=(8, 8), skipped_frames=True).raw_pairs(swap_images=False)
    assert len(unfiltered) > len(pairs)
    assert _tree_state(tmp_path) == before                                # nothing on disk changed


# ---------------------------------------------------------------------------------------------------- the command's plumbing
def test_params_merge_and_dataset_fallback():
    from unflow_amd import run as R
    config = {'train': {'height': 320, 'width': 1152, 'fb_weight': 0.0, 'num_iters': 10},
              'train_kitti': {'fb_weight': 0.2, 'mask_occlusion': 'fb'}, 'train_chairs': {'height': 384},
              'run': {'dataset': 'synthia', 'batch_size': 4}}
    kitti = R.run_params(config, 'kitti')
    assert kitti == {'height': 320, 'width': 1152, 'fb_weight': 0.2, 'num_iters': 10, 'mask_occlusion': 'fb'}
    assert R.run_params(config, 'chairs')['height'] == 384 and config['train']['height'] == 320
    assert R.run_params(config, 'cityscapes') == config['train']
    assert R.dataset_of(None, config) == 'synthia'                        # [run] dataset
    assert R.dataset_of('chairs', config) == 'chairs'                     # the flag wins
    assert R.dataset_of(None, {'run': {}}) == 'kitti' and R.dataset_of(None, {}) == 'kitti'
    with pytest.raises(SystemExit):
        R.dataset_of(None, {'run': {'dataset': 'sintel'}})
    a = R.parse_args(['--ex', 'x'])
    assert a.dataset is None and not a.ow and not a.debug and not a.no_eval and a.kitti_excludes is None
    with pytest.raises(SystemExit):
        R.parse_args(['--ex', 'x', '--dataset', 'sintel'])
    with pytest.raises(SystemExit):
        R.parse_args(['--ex', 'x', '--iters', '0'])


class _StubInput:
    log = []

    def __init__(self, data, **kw):
        self.kw = kw
        _StubInput.log.append(('init', type(data).__name__, kw))

    def input_raw(self, **kw):
        _StubInput.log.append(('input_raw', kw))
        return iter(())

    def input_train_gt(self, *args, **kw):
        _StubInput.log.append(('input_train_gt', args, kw))
        return iter(())


EXPECTED = {
    'chairs': ('ChairsData', {}, dict(swap_images=False)),
    'kitti': ('KITTIData', dict(skipped_frames=True), dict(swap_images=False, center_crop=True)),
    'cityscapes': ('CityscapesData', dict(skipped_frames=False), dict(swap_images=False, center_crop=True, skip=[0, 1])),
    'synthia': ('SynthiaData', {}, dict(swap_images=False)),
}


@pytest.mark.parametrize("dataset", sorted(EXPECTED))
def test_input_arguments_per_dataset(dataset, tmp_path):
    from unflow_amd import run as R
    data_cls, ctor, raw = EXPECTED[dataset]
    _StubInput.log = []
    data = R.dataset_data(dataset, str(tmp_path))
    batches = R.training_batches(dataset, data, 4, (320, 1152), kitti_input=_StubInput, chairs_input=_StubInput)
    batches(0, None)
    batches(7, 'cuda:0')
    common = dict(batch_size=4, normalize=False, dims=(320, 1152))
    assert _StubInput.log == [('init', data_cls, dict(common, **ctor)),
                              ('input_raw', dict(raw, shift=0, device=None)),
                              ('input_raw', dict(raw, shift=28, device='cuda:0'))]       # shift = iteration offset x batch size


def test_kitti_ft_takes_finetunes_batches(tmp_path, monkeypatch):
    import unflow_amd.kitti.input as KI
    from unflow_amd import run as R
    monkeypatch.setattr(KI, 'KITTIInput', _StubInput)
    _StubInput.log = []
    data = R.dataset_data('kitti_ft', str(tmp_path), kitti_excludes=EXCLUDES)
    assert data.excluded == {}                                            # the lists are for kitti_raw only
    batches = R.training_batches('kitti_ft', data, 2, (320, 1152))
    batches(3, None)
    assert _StubInput.log == [('init', 'Data', dict(batch_size=2, normalize=False, dims=(320, 1152))),
                              ('input_train_gt', (40,), dict(shift=6, device=None))]


def test_trainer_run_hands_the_iteration_offset_to_the_batches():
    """Trainer.run calls train_batch_fn(steps already trained): with a checkpoint at step 4 of a run from 0 the offset is 4, so the
    command's shift is 4 x batch_size.  Checked on the arithmetic of Trainer.run with the training itself stubbed out."""
    from unflow_amd.core.train import Trainer
    tr = Trainer.__new__(Trainer)
    tr.params = {'save_interval': 2}
    calls = []
    tr.checkpoint_step = lambda d: 4
    tr.restore = lambda d: None
    tr.train = lambda s, e, off, fn, d, on_display=None: calls.append((s, e, off, on_display)) or []
    hook = object()
    tr.run(0, 8, None, 'nowhere', on_display=hook)
    assert calls == [(5, 6, 4, hook), (7, 8, 6, hook)]


def test_world_size_is_refused(monkeypatch):
    from unflow_amd import run as R
    R.refuse_multi_rank({})
    R.refuse_multi_rank({'WORLD_SIZE': '1'})
    with pytest.raises(SystemExit, match='WORLD_SIZE'):
        R.refuse_multi_rank({'WORLD_SIZE': '2'})
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit, match='one GPU'):
        R.main(['--ex', 'never_created', '--config', os.path.join(HERE, 'no_such_config.ini')])


def _config(tmp_path, extra=''):
    cfg = tmp_path / 'config.ini'
    cfg.write_text("[dirs]\ndata = %s\nlog = %s\ncheckpoints = %s\n[run]\nbatch_size = 1\n%s[train]\nheight = 64\nwidth = 128\n"
                   "num_iters = 2\nsave_interval = 2\n" % (tmp_path / 'data', tmp_path / 'log', tmp_path / 'ckpt', extra))
    return str(cfg)


def test_warning_without_excludes_and_missing_data_message(tmp_path, capsys, monkeypatch):
    """The command up to the point where it needs frames: --dataset kitti without --kitti_excludes warns once, and the missing
    kitti_raw is reported by name (before any GPU work)."""
    from unflow_amd import run as R
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(RuntimeError) as err:
        R.main(['--ex', 'a', '--config', _config(tmp_path)])
    assert os.path.join(str(tmp_path / 'data'), 'kitti_raw') in str(err.value)
    assert capsys.readouterr().out.count(R.NO_EXCLUDES_WARNING) == 1
    with pytest.raises(RuntimeError):
        R.main(['--ex', 'b', '--config', _config(tmp_path), '--kitti_excludes', EXCLUDES])
    assert R.NO_EXCLUDES_WARNING not in capsys.readouterr().out
    with pytest.raises(RuntimeError) as err:                              # [run] dataset decides when the flag is absent
        R.main(['--ex', 'c', '--config', _config(tmp_path, 'dataset = chairs\n')])
    assert os.path.join('flying_chairs', 'image') in str(err.value)
    assert R.NO_EXCLUDES_WARNING not in capsys.readouterr().out
