"""CPU (-m "not gpu"): the Sintel / FlyingChairs / Middlebury inputs — flo_header, the three listings, the host iterators against
hand-built numpy (float arrays through their bit views), the planner's table and staging layout for .flo files, and
python -m unflow_amd.evaluate_flo's flags."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import flo_fixture as F
from unflow_amd import evaluate_flo as E
from unflow_amd.chairs.input import ChairsInput
from unflow_amd.core import input as I
from unflow_amd.core import png_device as D
from unflow_amd.middlebury.input import MiddleburyInput
from unflow_amd.sintel.input import SintelInput


# ------------------------------------------------------------------------------------------------------------- flo_header
def test_flo_header_accepts_a_good_file_and_names_a_bad_one(tmp_path):
    good = str(tmp_path / "good.flo")
    I.write_flo(good, np.zeros((5, 7, 2), np.float32))
    assert D.flo_header(good) == (5, 7)
    body = open(good, 'rb').read()
    assert len(body) == 12 + 8 * 5 * 7
    bad = {"tag.flo": struct.pack('<f', 202021.0) + body[4:], "truncated.flo": body[:-4], "trailing.flo": body + b'\0',
           "short.flo": body[:8], "negative.flo": body[:4] + struct.pack('<ii', -7, -5) + body[12:]}
    for name, data in bad.items():
        p = str(tmp_path / name)
        with open(p, 'wb') as f:
            f.write(data)
        with pytest.raises(ValueError, match=re.escape(p)):
            D.flo_header(p)


# ------------------------------------------------------------------------------------------------------------- listings
def test_sintel_listing_pairs_consecutive_frames_per_scene(tmp_path):
    F.make_sintel(tmp_path, [(3, (10, 12)), (4, (9, 14))], seed=1, test_scenes=[(3, (10, 12))])
    sin = SintelInput(F.Data(tmp_path), 2, (16, 16), normalize=False)
    pairs, (flow, invalid, occ) = sin.train_files('sintel/training/clean')
    rel = lambda p: os.path.relpath(p, str(tmp_path / 'sintel' / 'training'))        # noqa: E731
    assert [(rel(a), rel(b)) for a, b in pairs] == \
        [('clean/scene_0/frame_%04d.png' % i, 'clean/scene_0/frame_%04d.png' % (i + 1)) for i in (1, 2)] + \
        [('clean/scene_1/frame_%04d.png' % i, 'clean/scene_1/frame_%04d.png' % (i + 1)) for i in (1, 2, 3)]
    assert len(pairs) == len(flow) == len(invalid) == len(occ) == 5
    names = [(s, i) for s, n in ((0, 2), (1, 3)) for i in range(1, n + 1)]
    assert [rel(f) for f in flow] == ['flow/scene_%d/frame_%04d.flo' % k for k in names]
    assert [rel(f) for f in invalid] == ['invalid/scene_%d/frame_%04d.png' % k for k in names]      # each scene's last is dropped
    assert [rel(f) for f in occ] == ['occlusions/scene_%d/frame_%04d.png' % k for k in names]
    assert [os.path.basename(os.path.dirname(a)) for a, _ in sin.train_files('sintel/training/final')[0]] == ['scene_0'] * 2 + ['scene_1'] * 3
    # one occlusion map too many: the three lists disagree
    extra = str(tmp_path / 'sintel/training/occlusions/scene_1/frame_0004.png')
    with open(extra, 'wb') as f:
        f.write(I.encode_png8_gray(np.zeros((9, 14), np.uint8)))
    with pytest.raises(ValueError, match="5 flow files, 5 invalid maps .* 6 occlusion maps"):
        sin.gt_files()


def test_chairs_listing_pairs_2i_with_2i_plus_1(tmp_path):
    F.make_chairs(tmp_path, [(8, 10)] * 3, seed=2)
    ch = ChairsInput(F.Data(tmp_path), 2, (8, 10), normalize=False)
    pairs, (flows,) = ch.test_files()
    base = str(tmp_path / 'flying_chairs')
    assert pairs == [(os.path.join(base, 'test_image', '%05d_img1.png' % i), os.path.join(base, 'test_image', '%05d_img2.png' % i))
                     for i in (1, 2, 3)]
    assert flows == [os.path.join(base, 'flow', '%05d_flow.flo' % i) for i in (1, 2, 3)]
    os.remove(flows[2])
    with pytest.raises(ValueError, match="3 frame pairs .* 2 flow files"):
        ch.test_files()


def test_middlebury_listing_and_its_count_check(tmp_path):
    F.make_middlebury(tmp_path, [(2, (8, 10)), (3, (9, 11))], seed=3, eval_scenes=[(2, (8, 10))])
    mdb = MiddleburyInput(F.Data(tmp_path), 2, (16, 16), normalize=False)
    pairs, (flows,) = mdb.train_files()
    assert [tuple(os.path.basename(p) for p in pr) for pr in pairs] == [('frame10.png', 'frame11.png')] * 2 + [('frame11.png', 'frame12.png')]
    assert [os.path.basename(f) for f in flows] == ['flow10.flo', 'flow10.flo', 'flow11.flo']
    assert len(list(mdb.input_test())) == 1
    os.remove(flows[2])             # the reference would zip three pairs with two flow files without a word
    with pytest.raises(ValueError, match="3 frame pairs .* 2 flow files"):
        mdb.train_files()
    with pytest.raises(ValueError, match="3 frame pairs .* 2 flow files"):
        next(mdb.input_train())


# ------------------------------------------------------------------------------------------------------------- host iterators
def pad(a, H, W):
    """resize_image_with_crop_or_pad by hand for a map smaller than (H, W) in both axes."""
    h, w = a.shape[:2]
    out = np.zeros((H, W) + a.shape[2:], a.dtype)
    out[(H - h) // 2:(H - h) // 2 + h, (W - w) // 2:(W - w) // 2 + w] = a
    return out


def test_sintel_host_iterator_composes_the_two_maps(tmp_path):
    H, W = 16, 18
    truth = F.make_sintel(tmp_path, [(2, (11, 13))], seed=4, test_scenes=[(2, (11, 13))])
    flow, inv, occ = truth[(0, 0)]
    sin = SintelInput(F.Data(tmp_path), 2, (H, W), normalize=False)
    (batch,) = list(sin.input_train_clean())
    assert len(batch) == 7 and [b.shape for b in batch] == [(1, H, W, 3)] * 2 + [(1, 3)] + [(1, H, W, 2), (1, H, W, 1)] * 2
    assert tuple(batch[2][0]) == (11, 13, 3) and batch[2].dtype == np.int32
    frame = I.read_png_image(str(tmp_path / 'sintel/training/clean/scene_0/frame_0001.png'))
    assert F.same_bits(batch[0][0], pad(frame, H, W))
    f = pad(flow, H, W)
    visible = pad(1 - (occ != 0).astype(np.float32), H, W)[:, :, None]
    valid = pad(1 - (inv != 0).astype(np.float32), H, W)[:, :, None]
    # the padding happens BEFORE the composition: a padded pixel has inv = occ = 0, so both masks are 1 there and the flow 0
    inside = pad(np.ones((11, 13), bool), H, W)
    visible[~inside], valid[~inside] = 1, 1
    assert F.same_bits(batch[3][0], f) and F.same_bits(batch[4][0], valid)
    assert F.same_bits(batch[5][0], f * visible) and F.same_bits(batch[6][0], valid * visible)
    assert (batch[4][0][~inside] == 1).all() and (batch[6][0][~inside] == 1).all() and (F.bits(batch[3][0][~inside]) == 0).all()
    assert set(np.unique(batch[4])) == {0.0, 1.0} == set(np.unique(batch[6]))           # 0 / 1, not the reference's -254
    hidden = (occ != 0)
    assert hidden.any() and np.signbit(batch[5][0][2:13, 2:15][hidden]).all()             # -0 under a negative occluded component
    assert (batch[5][0][2:13, 2:15][hidden] == 0).all()
    (test,) = list(sin.input_test_final())
    assert len(test) == 3 and test[0].shape == (1, H, W, 3)
    # a mask of another size than its flow file is refused by name
    bad = str(tmp_path / 'sintel/training/occlusions/scene_0/frame_0001.png')
    with open(bad, 'wb') as fh:
        fh.write(I.encode_png8_gray(np.zeros((11, 12), np.uint8)))
    with pytest.raises(ValueError, match=re.escape(bad)):
        list(sin.input_train_clean())
    plan = D.EvalPlanner(*sin.train_files('sintel/training/clean')[:1], 2, (H, W), sin.gt_files(), gt_kind='sintel')
    with pytest.raises(ValueError, match=re.escape(bad)):
        plan.next_batch()


@pytest.mark.parametrize("dataset", ["chairs", "mdb"])
def test_one_map_host_iterators(tmp_path, dataset):
    H, W = 16, 18
    if dataset == "chairs":
        flow = F.make_chairs(tmp_path, [(11, 13)], seed=5, unknown=0.2)[0]
        it = ChairsInput(F.Data(tmp_path), 2, (H, W), normalize=True).input_test()
        first = str(tmp_path / 'flying_chairs/test_image/00001_img1.png')
    else:
        flow = F.make_middlebury(tmp_path, [(2, (11, 13))], seed=6, unknown=0.2)[0]
        it = MiddleburyInput(F.Data(tmp_path), 2, (H, W), normalize=True).input_train()
        first = str(tmp_path / 'middlebury/other-data/scene_0/frame10.png')
    (batch,) = list(it)
    assert len(batch) == 5 and [b.shape for b in batch] == [(1, H, W, 3)] * 2 + [(1, 3), (1, H, W, 2), (1, H, W, 1)]
    mean, stddev = np.asarray(I.Input.mean, np.float32), np.float32(I.Input.stddev)
    assert F.same_bits(batch[0][0], (pad(I.read_png_image(first), H, W) - mean) / stddev)        # padded, then normalised
    assert F.same_bits(batch[3][0], pad(flow, H, W))                                         # markers, NaN payloads and -0 kept
    with np.errstate(invalid='ignore'):
        known = ((flow[..., 0] < np.float32(1e9)) & (flow[..., 1] < np.float32(1e9))).astype(np.float32)
    assert 0 < known.sum() < known.size
    assert F.same_bits(batch[4][0], pad(known, H, W)[:, :, None])                            # the padding is unknown: mask 0


def test_chairs_input_raw_forwards_to_the_uncorrelated_pairs(tmp_path, capsys):
    F.make_chairs(tmp_path, [(8, 10)], seed=7, raw=(3, (8, 10)))
    ch = ChairsInput(F.Data(tmp_path, raw_dirs=['flying_chairs/image']), 2, (8, 10), normalize=False)
    shifted = ch.input_raw(swap_images=False, shift=1)
    assert shifted.pairs == ch.raw_pairs(swap_images=False, sequence=False, shift=1) != ch.raw_pairs(swap_images=False, sequence=False)
    it = ch.input_raw(swap_images=False)
    assert type(it) is I.RawPairBatches and not it.needs_crop and len(it.pairs) == 3
    assert sorted(it.pairs) == [tuple(str(tmp_path / 'flying_chairs/image' / ('%05d_img%d.png' % (i, k))) for k in (1, 2)) for i in (1, 2, 3)]
    im1, im2 = next(it)
    assert im1.shape == (2, 8, 10, 3) and F.same_bits(im1[0], I.read_png_image(it.pairs[0][0]))


# ------------------------------------------------------------------------------------------------------------- planner
def test_planner_lays_flo_files_out_aligned_and_column_major(tmp_path):
    """Three Sintel examples of 11 x 13 (8 * 11 * 13 = 1144 bytes per .flo body, not a multiple of 16; 11 x 14
    frames and 11 x 13 masks: PNG streams of 473 and 154 bytes), batches of two: a full batch and a short one."""
    rs = np.random.RandomState(8)
    tr = tmp_path / 'sintel' / 'training'
    for i in range(4):
        F.write_frame(str(tr / 'clean' / 's' / ('f%d.png' % i)), rs, 11, 14)
        F._put(str(tr / 'invalid' / 's' / ('f%d.png' % i)), I.encode_png8_gray(F.mask_map(rs, 11, 13)))
    for i in range(3):
        F.write_flo(str(tr / 'flow' / 's' / ('f%d.flo' % i)), F.flow_field(rs, 11, 13))
        F._put(str(tr / 'occlusions' / 's' / ('f%d.png' % i)), I.encode_png8_gray(F.mask_map(rs, 11, 13)))
    sin = SintelInput(F.Data(tmp_path), 2, (16, 16), normalize=False)
    pairs, gt = sin.train_files('sintel/training/clean')
    plan = D.EvalPlanner(pairs, 2, (16, 16), gt, gt_kind='sintel')
    assert plan.n_maps == 2
    sizes = []
    for k0 in (0, 2):
        examples = plan.next_batch()
        n = len(examples)
        sizes.append(n)
        assert [[f[2] for f in ex] for ex in examples] == [[D.FRAME, D.FRAME, D.FLO, D.MASK, D.MASK]] * n
        files = plan.table_files(examples)
        # column-major in the table's order: unflow_sintel_gt's 3 n rows (.flo, invalid, occlusions), then both frame columns
        cols = [gt[0], gt[1], gt[2], [p[0] for p in pairs], [p[1] for p in pairs]]
        assert [f[0] for f in files] == [c[k] for c in cols for k in range(k0, k0 + n)]
        job = D._Job(None, files, examples)
        assert (job.n_flo, job.n_mask, job.n_frames, job.n_gt) == (n, 2 * n, 2 * n, 0)
        rows, spans = np.asarray(job.rows), job.spans
        for r, (off, size) in zip(rows[:n], spans[:n]):                    # the .flo rows
            assert tuple(r) == (off, 0, 11, 13, 8, 4, -2, -1) and off % 16 == 0 and size == 1144
        assert [s[0] for s in spans[:n]] == [0, 1152][:n]                   # 1144 rounded up to the next multiple of 16
        end = spans[n - 1][0] + 1144
        for r, (off, size) in zip(rows[n:], spans[n:]):                    # the PNG rows: back to back behind the last .flo body
            assert off == end and r[0] == off and size == r[2] * (r[3] * r[4] + 1)
            end += size
        assert [s[1] for s in spans[n:]] == [154] * (2 * n) + [473] * (2 * n)
        assert job.n_raw == end
        assert [tuple(r[2:]) for r in rows[n:3 * n]] == [(11, 13, 1, 1, -2, -1)] * (2 * n)
        assert [tuple(r[2:]) for r in rows[3 * n:]] == [(11, 14, 3, 1, -2, -1)] * (2 * n)
        dst = [r[1] for r in rows[n:]]                                      # decoded bytes: the PNG rows only, tightly packed
        assert dst == list(np.cumsum([0] + [r[2] * r[3] * r[4] for r in rows[n:]])[:-1]) and job.n_dec == 2 * n * 143 + 2 * n * 462
    assert sizes == [2, 1] and plan.next_batch() is None
    # one list, one map; and the kinds refuse a wrong number of lists
    flo = D.EvalPlanner(pairs, 2, (16, 16), gt[:1], gt_kind='flo')
    ex = flo.next_batch()
    assert flo.n_maps == 1 and [f[2] for f in flo.table_files(ex)] == [D.FLO] * 2 + [D.FRAME] * 4
    for lists, kind in ((gt, 'flo'), (gt[:2], 'sintel'), (gt[:1], 'png')):
        with pytest.raises(ValueError):
            D.EvalPlanner(pairs, 2, (16, 16), lists, gt_kind=kind)
    kitti = D.EvalPlanner(pairs, 2, (16, 16))
    ex = kitti.next_batch()
    assert kitti.table_files(ex) == kitti.files(ex) and kitti.n_maps == 0  # no lists: a test split, frames only
    assert D.EvalPlanner(pairs, 2, (16, 16), gt[1:]).gt_roles == (D.GT, D.GT)          # lists without a kind: KITTI maps, as ever


# ------------------------------------------------------------------------------------------------------------- command line
def test_evaluate_flo_flags():
    a = E.parse_args(['--ex', 'x', '--dataset', 'sintel'])
    assert (a.variant, a.dims, a.num, a.has_gt, a.batch_size) == ('train_clean', (512, 1024), 10, True, 4)
    a = E.parse_args(['--ex', 'x', '--dataset', 'chairs', '--num', '-1'])
    assert (a.variant, a.dims, a.num, a.has_gt) == ('test', (384, 512), None, True)
    a = E.parse_args(['--ex', 'x', '--dataset', 'mdb', '--variant', 'test', '--dims', '64', '128'])
    assert (a.variant, a.dims, a.has_gt) == ('test', (64, 128), False)
    assert E.parse_args(['--ex', 'x', '--dataset', 'mdb']).dims == (512, 640)
    assert not E.parse_args(['--ex', 'x', '--dataset', 'sintel', '--variant', 'test_final']).has_gt
    for argv in (['--dataset', 'kitti'], ['--dataset', 'sintel', '--variant', 'train_2012'], ['--dataset', 'chairs', '--variant', 'train'],
                 ['--dataset', 'mdb', '--variant', 'test_clean'], ['--dataset', 'mdb', '--output_backward'],
                 ['--dataset', 'mdb', '--sheet'], ['--dataset', 'mdb', '--batch_size', '0'], []):
        with pytest.raises(SystemExit) as err:
            E.parse_args(['--ex', 'x'] + argv)
        assert err.value.code == 2, argv


def test_contact_sheets_are_put_together_from_the_exported_pictures(tmp_path):
    from unflow_amd.core.inference import VISUAL_IMAGES, visual_files
    from unflow_amd.visualize import SHEET_COLUMNS, contact_sheet
    rs = np.random.RandomState(9)
    pics = []
    for n, (h, w) in enumerate([(6, 8), (5, 9), (6, 8), (7, 7), (6, 8)]):
        pics.append({name: rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for name in VISUAL_IMAGES})
        for k, name in visual_files(n, True):
            I.write_png_rgb8(str(tmp_path / name), pics[n][VISUAL_IMAGES[k]])
    paths = E.write_sheets(str(tmp_path), 5, True, num_vis=100)
    assert [os.path.basename(p) for p in paths] == ['page_000.png', 'page_001.png']
    rows = [[ex[c] for c in SHEET_COLUMNS[True]] for ex in pics]
    for p, want in zip(paths, (contact_sheet(rows[:4]), contact_sheet(rows[4:]))):
        assert np.array_equal(I.decode_png(open(p, 'rb').read()), want)
    assert len(E.write_sheets(str(tmp_path), 5, True, num_vis=3)) == 1 and E.write_sheets(str(tmp_path), 5, True, num_vis=0) == []
    one = E.write_sheets(str(tmp_path), 1, False, num_vis=100)                # without ground truth: three columns
    assert np.array_equal(I.decode_png(open(one[0], 'rb').read()), contact_sheet([[pics[0][c] for c in SHEET_COLUMNS[False]]]))


def test_kitti_tools_point_at_the_new_module(capsys):
    from unflow_amd import evaluate, visualize
    for mod in (evaluate, visualize):
        with pytest.raises(SystemExit) as err:
            mod.parse_args(['--ex', 'x', '--dataset', 'sintel'])
        assert err.value.code == 2
        msg = capsys.readouterr().err
        assert 'not supported' in msg and 'unflow_amd.evaluate_flo' in msg


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_flo_entries_answer_on_the_host():
    from unflow_amd import build, _lib
    build.build()
    lib = _lib.lib()
    n, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(66)      # never dereferenced
    L = ctypes.c_long
    assert lib.unflow_flo_to_flow_gt(n, L(16), one, 1, 4, 4, one, one, n) == -1
    assert lib.unflow_flo_to_flow_gt(one, L(16), one, 1, 4, 4, one, n, n) == -1
    assert lib.unflow_flo_to_flow_gt(one, L(16), one, 0, 4, 4, one, one, n) == -5
    assert lib.unflow_flo_to_flow_gt(one, L(16), one, 65536, 4, 4, one, one, n) == -5
    assert lib.unflow_flo_to_flow_gt(one, L(0), one, 1, 4, 4, one, one, n) == -5
    assert lib.unflow_flo_to_flow_gt(one, L(16), one, 1, 0, 4, one, one, n) == -5
    assert lib.unflow_flo_to_flow_gt(one, L(16), one, 1, 1 << 15, 1 << 15, one, one, n) == -5
    assert lib.unflow_flo_to_flow_gt(odd, L(16), one, 1, 4, 4, one, one, n) == -5          # `raw` itself must be 4-byte aligned
    assert lib.unflow_sintel_gt(one, L(16), n, L(16), one, 1, 4, 4, one, one, n) == -1
    assert lib.unflow_sintel_gt(one, L(16), one, L(16), n, 1, 4, 4, one, one, n) == -1
    assert lib.unflow_sintel_gt(one, L(16), one, L(0), one, 1, 4, 4, one, one, n) == -5
    assert lib.unflow_sintel_gt(one, L(16), one, L(16), one, 1, 4, 0, one, one, n) == -5
    assert lib.unflow_sintel_gt(odd, L(16), one, L(16), one, 1, 4, 4, one, one, n) == -5
