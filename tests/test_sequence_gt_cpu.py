"""Ground truth along a clip without a GPU: the host side — the nmaps words of sequence_tables, output_buffers with and
without the keyword, the option's rules and the methods' guards, the checks of a scored push, TrackScore's ratios, SintelInput.clips
and the full-size composition on a synthetic tree, and the flags of python -m unflow_amd.evaluate_flo --sequence."""
import os

import numpy as np
import pytest
import torch

import flo_fixture as F


# ------------------------------------------------------------------------------------------------- tables and buffers
@pytest.mark.parametrize("k,B,carry", [(1, 1, 0), (1, 1, 1), (2, 4, 0), (4, 4, 4), (1, 4, 3), (3, 3, 2)])
def test_sequence_tables_nmaps_words(k, B, carry):
    from unflow_amd.core.inference import sequence_tables
    plain, valid, nxt = sequence_tables((37, 53), k, B, carry, u8=True, max_flow=3.0, track=(2, 99))
    assert plain.shape == (16 * B + 4,) and plain.dtype == np.int32
    assert np.array_equal(sequence_tables((37, 53), k, B, carry, u8=True, max_flow=3.0, track=(2, 99), nmaps=0)[0], plain)
    for nmaps in (1, 2):
        tab, v2, n2 = sequence_tables((37, 53), k, B, carry, u8=True, max_flow=3.0, track=(2, 99), nmaps=nmaps)
        assert tab.shape == plain.shape and tab.dtype == np.int32 and v2 == valid and n2 == nxt
        want = plain.copy()
        for i in valid:
            want[8 * B + 8 * i + 4] = nmaps                  # word 4 of every VALID pair row, and nothing else
        assert np.array_equal(tab, want)
        assert tab[16 * B + 2] == 2 and tab[16 * B + 3] == 99          # the two track words stay where they are


def test_output_buffers_rows_with_and_without_the_keyword():
    from unflow_amd.core.inference import output_buffers
    old = output_buffers(2, 96, 160, 50, 3)
    assert [r[0] for r in old] == ['flow', 'u16', 'sums', 'counts', 'flow_bw', 'u16_bw', 'occ', 'occ_counts', 'vis', 'track_disp',
                                   'track_alive', 'mid', 'mid_holes']
    assert output_buffers(2, 96, 160, 50, 3, ground_truth=False) == old
    new = output_buffers(2, 96, 160, 50, 3, ground_truth=True)
    assert new[:13] == old
    assert [(r[0], r[2], r[3], r[4]) for r in new[13:]] == [
        ('track_scores', (2, 16), torch.int32, 'track_gt'), ('track_err', (2,), torch.float64, 'track_gt'),
        ('gt_track_disp', (2, 50, 2), torch.float32, 'track_gt'), ('gt_track_alive', (2, 50), torch.uint8, 'track_gt')]
    assert len({r[1] for r in new}) == len(new)


# ------------------------------------------------------------------------------------------------- option and guards
def test_ground_truth_needs_sequence():
    from unflow_amd.core.inference import FlowEstimator
    for kw in (dict(), dict(bidirectional=True), dict(visual=True)):
        with pytest.raises(ValueError, match="ground_truth .*needs sequence=True"):
            FlowEstimator(dict(flownet='C'), 2, net_size=(64, 128), ground_truth=True, **kw)


def _bare(**flags):
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator.__new__(FlowEstimator)
    base = dict(sequence=False, seq_bidir=False, bidirectional=False, visual=False, track=False, ground_truth=False, interpolate=0)
    for k, v in dict(base, **flags).items():
        setattr(est, k, v)
    return est


@pytest.mark.parametrize("method", ['push_scored', 'evaluate_sequence'])
def test_scoring_methods_of_other_estimators_raise_and_name_the_option(method):
    frames = [np.zeros((64, 128, 3), np.uint8)] * 3
    args = (frames, [None, None, None]) if method == 'push_scored' else ([(frames, [])],)
    with pytest.raises(RuntimeError, match=r"%s: a sequence estimator without ground truth.*sequence=True, ground_truth=True" % method):
        getattr(_bare(sequence=True), method)(*args)
    with pytest.raises(RuntimeError, match=r"%s: .*sequence='bidirectional', ground_truth=True" % method):
        getattr(_bare(sequence=True, seq_bidir=True, bidirectional=True, track=True), method)(*args)
    with pytest.raises(RuntimeError, match=r"%s: a pair estimator; build it with FlowEstimator\(\.\.\., sequence=True\)" % method):
        getattr(_bare(), method)(*args)
    with pytest.raises(RuntimeError, match="evaluate: a sequence estimator"):
        _bare(sequence=True, ground_truth=True).evaluate(iter(()))


def test_a_scored_push_checks_its_ground_truth_before_staging():
    est = _bare(sequence=True, ground_truth=True)
    h, w = 6, 7
    est._clip, est._carry, est._clip_nmaps, est.dev = (h, w, True), 0, 0, torch.device('cuda:0')
    one = (np.zeros((h, w, 2), np.float32), np.ones((h, w, 1), np.float32))
    two = one + one
    got = est._clip_gts([None, one, one], 3, 'push_scored')
    assert got[0] is None and est._clip_nmaps == 1 and got[1][0][0].shape == (h, w, 2) and got[1][0][1].shape == (h, w)
    with pytest.raises(ValueError, match="frame 1 has no ground truth"):
        est._clip_gts([None, None, one], 3, 'push_scored')
    with pytest.raises(ValueError, match=r"frame 2 has 2 map\(s\), the clip's has 1"):
        est._clip_gts([None, one, two], 3, 'push_scored')
    with pytest.raises(ValueError, match="3 frames, 2 ground truths"):
        est._clip_gts([None, one], 3, 'push_scored')
    with pytest.raises(ValueError, match=r"frame 1 is a \[6, 7, 2\] flow and a \[6, 7\] mask"):
        est._clip_gts([None, (np.zeros((h, w + 1, 2), np.float32), one[1])], 2, 'push_scored')
    with pytest.raises(ValueError, match="frame 1 is .*got 3 arrays"):
        est._clip_gts([None, one + (one[0],)], 2, 'push_scored')
    est._carry = 2                                    # later in the clip every frame ends a pair
    with pytest.raises(ValueError, match="frame 0 has no ground truth"):
        est._clip_gts([None, one], 2, 'push_scored')
    est._clip_nmaps = 0
    assert est._clip_gts([two, two], 2, 'push_scored')[0][1][1].shape == (h, w) and est._clip_nmaps == 2


def test_track_score_ratios():
    from unflow_amd.core.inference import TRACK_SCORE_THRESHOLDS, track_score
    assert TRACK_SCORE_THRESHOLDS == (1.0, 2.0, 4.0, 8.0, 16.0)
    words = [10, 8, 6, 1, 2, 4, 8, 10, 1, 2, 3, 5, 6, 15, 20, 0]
    t = track_score(words, 12.0, None, None)
    assert (t.n_gt, t.n_pred, t.n_both) == (10, 8, 6) and t.epe == 2.0 and t.occ_acc == 0.75
    assert t.pos_acc == [0.1, 0.2, 0.4, 0.8, 1.0]
    assert t.jaccard == [1 / 17, 2 / 16, 3 / 15, 5 / 13, 6 / 12]
    z = track_score([0] * 16, 0.0, None, None)
    assert np.isnan(z.epe) and np.isnan(z.occ_acc) and all(np.isnan(v) for v in z.pos_acc + z.jaccard)


# ------------------------------------------------------------------------------------------------- the input
def _sintel(tmp_path, scenes=((2, (40, 64)), (3, (40, 64)), (5, (40, 64)))):
    from unflow_amd.sintel.input import SintelInput
    truth = F.make_sintel(tmp_path / "data", list(scenes), seed=41)
    return SintelInput(F.Data(tmp_path / "data"), 2, (40, 64), normalize=False), truth


def test_sintel_clips_lists_the_scenes(tmp_path):
    sin, truth = _sintel(tmp_path)
    for variant in ('clean', 'final'):
        clips = sin.clips(variant)
        assert [c[0] for c in clips] == ['scene_0', 'scene_1', 'scene_2']
        assert [len(c[1]) for c in clips] == [2, 3, 5] and [len(c[2]) for c in clips] == [1, 2, 4]
        pairs, gt = sin.train_files('sintel/training/' + variant)
        assert [p for c in clips for p in zip(c[1][:-1], c[1][1:])] == pairs          # the pairs of pair mode, in its order
        assert [t for c in clips for t in c[2]] == list(zip(*gt))
        for name, files, triples in clips:
            assert all(os.sep + variant + os.sep + name + os.sep in f for f in files)
            for i, (fl, inv, oc) in enumerate(triples):
                assert fl.endswith('frame_%04d.flo' % (i + 1)) and inv.endswith('frame_%04d.png' % (i + 1)) and 'invalid' in inv
                assert 'occlusions' in oc and oc.endswith('frame_%04d.png' % (i + 1))
    with pytest.raises(ValueError, match="variant"):
        sin.clips('albedo')
    # a scene that lost a flow file and another that gained one: the totals agree, the scenes do not
    tr = tmp_path / "data" / "sintel" / "training"
    os.rename(str(tr / "flow" / "scene_2" / "frame_0004.flo"), str(tr / "flow" / "scene_1" / "frame_0009.flo"))
    with pytest.raises(ValueError, match="scene scene_1 has 3 frames"):
        sin.clips('clean')


def test_full_size_composition_is_the_padded_one_without_the_padding(tmp_path):
    sin, truth = _sintel(tmp_path, scenes=((3, (37, 53)),))
    from unflow_amd.sintel.input import SintelInput
    exact = SintelInput(F.Data(tmp_path / "data"), 2, (37, 53), normalize=False)       # dims = the files' size: no crop, no pad
    for i, triple in enumerate(sin.clips('clean')[0][2]):
        full = sin.read_gt_full(*triple)
        want = exact._read_gt(*triple)
        assert full[0].shape == (37, 53, 2) and full[1].shape == (37, 53)
        assert F.same_bits(full[0], want[0]) and F.same_bits(full[2], want[2])
        assert F.same_bits(full[1], want[1][:, :, 0]) and F.same_bits(full[3], want[3][:, :, 0])
        flow, inv, occ = truth[(0, i)]
        assert np.array_equal(full[1], (inv == 0).astype(np.float32)) and np.array_equal(full[3], ((inv == 0) & (occ == 0)))


# ------------------------------------------------------------------------------------------------- the command line
def test_cli_sequence_flags(capsys):
    from unflow_amd import evaluate_flo as E
    base = ['--ex', 'x', '--dataset', 'sintel']
    d = E.parse_args(base)
    assert d.sequence is False and d.track is False and d.track_stride is None and d.track_option is False
    assert (d.variant, d.dims, d.num, d.batch_size, d.occlusion, d.output_benchmark, d.host_decode) == \
        ('train_clean', (512, 1024), 10, 4, False, False, False)                    # every other default is what it was
    a = E.parse_args(base + ['--sequence'])
    assert a.sequence and a.track_option is False
    assert E.parse_args(base + ['--sequence', '--track']).track_option is True
    assert E.parse_args(base + ['--sequence', '--track', '--track_stride', '4', '--occlusion']).track_option == 4
    assert E.parse_args(base + ['--sequence', '--variant', 'train_final', '--host_decode']).variant == 'train_final'
    capsys.readouterr()

    def refused(args, *words):
        with pytest.raises(SystemExit) as e:
            E.parse_args(args)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
    refused(['--ex', 'x', '--dataset', 'chairs', '--sequence'], '--sequence', 'pairs')
    refused(['--ex', 'x', '--dataset', 'mdb', '--sequence'], '--sequence', 'pairs')
    refused(base + ['--sequence', '--variant', 'test_clean'], 'ground truth')
    refused(base + ['--track'], 'need --sequence')
    refused(base + ['--track_stride', '2'], 'need --sequence')
    refused(base + ['--sequence', '--track_stride', '0'], 'at least 1')
    refused(base + ['--sequence', '--visual'], 'pictures')
    with pytest.raises(SystemExit) as e:
        E.parse_args(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--sequence' in out and '--track' in out and '--track_stride' in out
