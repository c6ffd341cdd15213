"""-m gpu: ground truth along a clip through FlowEstimator(..., sequence=..., ground_truth=True): the sums, counts
and occlusion counts of every pair against recomputations from the returned flow and masks (the checks tests/test_inference_gpu.py
applies to pair mode), the track scores against the numpy definition, pushes / reset / eager / the first replay ever against the
whole clip, a scoring estimator beside a plain one, evaluate_sequence on a synthetic Sintel tree against pushing by hand and
against pair mode, and the command line."""
import os

import numpy as np
import pytest
import torch

import flo_fixture as F
import test_sequence_gpu as SG          # clip(), _params(), _bound() and the shared parameter cache of the sequence tests
import track_ref as TR
import track_score_ref as R

pytestmark = pytest.mark.gpu

H, W, FH, FW, NFRAMES = 64, 128, 90, 151, 6
MAXF = (96, 160)                        # the estimator's buffers are wider than the frames: the pitch is not the width
CONFIGS = {                             # sequence, track, maps of the ground truth, the pushes of the short-push run (6 frames)
    'fw-S2-m2': (True, 2, 2, (1, 2, 1, 2)),
    'bi-points-m2': ('bidirectional', 'points', 2, (2, 1, 1, 2)),
    'bi-S2-m1': ('bidirectional', 2, 1, (1, 1, 2, 2)),
}
B = 2
HEAD_SCALE = 0.1                        # tests/test_track_gpu.py's: flows of a few tenths of a pixel, masks that leave tracks alive
_EST, _FIRST = {}, {}


def _points():
    return TR.sparse_points(np.random.RandomState(5), 65, FH, FW).astype(np.int32)


def _frames():
    return SG.clip(NFRAMES, FH, FW, 61)


def _gts(nmaps, n=NFRAMES - 1, h=FH, w=FW, seed=7):
    """Per pair a random ground truth of +-6 px, 30 % of the pixels invalid and (two maps) another 10 % occluded: (flow, mask) or
    (flow_occ, mask_occ, flow_noc, mask_noc), the masks [h, w, 1] for the first pair and [h, w] for the rest."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        flow = ((rs.rand(h, w, 2) - 0.5) * 12).astype(np.float32)
        m_occ = (rs.rand(h, w) < 0.7).astype(np.float32)
        m_noc = m_occ * (rs.rand(h, w) < 6.0 / 7.0).astype(np.float32)
        shape = (h, w, 1) if i == 0 else (h, w)
        g = (flow, m_occ.reshape(shape))
        if nmaps == 2:
            g += (flow * m_noc[..., None], m_noc.reshape(shape))
        out.append(g)
    return out


def _estimator(name, dev, use_graph=True, ground_truth=True):
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, ground_truth)
    if key not in _EST:
        seq, tr, _, _ = CONFIGS[name]
        est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=MAXF, device=dev, sequence=seq, use_graph=use_graph,
                            track=_points() if tr == 'points' else tr, ground_truth=ground_truth)
        tfp = SG._params(est, 'C')
        if seq == 'bidirectional':
            est.load_tf_params({k: (v * HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                                for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _pushed(est, frames, gts, pushes):
    """reset, then push_scored in the given portions; gts[i] belongs to the pair (i, i + 1)."""
    est.reset()
    per_frame, out, n0 = [None] + list(gts), [], 0
    for k in pushes:
        got = est.push_scored(frames[n0:n0 + k], per_frame[n0:n0 + k])
        assert len(got) == (k if n0 else k - 1)
        out += got
        n0 += k
    assert n0 == len(frames)
    return out


def _first(name, dev):
    """The whole clip, B frames per push, as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, True) not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None
        _FIRST[name] = _pushed(est, _frames(), _gts(CONFIGS[name][2]), (B,) * (NFRAMES // B))
        assert est.graph is not None
    return _FIRST[name]


def _diff(a, b):
    """The first difference of two PairScore lists, every field compared bit for bit; None when there is none."""
    if len(a) != len(b):
        return "%d pairs against %d" % (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(x.flow.view(np.int32), y.flow.view(np.int32)):
            return "pair %d: flow" % i
        for k in ('aee', 'outliers', 'mask_sum', 'occ_counts'):
            if getattr(x, k) != getattr(y, k):
                return "pair %d: %s %s against %s" % (i, k, getattr(x, k), getattr(y, k))
        if (x.track is None) != (y.track is None):
            return "pair %d: track" % i
        if x.track is not None:
            s, t = x.track, y.track
            if s[:3] != t[:3]:
                return "pair %d: track counts %s against %s" % (i, s[:3], t[:3])
            if not np.array_equal([s.epe, s.occ_acc] + s.pos_acc + s.jaccard, [t.epe, t.occ_acc] + t.pos_acc + t.jaccard, equal_nan=True):
                return "pair %d: track ratios %s against %s" % (i, s[3:7], t[3:7])
            if not np.array_equal(s.gt_alive, t.gt_alive):
                return "pair %d: gt_alive" % i
            if not np.array_equal(s.gt_disp.view(np.int32), t.gt_disp.view(np.int32)):
                bad = np.flatnonzero((s.gt_disp.view(np.int32) != t.gt_disp.view(np.int32)).reshape(-1, 2).any(1))
                return "pair %d: gt_disp of tracks %s (alive %s)" % (i, bad[:8], s.gt_alive.reshape(-1)[bad[:8]])
    return None


def _same(a, b):
    d = _diff(a, b)
    if d is not None:
        print("differs:", d)
    return d is None


# ------------------------------------------------------------------------------------------------- 1. the scores of a pair
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_sums_counts_and_occlusion_counts_follow_from_the_returned_flow(name, dev):
    from unflow_amd.core.inference import PairScore
    seq, tr, nmaps, _ = CONFIGS[name]
    scores = _first(name, dev)
    est = _estimator(name, dev)
    gts = _gts(nmaps)
    assert len(scores) == NFRAMES - 1 and all(isinstance(s, PairScore) for s in scores)
    occ = [b.occ_fw for b in est.estimate_sequence_bidirectional(_frames())] if seq == 'bidirectional' else None
    for i, s in enumerate(scores):
        assert s.flow.shape == (FH, FW, 2) and s.flow.dtype == np.float32 and len(s.aee) == len(s.outliers) == len(s.mask_sum) == nmaps
        f = s.flow.astype(np.float64)
        for k in range(nmaps):
            gk, mk = gts[i][2 * k].astype(np.float64), gts[i][2 * k + 1].reshape(FH, FW).astype(np.float64)
            d = np.sqrt(((gk - f) ** 2).sum(-1)) * mk
            thr = np.maximum(np.sqrt((gk ** 2).sum(-1)) * 0.05, 3.0)
            assert s.mask_sum[k] == mk.sum() > 0                                          # exact
            err_sum = s.aee[k] * s.mask_sum[k]
            assert abs(err_sum - d.sum()) <= 1e-6 * d.sum() * (1 + 1e-9), (i, k, err_sum, d.sum())
            near = int((np.abs(d - thr) < 1e-4).sum())
            assert near < 1e-3 * FH * FW, (i, k, near)                                    # the allowance stays under 0.1 % of the pixels
            n_ref, n_got = int((d >= thr).sum()), s.outliers[k] * s.mask_sum[k] / 100.0
            assert abs(n_got - round(n_got)) < 1e-6 and abs(round(n_got) - n_ref) <= near, (i, k, n_got, n_ref, near)
            assert n_ref > 0
        if seq == 'bidirectional' and nmaps == 2:
            m_occ, m_noc = gts[i][1].reshape(FH, FW), gts[i][3].reshape(FH, FW)
            ev, pos, o = m_occ == 1, m_noc == 0, occ[i]
            want = [int((ev & o & pos).sum()), int((ev & o & ~pos).sum()), int((ev & ~o & pos).sum())]
            assert s.occ_counts == want and sum(want) > 0, (i, s.occ_counts, want)
        else:
            assert s.occ_counts is None


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_track_scores_are_the_definition_on_the_estimators_own_tracks(name, dev):
    from unflow_amd.core.inference import TrackScore, track_grid
    seq, tr, nmaps, _ = CONFIGS[name]
    scores = _first(name, dev)
    est = _estimator(name, dev)
    gts = _gts(nmaps)
    tracks = est.track_sequence(_frames())                   # the same estimator, the same clip: the tracks that were scored
    if tr == 'points':
        anchors, shape = _points().astype(np.int64), (65,)
    else:
        anchors, shape = TR.grid_anchors(FH, FW, tr), track_grid((FH, FW), tr)
    N = len(anchors)
    disp, alive = np.zeros((N, 2), np.float32), np.ones(N, bool)
    seen = np.zeros(16, np.int64)
    for i, s in enumerate(scores):
        t = s.track
        assert isinstance(t, TrackScore) and t.gt_disp.shape == shape + (2,) and t.gt_alive.shape == shape and t.gt_alive.dtype == bool
        # the ground-truth track: the fp32 definition on map 0's flow and the last map's mask, seeded from the kernel's own last
        # step, the in-frame flag decided on the displacement both sides share (track_ref.check_replay's split)
        masks = np.stack([gts[i][2 * k + 1].reshape(FH, FW) for k in range(nmaps)])[:, None]
        got = t.gt_disp.reshape(-1, 2)
        new, alive = TR.step(disp, alive, anchors, gts[i][0], R.occ_of(masks, nmaps, 0), FH, FW, np.float32, frame_disp=got)
        assert np.array_equal(t.gt_alive.reshape(-1), alive), i
        assert np.abs(got[alive] - new[alive]).max(initial=0) <= 1e-5 * max(1.0, float(np.abs(new[alive]).max(initial=0))), i
        disp = got.copy()
        # the words and the error sum from the tracks as returned
        words, _ = R.score(tracks[i].disp.reshape(-1, 2), tracks[i].alive.reshape(-1), got, alive)
        exact = R.err_exact(tracks[i].disp.reshape(-1, 2), tracks[i].alive.reshape(-1), got, alive)
        assert (t.n_gt, t.n_pred, t.n_both) == tuple(int(v) for v in words[:3]), (i, t[:3], words[:3])
        nan = float('nan')
        assert np.array_equal(t.pos_acc, [words[3 + k] / words[0] if words[0] else nan for k in range(5)], equal_nan=True)
        assert np.array_equal(t.jaccard, [words[8 + k] / (words[0] + words[1] - words[8 + k]) if words[0] + words[1] - words[8 + k]
                                          else nan for k in range(5)], equal_nan=True)
        assert t.occ_acc == words[13] / N
        if words[2]:
            assert abs(t.epe * words[2] - exact) <= 2.0 ** -22 * exact * (1 + 1e-9), (i, t.epe * words[2], exact)
        else:
            assert np.isnan(t.epe)
        seen += words
    print("%s: summed words %s" % (name, seen[:14].tolist()))
    assert seen[0] > 0 and seen[1] > 0 and seen[13] > 0


# ------------------------------------------------------------------------------------------------- 2. reproducibility
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pushes_reset_and_eager_are_bit_identical_to_the_whole_clip(name, dev):
    ref = _first(name, dev)                        # from the estimator's first replay ever
    est = _estimator(name, dev)
    frames, gts = _frames(), _gts(CONFIGS[name][2])
    g = est.graph
    whole = (B,) * (NFRAMES // B)
    assert _same(_pushed(est, frames, gts, whole), ref)                   # the same clip again
    assert _same(_pushed(est, frames, gts, CONFIGS[name][3]), ref)        # uneven portions through the same state
    assert est.graph is g                                                 # one graph, never re-captured
    eager = _estimator(name, dev, use_graph=False)
    assert _same(_pushed(eager, frames, gts, whole), ref) and eager.graph is None
    # another clip in between leaves nothing behind
    other = _pushed(est, SG.clip(4, FH, FW, 62), _gts(CONFIGS[name][2], 3, seed=8), (2, 2))
    assert len(other) == 3 and not _same(other, ref[:3])
    assert _same(_pushed(est, frames, gts, whole), ref)
    # ground truth already on the device: the same scores
    on_dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in g_) for g_ in gts]
    assert _same(_pushed(est, frames, on_dev, whole), ref)


@pytest.mark.parametrize("name", ['fw-S2-m2', 'bi-points-m2'])
def test_a_scoring_estimator_returns_what_a_plain_one_returns(name, dev):
    ref = _first(name, dev)
    est, plain = _estimator(name, dev), _estimator(name, dev, ground_truth=False)
    frames = _frames()
    assert plain.gt_flow is None and plain.gt_mask is None and plain.out_track_scores is None and plain.track_score_ws is None
    assert est.gt_flow.shape == (2, B) + MAXF + (2,) and est.gt_mask.shape == (2, B) + MAXF
    a, b = est.estimate_sequence(frames), plain.estimate_sequence(frames)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b)) and len(a) == NFRAMES - 1
    assert all(np.array_equal(x.view(np.int32), s.flow.view(np.int32)) for x, s in zip(a, ref))
    ta, tb = est.track_sequence(frames), plain.track_sequence(frames)
    assert all(np.array_equal(x.disp.view(np.int32), y.disp.view(np.int32)) and np.array_equal(x.alive, y.alive) for x, y in zip(ta, tb))
    if CONFIGS[name][0] == 'bidirectional':
        a, b = est.estimate_sequence_bidirectional(frames), plain.estimate_sequence_bidirectional(frames)
        assert all(np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u, v.view(np.int32) if v.dtype == np.float32 else v)
                   for x, y in zip(a, b) for u, v in zip(x, y))
    for call in (lambda: plain.push_scored(frames[:2], [None, None]), lambda: plain.evaluate_sequence([(frames, [])])):
        with pytest.raises(RuntimeError, match="without ground truth.*ground_truth=True"):
            call()
    est.reset()
    with pytest.raises(ValueError, match="frame 1 has no ground truth"):
        est.push_scored(frames[:2], [None, None])
    est.reset()


# ------------------------------------------------------------------------------------------------- 3. clips from files
SCENES = [(2, (40, 64)), (3, (40, 64)), (5, (40, 64))]


@pytest.fixture(scope="module")
def sintel(tmp_path_factory, dev):
    """A synthetic Sintel tree, a checkpoint and a config.ini: (tree root, SintelInput, parameters, config path)."""
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import save_checkpoint
    from unflow_amd.sintel.input import SintelInput
    tmp = tmp_path_factory.mktemp("sintel_clips")
    F.make_sintel(tmp / "data", SCENES, seed=43)
    est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=(40, 64), device=dev, sequence='bidirectional', track=2,
                        ground_truth=True)
    tfp = est.engine.init_params(seed=6)
    tfp = {k: (v * HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v).cpu() for k, v in tfp.items()}
    est.load_tf_params(tfp)
    ck = tmp / "ckpt" / "run"
    ck.mkdir(parents=True)
    save_checkpoint(str(ck / "model.ckpt-7"), tfp, 7)
    (ck / "checkpoint").write_text('model_checkpoint_path: "model.ckpt-7"\n')
    cfg = tmp / "config.ini"
    cfg.write_text("[dirs]\ndata = %s\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp / "data", tmp / "log", tmp / "ckpt"))
    return tmp, SintelInput(F.Data(tmp / "data"), B, (H, W), normalize=False), est, tfp, str(cfg)


def test_evaluate_sequence_equals_pushing_every_clip_by_hand_and_agrees_with_pair_mode(sintel, dev):
    from unflow_amd import evaluate_flo as E
    from unflow_amd.core.inference import FlowEstimator, track_score
    from unflow_amd.core.png_device import sintel_gt_device
    from unflow_amd.sequence import read_frame
    tmp, sin, est, tfp, _ = sintel
    clips = sin.clips('clean')
    res = est.evaluate_sequence(E.clip_stream(sin, clips, B, None))
    assert res['names'] == ['AEE/occluded', 'outliers/occluded', 'AEE/non-occluded', 'outliers/non-occluded']
    assert res['num_examples'] == 7 and res['per_clip'] == [1, 2, 4] and len(res['per_example']) == 7 and len(res['occ_counts']) == 7
    assert len(res['per_example_track']) == 7 and all(k in res for k in E.TRACK_NAMES + ('occ/precision', 'occ/recall', 'occ/F1'))
    # by hand: every clip pushed through push_scored
    rows, occ, tracks = [], [], []
    for _, files, triples in clips:
        frames = [read_frame(p) for p in files]
        portions = [min(B, len(frames) - n) for n in range(0, len(frames), B)]
        for s in _pushed(est, frames, [sin.read_gt_full(*t) for t in triples], portions):
            rows.append([v for m in range(2) for v in (s.aee[m], s.outliers[m])])
            occ.append(s.occ_counts)
            tracks.append(s.track)
    assert res['per_example'] == rows and res['occ_counts'] == occ
    assert np.array_equal(np.mean(np.asarray(rows, np.float64), axis=0), [res[k] for k in res['names']])
    assert all(t.gt_disp is None and t.gt_alive is None for t in res['per_example_track'])
    flat = lambda ts: np.asarray([list(t[:4]) + t.pos_acc + t.jaccard + [t.occ_acc] for t in ts], np.float64)      # noqa: E731
    assert np.array_equal(flat(res['per_example_track']), flat(tracks), equal_nan=True)
    # the pooled track scores: from the summed integers, not averages of ratios
    n_gt, n_pred, n_both = (sum(t[k] for t in tracks) for k in range(3))
    within_gt = [sum(round(t.pos_acc[k] * t.n_gt) for t in tracks if t.n_gt) for k in range(5)]
    assert n_gt > 0 and abs(res['track/delta_avg'] - np.mean([v / n_gt for v in within_gt])) < 1e-12
    agree = sum(round(t.occ_acc * t.gt_alive.size) for t in tracks)
    assert abs(res['track/occ_acc'] - agree / sum(t.gt_alive.size for t in tracks)) < 1e-12
    if n_both:
        assert abs(res['track/epe'] - sum(t.epe * t.n_both for t in tracks if t.n_both) / n_both) < 1e-9
    # the ground truth composed on the device gives the same bits, so the same scores; num cuts behind that many pairs
    flow, mask = sintel_gt_device(clips[2][2], dev)
    for i, t in enumerate(clips[2][2]):
        host = sin.read_gt_full(*t)
        for a, b in zip(host, (flow[0, i], mask[0, i], flow[1, i], mask[1, i])):
            assert F.same_bits(np.ascontiguousarray(a), b.cpu().numpy())
    on_dev = est.evaluate_sequence(E.clip_stream(sin, clips, B, dev))
    assert on_dev['per_example'] == rows and on_dev['occ_counts'] == occ and on_dev['track/AJ'] == res['track/AJ']
    cut = est.evaluate_sequence(E.clip_stream(sin, clips, B, None, num=4))
    assert cut['per_example'] == rows[:4] and cut['per_clip'] == [1, 2, 1]
    # pair mode on the same tree: the AEE of every pair within the sequence tests' bound
    pair = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), device=dev, bidirectional=True)
    pair.load_tf_params(tfp)
    want = pair.evaluate(sin.input_train_clean(device=None))
    assert want['names'] == res['names'] and want['num_examples'] == 7
    for i, (a, b) in enumerate(zip(res['per_example'], want['per_example'])):
        print("pair %d: AEE sequence %.6f %.6f, pair mode %.6f %.6f" % (i, a[0], a[2], b[0], b[2]))
        assert abs(a[0] - b[0]) < SG._bound() and abs(a[2] - b[2]) < SG._bound(), (i, a, b)


def test_evaluate_flo_sequence_command_line(sintel, dev, capsys, tmp_path):
    from unflow_amd import evaluate_flo as E
    tmp, sin, est, _, cfg = sintel
    res = est.evaluate_sequence(E.clip_stream(sin, sin.clips('final'), B, None))
    capsys.readouterr()
    argv = ['--dataset', 'sintel', '--variant', 'train_final', '--ex', 'run', '--num', '-1', '--batch_size', str(B), '--dims', str(H),
            str(W), '--config', cfg, '--sequence', '--occlusion', '--track_stride', '2']
    assert E.main(argv + ['--out', str(tmp_path / "dev"), '--output_benchmark']) == 0
    out = capsys.readouterr().out
    lines = dict(line.split() for line in out.splitlines() if line and line[0] != '-' and len(line.split()) == 2)
    for k in res['names'] + ['occ/precision', 'occ/recall', 'occ/F1'] + list(E.TRACK_NAMES):
        assert lines[k] == "%.4f" % res[k], (k, lines[k], res[k])
    assert lines['examples:'] == '7'
    for scene, n in (('scene_0', 1), ('scene_1', 2), ('scene_2', 4)):
        names = sorted(os.listdir(str(tmp_path / "dev" / "run" / scene)))
        assert names == sorted(n_ % i for i in range(n) for n_ in ('%06d_10.flo', '%06d_10_occ.png', '%06d_track.flo')), names
    assert E.main(argv + ['--out', str(tmp_path / "host"), '--host_decode']) == 0
    assert capsys.readouterr().out == "\n".join(line for line in out.splitlines() if not line.startswith('wrote')) + "\n"
