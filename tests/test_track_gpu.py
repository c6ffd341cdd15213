"""-m gpu: tracks along a clip — unflow_sequence_track at its entry point against the numpy definition of
tests/track_ref.py, step by step, on synthetic flows and masks; against chaining with the project's image_warp; what it leaves
alone; its state across launches; and FlowEstimator(..., sequence=..., track=...) against the same definition chained over the
estimator's own flows and masks, across pushes / reset / graph and eager, beside a plain estimator, and through export_sequence
and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_sequence_gpu as SG          # clip(), _params() and the shared parameter cache of the sequence tests
import track_ref as T

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
CASES = T.entry_cases()
BY_ID = dict(CASES)
SENTINEL, SENTINEL_U8 = -777.0, 9
ERR_SHAPE = -5


def _L():
    from unflow_amd import _lib
    return _lib


class Launch:
    """The device buffers of one case, rows beyond the tracks and slots beyond the pairs filled with a sentinel, and the call."""

    def __init__(self, case, state, dev, Ncap=None, tab=None):
        self.case, self.dev = case, dev
        N, B = case['N'], case['B']
        self.Ncap = Ncap = case['Ncap'] if Ncap is None else Ncap
        self.n = n = min(N, Ncap)
        self.flow = torch.from_numpy(case['flow']).to(dev)
        self.occ = None if case['occ'] is None else torch.from_numpy(case['occ']).to(dev)
        self.tab = torch.from_numpy(case['tab'] if tab is None else tab).to(dev)
        self.anchors = torch.from_numpy(case['anchors'].astype(np.int32)).to(dev) if case['sparse'] else None
        self.disp = torch.full((Ncap, 2), SENTINEL, device=dev)
        self.alive = torch.full((Ncap,), SENTINEL_U8, dtype=torch.uint8, device=dev)
        if state is not None:
            self.disp[:n] = torch.from_numpy(state[0][:n]).to(dev)
            self.alive[:n] = torch.from_numpy(state[1][:n].astype(np.uint8)).to(dev)
        self.out_disp = torch.full((B, Ncap, 2), SENTINEL, device=dev)
        self.out_alive = torch.full((B, Ncap), SENTINEL_U8, dtype=torch.uint8, device=dev)

    def run(self, **kw):
        L, c = _L(), self.case
        a = dict(B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], Ncap=self.Ncap)
        a.update(kw)
        st = L.lib().unflow_sequence_track(L.ptr(self.flow), L.ptr(self.occ), L.ptr(self.tab), a['B'], a['Hmax'], a['Wmax'],
                                           L.ptr(self.anchors), a['Ncap'], L.ptr(self.disp), L.ptr(self.alive),
                                           L.ptr(self.out_disp), L.ptr(self.out_alive), L.stream())
        torch.cuda.synchronize()
        return st

    def results(self):
        """({valid slot: (disp fp32 [n, 2], alive bool [n])}, the state (disp, alive)); everything else still holds the sentinel."""
        n, c = self.n, self.case
        od, oa = self.out_disp.cpu().numpy(), self.out_alive.cpu().numpy()
        sd, sa = self.disp.cpu().numpy(), self.alive.cpu().numpy()
        assert set(np.unique(oa[list(c['valid']), :n])) <= {0, 1} and set(np.unique(sa[:n])) <= {0, 1}
        for i in range(c['B']):
            if i not in c['valid']:
                assert (od[i] == SENTINEL).all() and (oa[i] == SENTINEL_U8).all(), "slot %d is no pair and was written" % i
        assert (od[:, n:] == SENTINEL).all() and (oa[:, n:] == SENTINEL_U8).all(), "rows beyond the tracks were written"
        assert (sd[n:] == SENTINEL).all() and (sa[n:] == SENTINEL_U8).all(), "state beyond the tracks was written"
        return {i: (od[i, :n].copy(), oa[i, :n].astype(bool)) for i in c['valid']}, (sd[:n].copy(), sa[:n].astype(bool))

    def untouched(self):
        ok = bool((self.out_disp == SENTINEL).all()) and bool((self.out_alive == SENTINEL_U8).all())
        return ok


# ------------------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_track_kernel_against_the_mirror_step_by_step(cid, dev):
    """Every case of track_ref.entry_cases: the pitch that is not the width, ragged grids, sparse tables (one anchor outside), a
    launch past the grid's cap, every flow kind with a blob mask and with occ_fw = NULL, a clip's first replay (slot 0 no pair), a
    short first replay (no pair at all), trailing slots that are no pairs.  check_replay: alive bit for bit, disp within
    bound_of(yardstick, mirror) of the mirror seeded from the kernel's own previous slot; the sentinels in Launch.results."""
    case = BY_ID[cid]
    state = T.draw_state(case)
    run = Launch(case, state if case['carry'] else None, dev)       # carry source 0: the state holds the sentinel, never read
    assert run.run() == 0
    outs, new_state = run.results()
    worst = T.check_replay(case, state, outs, new_state)
    alive = [float(a.mean()) for _, a in outs.values()]
    print("%s: N = %d, valid slots %s, alive per slot %s, worst error / bound %.3f"
          % (cid, case['N'], case['valid'], ["%.2f" % a for a in alive], worst))
    if case['pattern'] == 'nopairs':                                 # the state was still initialised
        assert (new_state[0] == 0).all() and new_state[1].all()


@pytest.mark.parametrize("kind", ['smooth', 'tiny', 'far', 'const'])
def test_dense_stride_one_is_the_image_warp_chain_bit_for_bit(kind, dev):
    """disp_i = disp_(i-1) + image_warp(flow_i, disp_(i-1)), the project's existing op, on the tracks alive after slot i."""
    from unflow_amd.core.image_warp import image_warp
    shape = dict(T.RAGGED, Hmax=T.RAGGED['h'], Wmax=T.RAGGED['w'])          # image_warp takes dense images
    case = T.make_case('chain', anchors=1, kind=kind, occ=False, pattern='first', **shape)
    run = Launch(case, None, dev)
    assert run.run() == 0
    outs, _ = run.results()
    h, w = case['h'], case['w']
    prev = torch.zeros(1, h, w, 2, device=dev)
    seen = 0
    for i in case['valid']:
        want = (prev + image_warp(run.flow[i:i + 1].contiguous(), prev)).cpu().numpy().reshape(-1, 2)
        got, alive = outs[i]
        assert np.array_equal(got[alive].view(np.int32), want[alive].view(np.int32)), (kind, i)
        seen += int(alive.sum())
        prev = torch.from_numpy(got).to(dev).reshape(1, h, w, 2)
        prev = torch.where(torch.isfinite(prev) & (prev.abs() < 1e6), prev, torch.zeros_like(prev))    # (dead tracks: anything)
    assert seen > 100


def test_two_launches_equal_one_over_the_concatenated_pairs(dev):
    """A later replay of four pairs against two later replays of two pairs each over the same flows and masks, from the same
    state: the outputs and the final state bit for bit."""
    from unflow_amd.core.inference import sequence_tables
    one = BY_ID['ragged-S1-smooth-occ-first']
    one = dict(one, carry=4, valid=[0, 1, 2, 3], tab=sequence_tables((one['h'], one['w']), 4, 4, 4, track=(1, one['N']))[0])
    state = T.draw_state(one)
    whole = Launch(one, state, dev)
    assert whole.run() == 0
    outs, final = whole.results()
    T.check_replay(one, state, outs, final)
    got, cur = {}, state
    for half in (0, 1):
        sl = slice(2 * half, 2 * half + 2)
        part = dict(one, B=2, carry=2, valid=[0, 1], flow=one['flow'][sl], occ=one['occ'][sl],
                    tab=sequence_tables((one['h'], one['w']), 2, 2, 2, track=(1, one['N']))[0])
        run = Launch(part, cur, dev)
        assert run.run() == 0
        o, cur = run.results()
        got.update({2 * half + i: v for i, v in o.items()})
    for i in range(4):
        assert np.array_equal(got[i][0].view(np.int32), outs[i][0].view(np.int32)) and np.array_equal(got[i][1], outs[i][1]), i
    assert np.array_equal(cur[0].view(np.int32), final[0].view(np.int32)) and np.array_equal(cur[1], final[1])
    assert 0 < final[1].mean() < 1


@pytest.mark.parametrize("cid", ['ragged-S1-smooth-occ-first', 'sparse-65-far-noocc-first', 'small-smooth-occ-nopairs'])
def test_a_first_replay_run_twice_is_a_first_replay_run_once(cid, dev):
    """Carry source 0: the kernel re-initialises, so the eager pass and the captured graph's first replay of an estimator's first
    replay ever — the same launch twice — give what one launch gives, whatever the state held before."""
    case = BY_ID[cid]
    garbage = (np.full((case['N'], 2), np.nan, np.float32), np.zeros(case['N'], bool))
    once = Launch(case, garbage, dev)
    assert once.run() == 0
    twice = Launch(case, T.draw_state(case), dev)
    assert twice.run() == 0 and twice.run() == 0
    a, b = once.results(), twice.results()
    T.check_replay(case, None, *a)
    for i in case['valid']:
        assert np.array_equal(a[0][i][0].view(np.int32), b[0][i][0].view(np.int32)) and np.array_equal(a[0][i][1], b[0][i][1])
    assert np.array_equal(a[1][0].view(np.int32), b[1][0].view(np.int32)) and np.array_equal(a[1][1], b[1][1])


def test_more_tracks_than_capacity_are_clamped(dev):
    """N is read on the device: above Ncap the kernel tracks the first Ncap and writes no row beyond them."""
    case = BY_ID['sparse-65-smooth-occ-full']
    state = T.draw_state(case)
    run = Launch(case, state, dev, Ncap=40)
    assert run.run() == 0
    outs, new_state = run.results()
    cut = dict(case, N=40, anchors=case['anchors'][:40])
    T.check_replay(cut, (state[0][:40], state[1][:40]), outs, new_state)


def test_bad_arguments_return_the_shape_error_and_write_nothing(dev):
    case = BY_ID['ragged-S2-smooth-occ-full']
    state = T.draw_state(case)
    run = Launch(case, state, dev)
    before = (run.disp.clone(), run.alive.clone())
    for kw in (dict(B=0), dict(B=-1), dict(Ncap=0), dict(Ncap=-5), dict(Hmax=0), dict(Wmax=-1), dict(Hmax=65536, Wmax=32768)):
        assert run.run(**kw) == ERR_SHAPE, kw
    assert run.untouched() and torch.equal(run.disp, before[0]) and torch.equal(run.alive, before[1])
    # a dense grid of stride 0 or less is read on the device: the launch succeeds and tracks nothing
    for S in (0, -3):
        tab = case['tab'].copy()
        tab[16 * case['B'] + 2] = S
        bad = Launch(case, state, dev, tab=tab)
        assert bad.run() == 0
        assert bad.untouched() and torch.equal(bad.disp, before[0]) and torch.equal(bad.alive, before[1])
    # and a pair slot whose frame exceeds the buffers is no pair
    tab = case['tab'].copy()
    tab[8 * case['B'] + 1] = case['Wmax'] + 1
    odd = Launch(dict(case, valid=[1, 2, 3]), state, dev, tab=tab)
    assert odd.run() == 0
    odd.results()
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 2. the estimator
H, W, FH, FW, NFRAMES = 64, 128, 90, 151, 8
MAXF = (96, 160)                        # the estimator's buffers are wider than the frames: the pitch is not the width
CONFIGS = {                             # sequence, batch, track, the pushes of the short-push run (8 frames)
    'fw-B2-dense': (True, 2, True, (2, 1, 2, 2, 1)),
    'bi-B3-S3': ('bidirectional', 3, 3, (2, 3, 1, 2)),
    'bi-B2-points': ('bidirectional', 2, 'points', (2, 2, 1, 2, 1)),
    'fw-B3-S2': (True, 3, 2, (2, 3, 1, 2)),
}
HEAD_SCALE = 0.1
_EST, _FIRST = {}, {}


def _points():
    return T.sparse_points(np.random.RandomState(5), 65, FH, FW).astype(np.int32)


def _frames():
    return SG.clip(NFRAMES, FH, FW, 61)


def _estimator(name, dev, use_graph=True, track=None):
    """The estimator of a configuration, built once; track=False: the same estimator without tracks."""
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, track)
    if key not in _EST:
        seq, B, tr, _ = CONFIGS[name]
        tr = (_points() if tr == 'points' else tr) if track is None else track
        est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=MAXF, device=dev, sequence=seq, use_graph=use_graph,
                            track=tr)
        tfp = SG._params(est, 'C')
        if seq == 'bidirectional':
            # untrained forward and backward flows of pixels disagree, and at the shared parameters' scale the forward mask
            # covers 99 % of every pair: no track outlives the first.  Flow heads at a tenth (flows of a few tenths of a pixel)
            # leave the mask on 60 % of the first pair and 20 % of the last, so both outcomes of alive occur along the clip
            est.load_tf_params({k: (v * HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                                for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _first(name, dev):
    """track_sequence of the whole clip as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, None) not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None
        _FIRST[name] = est.track_sequence(_frames())
        assert est.graph is not None
    return _FIRST[name]


def _same_tracks(a, b):
    return len(a) == len(b) and all(np.array_equal(x.disp.view(np.int32), y.disp.view(np.int32)) and np.array_equal(x.alive, y.alive)
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_track_sequence_is_the_yardstick_chained_over_the_estimators_own_flows(name, dev):
    from unflow_amd.core.inference import Track, track_grid
    seq, B, tr, _ = CONFIGS[name]
    tracks = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames()
    if seq == 'bidirectional':
        both = est.estimate_sequence_bidirectional(frames)
        flows, occ = [b.flow_fw for b in both], np.stack([b.occ_fw for b in both]).astype(np.uint8)
    else:
        flows, occ = est.estimate_sequence(frames), None
    n = NFRAMES - 1
    assert len(tracks) == n and all(isinstance(t, Track) for t in tracks)
    if tr == 'points':
        anchors, shape = _points().astype(np.int64), (65,)
    else:
        S = 1 if tr is True else tr
        anchors, shape = T.grid_anchors(FH, FW, S), track_grid((FH, FW), S)
    for t in tracks:
        assert t.disp.shape == shape + (2,) and t.disp.dtype == np.float32 and t.alive.shape == shape and t.alive.dtype == bool
    case = dict(B=n, Hmax=FH, Wmax=FW, h=FH, w=FW, N=len(anchors), anchors=anchors, carry=0, valid=list(range(n)),
                flow=np.stack(flows), occ=occ)
    outs = {i: (t.disp.reshape(-1, 2), t.alive.reshape(-1)) for i, t in enumerate(tracks)}
    worst = T.check_replay(case, None, outs, outs[n - 1])
    alive = [float(t.alive.mean()) for t in tracks]
    print("%s: %d tracks, alive per pair %s, max |disp| %.2f, worst error / bound %.3f"
          % (name, len(anchors), ["%.3f" % a for a in alive], max(float(np.abs(t.disp).max()) for t in tracks), worst))
    assert tracks[0].alive.any() and not tracks[-1].alive.all()          # both outcomes occur on the clip
    assert max(float(np.abs(t.disp).max()) for t in tracks) > 0.05
    if tr == 'points':
        k = 65 // 2                                                      # the anchor outside the frame
        assert all(not t.alive[k] and (t.disp[k] == 0).all() for t in tracks)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pushes_reset_and_eager_are_bit_identical_to_the_whole_clip(name, dev):
    ref = _first(name, dev)                        # from the estimator's first replay ever
    est = _estimator(name, dev)
    frames = _frames()
    g = est.graph
    assert _same_tracks(est.track_sequence(iter(frames)), ref)            # the same clip again: reset() inside
    est.reset()
    got, n0 = [], 0
    for k in CONFIGS[name][3]:
        out = est.push_tracks(frames[n0:n0 + k])
        assert len(out) == (k if n0 else k - 1)
        got += out
        n0 += k
    assert n0 == NFRAMES and _same_tracks(got, ref)
    assert est.graph is g                                                 # one graph, never re-captured
    eager = _estimator(name, dev, use_graph=False)
    assert _same_tracks(eager.track_sequence(frames), ref) and eager.graph is None
    # another clip in between leaves nothing behind
    other = est.track_sequence(SG.clip(4, FH, FW, 62))
    assert len(other) == 3 and not _same_tracks(other, ref[:3])
    assert _same_tracks(est.track_sequence(frames), ref)


@pytest.mark.parametrize("name", ['fw-B2-dense', 'bi-B3-S3'])
def test_a_tracking_estimator_returns_what_a_plain_one_returns(name, dev):
    _first(name, dev)
    est, plain = _estimator(name, dev), _estimator(name, dev, track=False)
    frames = _frames()
    assert plain.track is False and plain.track_cap == 0 and plain.out_track_disp is None
    a, b = est.estimate_sequence(frames), plain.estimate_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    if CONFIGS[name][0] == 'bidirectional':
        a, b = est.estimate_sequence_bidirectional(frames), plain.estimate_sequence_bidirectional(frames)
        assert all(np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u, v.view(np.int32) if v.dtype == np.float32 else v)
                   for x, y in zip(a, b) for u, v in zip(x, y))
    # the other modes' methods raise as specified
    for call in (lambda: plain.push_tracks(frames[:2]), lambda: plain.track_sequence(frames)):
        with pytest.raises(RuntimeError, match="without tracks.*track=True"):
            call()
    with pytest.raises(ValueError, match="the tracks need"):
        plain.export_sequence(frames, "unused", tracks=True)
    with pytest.raises(RuntimeError, match="sequence estimator"):
        est.estimate(frames[:-1], frames[1:])


def test_pair_estimators_refuse_the_track_methods_and_the_option(dev):
    from unflow_amd.core.inference import FlowEstimator
    pair = FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev)
    for call in (lambda: pair.push_tracks([]), lambda: pair.track_sequence([])):
        with pytest.raises(RuntimeError, match="sequence=True"):
            call()
    with pytest.raises(ValueError, match="needs sequence=True"):
        FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev, track=True)
    # more tracks than the buffers hold are refused on the host, before the replay (the kernel would clamp)
    _first('fw-B3-S2', dev)
    est = _estimator('fw-B3-S2', dev)
    cap, est.track_cap = est.track_cap, 10
    try:
        est.reset()
        with pytest.raises(ValueError, match="exceed the estimator's capacity"):
            est.push_tracks(_frames()[:2])
    finally:
        est.track_cap = cap
        est.reset()
    assert _same_tracks(est.track_sequence(_frames()), _first('fw-B3-S2', dev))


# ------------------------------------------------------------------------------------------------- 3. export and the command line
def _read_flo_device(paths, h, w, dev):
    """The .flo files through the project's device reader (unflow_flo_to_flow_gt): flow [n, h, w, 2] and mask [n, h, w]."""
    from unflow_amd.core.png_device import flo_header
    L = _L()
    raw, rows = bytearray(), []
    for p in paths:
        assert flo_header(p) == (h, w)
        while len(raw) % 16:
            raw.append(0)
        with open(p, 'rb') as f:
            body = f.read()[12:]
        assert len(body) == h * w * 8
        rows.append((len(raw), 0, h, w, 8, 4, 0, 0))
        raw += body
    raw_dev = torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).to(dev)
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    flow = torch.zeros(len(paths), h, w, 2, device=dev)
    mask = torch.zeros(len(paths), h, w, device=dev)
    L.check(L.lib().unflow_flo_to_flow_gt(L.ptr(raw_dev), L.cl(len(raw)), L.ptr(table), len(paths), h, w, L.ptr(flow), L.ptr(mask),
                                          L.stream()), "flo_to_flow_gt")
    torch.cuda.synchronize()
    return flow.cpu().numpy(), mask.cpu().numpy()


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory, dev):
    """A FlowNetC checkpoint whose flows are a few tenths of a pixel at least, the frames of a clip as PNG files, a config.ini:
    (frames, their folder, the checkpoint folder, config.ini), made once for the export tests."""
    from unflow_amd.core.input import write_png_rgb8
    tmp_path = tmp_path_factory.mktemp("track_ckpt")
    from unflow_amd.core.train import Trainer
    frames = SG.clip(5, FH, FW, 50, u8=True)
    fdir = tmp_path / "frames"
    fdir.mkdir()
    for i, f in enumerate(frames):
        write_png_rgb8(str(fdir / ("f%03d.png" % i)), f)
    params = dict(flownet='C', pyramid_loss=True, border_mask=True, ternary_weight=1.0, smooth_2nd_weight=3.0,
                  learning_rate=1e-4, save_interval=1, display_interval=1)
    tr = Trainer(1, H, W, params, device=dev, seed=3, augment=False)
    tfp = tr.engine.export_tf_params()
    tfp = {k: (v * 4.0 if k.split('/')[-2] == 'flow2' and k.endswith('/weights') else v) for k, v in tfp.items()}
    tr.engine.load_tf_params(tfp)
    ckpt_dir = str(tmp_path / "ckpts" / "clipnet")
    os.makedirs(ckpt_dir)
    tr.save(ckpt_dir, 7)
    del tr
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp_path / "log", tmp_path / "ckpts"))
    return frames, str(fdir), ckpt_dir, str(cfg)


def _cli(tmp_path, fdir, cfg, out, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--out', str(tmp_path / out),
                        '--flo', '--batch', '2', '--net_size', str(H), str(W), '--config', cfg] + list(flags),
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(tmp_path / out / "clipnet")


def test_export_dense_tracks_and_cli(dev, tmp_path, checkpoint):
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence='bidirectional', track=2)
    tracks = est.track_sequence(frames)
    gh, gw = tracks[0].alive.shape
    assert (gh, gw) == (45, 76) and any(t.alive.any() for t in tracks) and not tracks[-1].alive.all()
    names = [n % i for i in range(4) for n in ('%06d_10.flo', '%06d_10_occ.png', '%06d_track.flo')]
    host = est.export_sequence(frames, str(tmp_path / "host"), fmt='flo', occlusion=True, tracks=True)
    pool = est.export_sequence(iter(frames), str(tmp_path / "pool"), fmt='flo', occlusion=True, tracks=True, workers=2)
    assert [os.path.basename(p) for p in host] == names and [os.path.basename(p) for p in pool] == names
    mine = [p for p in host if p.endswith('_track.flo')]
    flow, mask = _read_flo_device(mine, gh, gw, dev)
    for i, t in enumerate(tracks):
        assert np.array_equal(mask[i] != 0, t.alive), i                         # dead tracks read back as mask = 0
        assert np.array_equal(flow[i][t.alive].view(np.int32), t.disp[t.alive].view(np.int32)), i
        assert (flow[i][~t.alive] == np.float32(1e10)).all()
    for a, b in zip(host, pool):
        with open(a, 'rb') as fa, open(b, 'rb') as fb:
            assert fa.read() == fb.read() or a.endswith('.png'), a
    # without tracks=True the files are the ones of an estimator without tracks
    plain = est.export_sequence(frames, str(tmp_path / "plain"), fmt='flo', occlusion=True)
    assert [os.path.basename(p) for p in plain] == [n for n in names if 'track' not in n]
    # the command line, as a child process: the same files
    out = _cli(tmp_path, fdir, cfg, "cli", '--occlusion', '--track_stride', '2')
    assert sorted(os.listdir(out)) == sorted(names)
    for p in host:
        with open(os.path.join(out, os.path.basename(p)), 'rb') as fa, open(p, 'rb') as fb:
            assert fa.read() == fb.read(), p


def test_export_sparse_tracks_and_cli(dev, tmp_path, checkpoint):
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    pts = _points()
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence=True, track=pts)
    tracks = est.track_sequence(frames)
    paths = est.export_sequence(frames, str(tmp_path / "npz"), fmt='flo', tracks=True)
    assert [os.path.basename(p) for p in paths] == ['%06d_10.flo' % i for i in range(4)] + ['tracks.npz']

    def same(path):
        z = np.load(path)
        assert sorted(z.files) == ['alive', 'anchors', 'disp']
        assert z['anchors'].dtype == np.int32 and np.array_equal(z['anchors'], pts)
        assert z['disp'].dtype == np.float32 and z['disp'].shape == (4, 65, 2) and z['alive'].dtype == bool
        assert np.array_equal(z['disp'].view(np.int32), np.stack([t.disp for t in tracks]).view(np.int32))
        assert np.array_equal(z['alive'], np.stack([t.alive for t in tracks]))
    same(paths[-1])
    listing = tmp_path / "points.txt"
    listing.write_text("# x y\n" + "".join("%d %d\n" % (x, y) for x, y in pts))
    out = _cli(tmp_path, fdir, cfg, "cli", '--track_points', str(listing))
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in paths)
    same(os.path.join(out, 'tracks.npz'))
