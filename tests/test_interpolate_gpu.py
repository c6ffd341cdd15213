"""-m gpu: in-between frames along a clip — unflow_sequence_interpolate at its entry point against the numpy
definition of tests/mid_ref.py, pixel for pixel and count for count (equality: the fp32 steps are rounded one by one on both sides
and the sums are integers); what it leaves alone, and its scratch zero again; reproducibility between launches and between graph
replay and eager; prev across launches; and FlowEstimator(..., sequence=..., interpolate=n) against the same definition applied to
the estimator's own flows and masks, across pushes / reset / graph and eager, beside a plain estimator, and through
export_sequence's two writers and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mid_ref as M
import test_sequence_gpu as SG          # clip(), _params() and the shared parameter cache of the sequence tests

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
CASES = M.entry_cases()
BY_ID = dict(CASES)
SENTINEL, SENTINEL_HOLES, TAIL = 0xA5, -777, 4096
ERR_SHAPE, ERR_NULL = -5, -1


def _L():
    from unflow_amd import _lib
    return _lib


def _poison(shape, u8, dev):
    """A prev that must not be read: NaN (fp32; one read would reach the output through the blend) or a byte pattern."""
    return torch.full(shape, 0xEE, dtype=torch.uint8, device=dev) if u8 else torch.full(shape, float('nan'), device=dev)


class Launch:
    """The device buffers of one case, the outputs filled with sentinels (and a tail behind them), and the call."""

    def __init__(self, case, prev, dev):
        L, c = _L(), case
        self.case, self.dev = case, dev
        n, B, Hm, Wm = c['n'], c['B'], c['Hmax'], c['Wmax']
        self.frames = torch.from_numpy(c['frames']).to(dev)
        self.tab = torch.from_numpy(c['tab']).to(dev)
        self.flow_fw = torch.from_numpy(c['flow_fw']).to(dev)
        self.flow_bw = None if c['flow_bw'] is None else torch.from_numpy(c['flow_bw']).to(dev)
        self.occ = None if c['occ'] is None else torch.from_numpy(c['occ']).to(dev)
        self.prev = _poison((Hm, Wm, 3), c['u8'], dev) if prev is None else torch.from_numpy(prev).to(dev)
        nbytes = int(L.lib().unflow_sequence_interpolate_workspace_bytes(n, B, Hm, Wm))
        assert nbytes == n * B * Hm * Wm * 32
        self.sums = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
        self.npx = n * B * Hm * Wm * 3
        self.out_mid = torch.full((self.npx + TAIL,), SENTINEL, dtype=torch.uint8, device=dev)
        self.out_holes = torch.full((n * B + 8,), SENTINEL_HOLES, dtype=torch.int32, device=dev)

    def call(self, **kw):
        L, c = _L(), self.case
        a = dict(B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], n=c['n'], bw=self.flow_bw, ofw=None if self.occ is None else self.occ[0],
                 obw=None if self.occ is None else self.occ[1])
        a.update(kw)
        return L.lib().unflow_sequence_interpolate(L.ptr(self.frames), L.ptr(self.tab), a['B'], a['Hmax'], a['Wmax'], a['n'],
                                                   L.ptr(self.flow_fw), L.ptr(a['bw']), L.ptr(a['ofw']), L.ptr(a['obw']),
                                                   L.ptr(self.prev), L.ptr(self.sums), L.ptr(self.out_mid), L.ptr(self.out_holes),
                                                   L.stream())

    def run(self, **kw):
        st = self.call(**kw)
        torch.cuda.synchronize()
        return st

    def outputs(self):
        """(out_mid [n, B, Hmax, Wmax, 3], out_holes [n, B]) on the host; the tails behind them still hold the sentinels and the
        scratch is all zero."""
        c = self.case
        n, B = c['n'], c['B']
        mid, holes = self.out_mid.cpu().numpy(), self.out_holes.cpu().numpy()
        assert (mid[self.npx:] == SENTINEL).all() and (holes[n * B:] == SENTINEL_HOLES).all(), "rows beyond B were written"
        assert not bool(self.sums.any()), "the scratch is not zero after the launch"
        return mid[:self.npx].reshape(n, B, c['Hmax'], c['Wmax'], 3), holes[:n * B].reshape(n, B)

    def untouched(self):
        return bool((self.out_mid == SENTINEL).all()) and bool((self.out_holes == SENTINEL_HOLES).all())


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]) for i in a)


# ------------------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_kernel_equals_the_mirror_at_every_pixel(cid, dev):
    """Every case of mid_ref.entry_cases: the pitch that is not the width, n in {1, 3}, uint8 and fp32 frames, one and both
    directions with blob masks, the four flow kinds, every replay pattern, one pair past the grid's cap.  out_mid and out_holes equal
    the mirror on every valid slot; slots that are no pairs, pixels outside (h, w) and the bytes behind the buffers keep their
    sentinels; the scratch is zero again; prev holds the last new frame's corner and nothing else changed in it."""
    case = BY_ID[cid]
    outs, new_prev, _ = M.mirror_of(cid)
    prev = M.prev_of(case)
    run = Launch(case, prev, dev)                         # carry source 0: a poisoned prev, never read
    before = run.prev.cpu().numpy()
    assert run.run() == 0
    mid, holes = run.outputs()
    seen = M.compare(case, outs, mid, holes, SENTINEL, SENTINEL_HOLES)
    h, w, k = case['h'], case['w'], case['k']
    after = run.prev.cpu().numpy()
    assert np.array_equal(after[:h, :w], case['frames'][k - 1, :h, :w]) and np.array_equal(after[:h, :w], new_prev[:h, :w])
    keep = np.ones(after.shape[:2], bool)
    keep[:h, :w] = False
    assert np.array_equal(after[keep], before[keep], equal_nan=True), "prev was written outside the frame"
    print("%s: %d pixels equal, holes per (j, slot) %s" % (cid, seen, {i: o[1].tolist() for i, o in outs.items()}))
    assert seen > 0 or not case['valid']


def test_bad_arguments_return_the_shape_error_and_write_nothing(dev):
    case = BY_ID['ragged-n3-u8-bidir-const-full']
    run = Launch(case, M.prev_of(case), dev)
    before = run.prev.clone()
    for kw in (dict(n=0), dict(n=8), dict(n=-1), dict(B=0), dict(B=-2), dict(Hmax=0), dict(Wmax=-1), dict(Hmax=65536, Wmax=32768),
               dict(bw=None), dict(ofw=None), dict(obw=None), dict(bw=None, ofw=None), dict(ofw=None, obw=None)):
        assert run.run(**kw) == ERR_SHAPE, kw
    assert run.untouched() and torch.equal(run.prev, before) and not bool(run.sums.any())
    # a pair slot whose frame exceeds the buffers is no pair; the others are what they were
    tab = case['tab'].copy()
    tab[8 * case['B'] + 8 + 1] = case['Wmax'] + 1
    odd = Launch(dict(case, tab=tab, valid=[0, 2]), M.prev_of(case), dev)
    assert odd.run() == 0
    outs = M.mirror_of(case['id'])[0]
    M.compare(odd.case, {i: outs[i] for i in (0, 2)}, *odd.outputs(), SENTINEL, SENTINEL_HOLES)
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_graph_replay_give_identical_bytes(dev):
    """The torn case — i.i.d. +-12 px in both directions, collisions on most targets: the atomics arrive in another order every
    time, the integer sums do not care.  A second launch on the same buffers (the scratch left zero by the first; prev put back)
    and a captured graph replayed twice all give the eager launch's bytes."""
    case = BY_ID['ragged-n3-u8-bidir-iid12-full']
    eager = Launch(case, M.prev_of(case), dev)
    assert eager.run() == 0
    first = [t.copy() for t in eager.outputs()]
    eager.out_mid.fill_(SENTINEL)
    eager.prev.copy_(torch.from_numpy(case['prev']))      # the first launch left the clip's last frame there
    assert eager.run() == 0
    again = eager.outputs()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    cap = Launch(case, M.prev_of(case), dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert cap.call() == 0
    torch.cuda.current_stream(dev).wait_stream(s)
    assert cap.untouched()                                # captured, not run
    for _ in range(2):
        cap.out_mid.fill_(SENTINEL)
        cap.prev.copy_(torch.from_numpy(case['prev']))
        g.replay()
        torch.cuda.synchronize()
        got = cap.outputs()
        assert np.array_equal(first[0], got[0]) and np.array_equal(first[1], got[1])
    M.compare(case, M.mirror_of(case['id'])[0], *got, SENTINEL, SENTINEL_HOLES)


# ------------------------------------------------------------------------------------------------- 3. prev across launches
@pytest.mark.parametrize("u8,bidir", [(True, False), (False, True)], ids=['u8-fw', 'f32-bidir'])
def test_a_clip_pushed_in_replays_of_different_lengths(u8, bidir, dev):
    """Nine frames through B = 3 slots in pushes of 2, 3, 1, 1, 2: prev lives in ONE device buffer from launch to launch (poisoned
    before the first), the host overwrites the frames before each — every pair's in-between frames equal the mirror's on the same
    flows, and equal those of the same clip pushed three at a time."""
    from unflow_amd.core.inference import sequence_tables
    shape = M.RAGGED
    B, Hm, Wm, h, w, n, T = shape['B'], shape['Hmax'], shape['Wmax'], shape['h'], shape['w'], 3 if bidir else 1, 9
    rs = M.WP._rs('mid-clip', u8, bidir)
    clip = M.draw_frames(rs, T - 1, Hm, Wm, h, w, u8)
    fw = M.draw_flows(rs, T - 1, Hm, Wm, h, w, 'iid12')
    bw = M.draw_flows(rs, T - 1, Hm, Wm, h, w, 'smooth') if bidir else None
    occ = np.stack([M.T.draw_occ(rs, T - 1, Hm, Wm, h, w) for _ in range(2)]) if bidir else None

    def pushed(pushes):
        got, mirror, carry, n0, dev_prev, host_prev = [], [], 0, 0, None, None
        for k in pushes:
            tab, valid, nxt = sequence_tables((h, w), k, B, carry, u8=u8)
            fr = np.full((B, Hm, Wm, 3), 77, clip.dtype)             # slots beyond the new frames: stale bytes
            fr[:k] = clip[n0:n0 + k]
            idx = [min(max(n0 - 1 + i, 0), T - 2) for i in range(B)]        # pair slot i = pair n0 - 1 + i of the clip
            pick = lambda a: None if a is None else np.ascontiguousarray(a[idx])       # noqa: E731
            case = dict(B=B, Hmax=Hm, Wmax=Wm, h=h, w=w, n=n, u8=u8, k=k, carry=carry, tab=tab, valid=valid, frames=fr,
                        flow_fw=pick(fw), flow_bw=pick(bw),
                        occ=None if occ is None else np.ascontiguousarray(occ[:, idx]))
            run = Launch(case, None, dev)
            if dev_prev is not None:
                run.prev = dev_prev
            assert run.run() == 0
            outs, host_prev, _ = M.replay(case, host_prev if carry else None)
            mid, holes = run.outputs()
            M.compare(case, outs, mid, holes, SENTINEL, SENTINEL_HOLES)
            got += [(mid[:, i, :h, :w].copy(), holes[:, i].copy()) for i in valid]
            mirror += [outs[i] for i in valid]
            dev_prev, carry, n0 = run.prev, nxt, n0 + k
        assert n0 == T and len(got) == T - 1
        return dict(enumerate(got)), dict(enumerate(mirror))
    ragged, mirror = pushed((2, 3, 1, 1, 2))
    assert _same(ragged, mirror)
    whole, _ = pushed((3, 3, 3))
    assert _same(ragged, whole)
    assert sum(int(v[1].sum()) for v in whole.values()) > 100


def test_carry_source_zero_never_reads_prev(dev):
    """Slot 0 marked a pair in the table while the carry source is 0 (a table no estimator writes): it is no pair, and the NaN in
    prev reaches nothing."""
    case = BY_ID['ragged-n3-f32-bidir-smooth-first']
    assert not case['u8'] and case['carry'] == 0 and case['valid'] == [1, 2]
    tab = case['tab'].copy()
    tab[8 * case['B']:8 * case['B'] + 8] = tab[8 * case['B'] + 8:8 * case['B'] + 16]
    run = Launch(dict(case, tab=tab), None, dev)
    assert bool(torch.isnan(run.prev).all()) and run.run() == 0
    M.compare(case, M.mirror_of(case['id'])[0], *run.outputs(), SENTINEL, SENTINEL_HOLES)


# ------------------------------------------------------------------------------------------------- 5. the estimator
H, W, FH, FW, NFRAMES = 64, 128, 90, 151, 5
MAXF = (96, 160)                        # the estimator's buffers are wider than the frames: the pitch is not the width
CONFIGS = {                             # sequence, batch, n, uint8 frames, the pushes of the short-push run (5 frames)
    'fw-B2-n1-u8': (True, 2, 1, True, (2, 1, 2)),
    'bi-B2-n3-f32': ('bidirectional', 2, 3, False, (1, 2, 2)),
}
HEAD_SCALE = 0.1
_EST, _FIRST = {}, {}


def _frames(name):
    return SG.clip(NFRAMES, FH, FW, 71, u8=CONFIGS[name][3])


def _estimator(name, dev, use_graph=True, interpolate=True):
    """The estimator of a configuration, built once; interpolate=False: the same estimator without the option."""
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, interpolate)
    if key not in _EST:
        seq, B, n, _, _ = CONFIGS[name]
        est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=MAXF, device=dev, sequence=seq, use_graph=use_graph,
                            interpolate=n if interpolate else None)
        tfp = SG._params(est, 'C')
        if seq == 'bidirectional':
            # untrained forward and backward flows disagree and the masks cover nearly every pixel; flow heads at a tenth leave
            # both occluded and blended pixels (tests/test_track_gpu.py)
            est.load_tf_params({k: (v * HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                                for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _first(name, dev):
    """interpolate_sequence of the whole clip as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, True) not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None
        _FIRST[name] = est.interpolate_sequence(_frames(name))
        assert est.graph is not None
    return _FIRST[name]


def _same_mids(a, b):
    return len(a) == len(b) and all(np.array_equal(x.frames, y.frames) and np.array_equal(x.holes, y.holes) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_interpolate_sequence_is_the_mirror_on_the_estimators_own_flows(name, dev):
    from unflow_amd.core.inference import Interpolated
    seq, B, n, u8, _ = CONFIGS[name]
    mids = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    assert len(mids) == NFRAMES - 1 and all(isinstance(m, Interpolated) for m in mids)
    if seq == 'bidirectional':
        both = est.estimate_sequence_bidirectional(frames)
    else:
        both = [(f, None, None, None) for f in est.estimate_sequence(frames)]
    for i, (m, (fw, bw, ofw, obw)) in enumerate(zip(mids, both)):
        assert m.frames.shape == (n, FH, FW, 3) and m.frames.dtype == np.uint8 and m.holes.shape == (n,)
        mask = lambda o: None if o is None else np.ascontiguousarray(o.astype(np.uint8))       # noqa: E731
        im0, im1 = (np.ascontiguousarray(f if u8 else np.asarray(f, np.float32)) for f in frames[i:i + 2])
        want, holes, _ = M.interpolate_pair(im0, im1, fw, bw, mask(ofw), mask(obw), FH, FW, n)
        bad = np.argwhere((m.frames != want).any(-1))
        assert len(bad) == 0, (name, i, len(bad), bad[:4])
        assert np.array_equal(m.holes, holes), (name, i, m.holes, holes)
        if ofw is not None:
            print("%s pair %d: occluded fw %.2f bw %.2f, holes %s" % (name, i, ofw.mean(), obw.mean(), holes.tolist()))
    if seq == 'bidirectional':
        assert any(0.02 < b.occ_fw.mean() < 0.98 for b in both)            # occluded and blended pixels both occur


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pushes_reset_and_eager_are_bit_identical_to_the_whole_clip(name, dev):
    ref = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    g = est.graph
    assert _same_mids(est.interpolate_sequence(iter(frames)), ref)         # the same clip again: reset() inside
    est.reset()
    got, n0 = [], 0
    for k in CONFIGS[name][4]:
        out = est.push_interpolated(frames[n0:n0 + k])
        assert len(out) == (k if n0 else k - 1)
        got += out
        n0 += k
    assert n0 == NFRAMES and _same_mids(got, ref)
    assert est.graph is g                                                  # one graph, never re-captured
    eager = _estimator(name, dev, use_graph=False)
    assert _same_mids(eager.interpolate_sequence(frames), ref) and eager.graph is None
    # another clip in between leaves nothing behind: after reset() the frame kept from it is not used
    other = est.interpolate_sequence(SG.clip(3, FH, FW, 72, u8=CONFIGS[name][3]))
    assert len(other) == 2 and not _same_mids(other, ref[:2])
    assert _same_mids(est.interpolate_sequence(frames), ref)
    assert not bool(est.mid_sums.any())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_an_interpolating_estimator_returns_what_a_plain_one_returns(name, dev):
    _first(name, dev)
    est, plain = _estimator(name, dev), _estimator(name, dev, interpolate=False)
    frames = _frames(name)
    assert plain.interpolate == 0 and plain.out_mid is None and plain.mid_sums is None and plain.mid_prev is None
    a, b = est.estimate_sequence(frames), plain.estimate_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    if CONFIGS[name][0] == 'bidirectional':
        a, b = est.estimate_sequence_bidirectional(frames), plain.estimate_sequence_bidirectional(frames)
        assert all(np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u, v.view(np.int32) if v.dtype == np.float32 else v)
                   for x, y in zip(a, b) for u, v in zip(x, y))
    for call in (lambda: plain.push_interpolated(frames[:2]), lambda: plain.interpolate_sequence(frames)):
        with pytest.raises(RuntimeError, match="without in-between frames.*interpolate=n"):
            call()
    with pytest.raises(ValueError, match="in-between frames need"):
        plain.export_sequence(frames, "unused", interpolate=True)
    with pytest.raises(RuntimeError, match="sequence estimator"):
        est.estimate(frames[:-1], frames[1:])


def test_the_option_is_checked(dev):
    from unflow_amd.core.inference import FlowEstimator
    with pytest.raises(ValueError, match="needs sequence=True"):
        FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev, interpolate=1)
    for bad in (0, 8, -1, 2.0, '1', True):
        with pytest.raises(ValueError, match="1 to 7"):
            FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev, sequence=True, interpolate=bad)
    pair = FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev)
    for call in (lambda: pair.push_interpolated([]), lambda: pair.interpolate_sequence([])):
        with pytest.raises(RuntimeError, match="sequence=True"):
            call()


# ------------------------------------------------------------------------------------------------- 6. files and the command line
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory, dev):
    """A FlowNetC checkpoint whose flows are a few tenths of a pixel at least, the frames of a clip as PNG files, a config.ini:
    (frames, their folder, the checkpoint folder, config.ini), made once for the export tests (tests/test_track_gpu.py's)."""
    from unflow_amd.core.input import write_png_rgb8
    from unflow_amd.core.train import Trainer
    tmp_path = tmp_path_factory.mktemp("mid_ckpt")
    frames = SG.clip(4, FH, FW, 50, u8=True)
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


def _decoded(path):
    from unflow_amd.core.input import decode_png
    with open(path, 'rb') as f:
        return decode_png(f.read())


def test_export_writes_the_returned_frames_through_both_writers(dev, tmp_path, checkpoint):
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence='bidirectional', interpolate=2)
    mids = est.interpolate_sequence(frames)
    assert len(mids) == 3 and any((m.frames[0] != m.frames[1]).any() for m in mids)
    names = [n % ((i,) * n.count('%')) for i in range(3) for n in ('%06d_10.png', '%06d_10_occ.png', '%06d_mid1.png', '%06d_mid2.png')]
    host = est.export_sequence(frames, str(tmp_path / "host"), occlusion=True, interpolate=True)
    pool = est.export_sequence(iter(frames), str(tmp_path / "pool"), occlusion=True, interpolate=True, workers=2)
    dev_z = est.export_sequence(frames, str(tmp_path / "devz"), occlusion=True, interpolate=True, workers=2, deflate='device')
    for paths in (host, pool, dev_z):
        assert [os.path.basename(p) for p in paths] == names
        for i, m in enumerate(mids):
            for j in (1, 2):
                got = _decoded(os.path.join(os.path.dirname(paths[0]), '%06d_mid%d.png' % (i, j)))
                assert got.dtype == np.uint8 and np.array_equal(got, m.frames[j - 1]), (paths[0], i, j)
    for a, b, c in zip(host, pool, dev_z):                                  # every file decodes to identical pixels
        assert np.array_equal(_decoded(a), _decoded(b)) and np.array_equal(_decoded(a), _decoded(c)), a
    # without interpolate=True the files are the ones of an estimator without the option
    plain = est.export_sequence(frames, str(tmp_path / "plain"), occlusion=True)
    assert [os.path.basename(p) for p in plain] == [n for n in names if 'mid' not in n]


def test_the_command_line_writes_the_same_files(dev, tmp_path, checkpoint):
    """python -m unflow_amd.sequence --interpolate 1, as a child process, one direction: the files of such an estimator."""
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    one = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence=True, interpolate=1)
    want = one.interpolate_sequence(frames)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--out', str(tmp_path / "cli"),
                        '--batch', '2', '--net_size', str(H), str(W), '--config', cfg, '--interpolate', '1'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(out)) == sorted(n % i for i in range(3) for n in ('%06d_10.png', '%06d_mid1.png'))
    for i, m in enumerate(want):
        assert np.array_equal(_decoded(os.path.join(out, '%06d_mid1.png' % i)), m.frames[0]), i
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--config', cfg,
                        '--interpolate', '8'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and '1 to 7' in r.stderr
