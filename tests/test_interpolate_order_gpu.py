"""-m gpu: the consistency-ordered in-between frames — unflow_sequence_interpolate_ordered at its entry point against
the numpy definition of tests/mid_order_ref.py, pixel for pixel and count for count (equality, as for the unordered entry); order 0
against the unordered entry's bytes; what it leaves alone, and its scratch zero again; reproducibility between launches and between
graph replay and eager; prev across launches; and FlowEstimator(..., interpolate=n, interpolate_order=k) against the same definition
applied to the estimator's own flows and masks, beside a plain estimator, under held_out, through export_sequence's three writers
and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mid_order_ref as R
import mid_ref as M
import test_interpolate_gpu as TG       # Launch, the sentinels and the checkpoint fixture of the unordered entry's tests
import test_sequence_gpu as SG
from test_interpolate_gpu import checkpoint  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
CASES = R.entry_cases()
BY_ID = dict(CASES)
SENTINEL, SENTINEL_HOLES = TG.SENTINEL, TG.SENTINEL_HOLES
ERR_SHAPE, ERR_NULL = -5, -1


class Launch(TG.Launch):
    """TG.Launch through unflow_sequence_interpolate_ordered at the case's order (or order=...)."""

    def call(self, **kw):
        L, c = TG._L(), self.case
        a = dict(B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], n=c['n'], bw=self.flow_bw, ofw=None if self.occ is None else self.occ[0],
                 obw=None if self.occ is None else self.occ[1], order=c['order'])
        a.update(kw)
        return L.lib().unflow_sequence_interpolate_ordered(L.ptr(self.frames), L.ptr(self.tab), a['B'], a['Hmax'], a['Wmax'], a['n'],
                                                           L.ptr(self.flow_fw), L.ptr(a['bw']), L.ptr(a['ofw']), L.ptr(a['obw']),
                                                           L.ptr(self.prev), L.ptr(self.sums), L.ptr(self.out_mid),
                                                           L.ptr(self.out_holes), a['order'], L.stream())


# ------------------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_kernel_equals_the_mirror_at_every_pixel(cid, dev):
    """Every case of mid_order_ref.entry_cases.  out_mid and out_holes equal the mirror on every valid slot; slots that are no pairs,
    pixels outside (h, w) and the bytes behind the buffers keep their sentinels; the scratch is zero again; prev holds the last new
    frame's corner and nothing else changed in it."""
    case = BY_ID[cid]
    outs, new_prev, _ = R.mirror_of(cid)
    run = Launch(case, M.prev_of(case), dev)              # carry source 0: a poisoned prev, never read
    before = run.prev.cpu().numpy()
    assert run.run() == 0
    mid, holes = run.outputs()
    seen = R.compare(case, outs, mid, holes, SENTINEL, SENTINEL_HOLES)
    h, w, k = case['h'], case['w'], case['k']
    after = run.prev.cpu().numpy()
    assert np.array_equal(after[:h, :w], new_prev[:h, :w], equal_nan=True)
    keep = np.ones(after.shape[:2], bool)
    keep[:h, :w] = False
    assert np.array_equal(after[keep], before[keep], equal_nan=True), "prev was written outside the frame"
    print("%s: %d pixels equal, holes per (j, slot) %s" % (cid, seen, {i: o[1].tolist() for i, o in outs.items()}))
    assert seen > 0 or not case['valid']


@pytest.mark.parametrize("cid", ['ragged-n3-u8-bidir-iid12-full', 'ragged-n1-f32-fw-wild-full', 'ragged-n1-u8-fw-smooth-short'])
def test_order_zero_gives_the_unordered_entrys_bytes(cid, dev):
    case = dict(M.entry_cases())[cid]
    old = TG.Launch(case, M.prev_of(case), dev)
    new = Launch(dict(case, order=0), M.prev_of(case), dev)
    assert old.run() == 0 and new.run() == 0
    a, b = old.outputs(), new.outputs()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert old.prev.cpu().numpy().tobytes() == new.prev.cpu().numpy().tobytes()
    M.compare(case, M.mirror_of(cid)[0], *b, SENTINEL, SENTINEL_HOLES)


def test_bad_arguments_return_the_shape_error_and_write_nothing(dev):
    case = BY_ID['ragged-n3-u8-bidir-const-full-k2']
    run = Launch(case, M.prev_of(case), dev)
    before = run.prev.clone()
    for kw in (dict(order=-1), dict(order=5), dict(order=1 << 20), dict(n=0), dict(n=8), dict(B=0), dict(Hmax=0), dict(Wmax=-1),
               dict(Hmax=65536, Wmax=32768), dict(Hmax=2897, Wmax=2897), dict(bw=None), dict(ofw=None), dict(obw=None),
               dict(bw=None, ofw=None), dict(ofw=None, obw=None), dict(order=0, n=0), dict(order=0, bw=None)):
        assert run.run(**kw) == ERR_SHAPE, kw
    assert 2897 * 2897 > R.PIXELS_MAX
    assert run.untouched() and torch.equal(run.prev, before) and not bool(run.sums.any())
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_graph_replay_give_identical_bytes(dev):
    """The torn case — i.i.d. +-12 px in both directions, collisions on most targets, every conf among them: the atomics arrive in
    another order every time, the integer sums do not care.  A second launch on the same buffers and a captured graph replayed
    twice all give the eager launch's bytes."""
    case = BY_ID['ragged-n3-u8-bidir-iid12-full-k1']
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
    R.compare(case, R.mirror_of(case['id'])[0], *got, SENTINEL, SENTINEL_HOLES)


# ------------------------------------------------------------------------------------------------- 3. prev across launches
@pytest.mark.parametrize("u8,bidir,order", [(True, False, 2), (False, True, 1)], ids=['u8-fw-k2', 'f32-bidir-k1'])
def test_a_clip_pushed_in_replays_of_different_lengths(u8, bidir, order, dev):
    """Nine frames through B = 3 slots in pushes of 2, 3, 1, 1, 2: prev lives in ONE device buffer from launch to launch (poisoned
    before the first) — every pair's in-between frames equal the mirror's on the same flows, and equal those of the same clip pushed
    three at a time."""
    from unflow_amd.core.inference import sequence_tables
    shape = M.RAGGED
    B, Hm, Wm, h, w, n, T = shape['B'], shape['Hmax'], shape['Wmax'], shape['h'], shape['w'], 3 if bidir else 1, 9
    rs = M.WP._rs('mid-order-clip', u8, bidir)
    clip = M.draw_frames(rs, T - 1, Hm, Wm, h, w, u8)
    fw = M.draw_flows(rs, T - 1, Hm, Wm, h, w, 'const')
    fw[:, 5:h - 5:3, 4:w - 4:2] += (rs.rand(*fw[:, 5:h - 5:3, 4:w - 4:2].shape) * 6 - 3).astype(np.float32)    # consistent and torn pixels
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
                        flow_fw=pick(fw), flow_bw=pick(bw), order=order,
                        occ=None if occ is None else np.ascontiguousarray(occ[:, idx]))
            run = Launch(case, None, dev)
            if dev_prev is not None:
                run.prev = dev_prev
            assert run.run() == 0
            outs, host_prev, _ = R.replay(case, host_prev if carry else None)
            mid, holes = run.outputs()
            R.compare(case, outs, mid, holes, SENTINEL, SENTINEL_HOLES)
            got += [(mid[:, i, :h, :w].copy(), holes[:, i].copy()) for i in valid]
            mirror += [outs[i] for i in valid]
            dev_prev, carry, n0 = run.prev, nxt, n0 + k
        assert n0 == T and len(got) == T - 1
        return dict(enumerate(got)), dict(enumerate(mirror))
    ragged, mirror = pushed((2, 3, 1, 1, 2))
    assert TG._same(ragged, mirror)
    whole, _ = pushed((3, 3, 3))
    assert TG._same(ragged, whole)


# ------------------------------------------------------------------------------------------------- 4. the estimator
H, W, FH, FW, NFRAMES, MAXF = TG.H, TG.W, TG.FH, TG.FW, TG.NFRAMES, TG.MAXF
CONFIGS = {                             # sequence, batch, n, order, uint8 frames, the pushes of the short-push run (5 frames)
    'fw-B2-n1-k2-u8': (True, 2, 1, 2, True, (2, 1, 2)),
    'bi-B2-n3-k1-f32': ('bidirectional', 2, 3, 1, False, (1, 2, 2)),
}
_EST, _FIRST = {}, {}


def _frames(name):
    return SG.clip(NFRAMES, FH, FW, 71, u8=CONFIGS[name][4])


def _estimator(name, dev, use_graph=True, kind='ordered'):
    """The estimator of a configuration, built once.  kind: 'ordered', 'held' (ordered and held_out), 'plain' (no interpolate)."""
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, kind)
    if key not in _EST:
        seq, B, n, order, _, _ = CONFIGS[name]
        opts = dict(plain={}, ordered=dict(interpolate=n, interpolate_order=order),
                    held=dict(interpolate=n, interpolate_order=order, held_out=True))[kind]
        est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=MAXF, device=dev, sequence=seq, use_graph=use_graph, **opts)
        tfp = SG._params(est, 'C')
        if seq == 'bidirectional':
            est.load_tf_params({k: (v * TG.HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                                for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _first(name, dev):
    """interpolate_sequence of the whole clip as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, 'ordered') not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None and est.interpolate_order == CONFIGS[name][3]
        _FIRST[name] = est.interpolate_sequence(_frames(name))
        assert est.graph is not None
    return _FIRST[name]


def _mirror(name, est, frames):
    """The mirror on the estimator's own flows and masks: [(mid, holes)] per pair."""
    seq, B, n, order, u8, _ = CONFIGS[name]
    if seq == 'bidirectional':
        both = est.estimate_sequence_bidirectional(frames)
    else:
        both = [(f, None, None, None) for f in est.estimate_sequence(frames)]
    out = []
    for i, (fw, bw, ofw, obw) in enumerate(both):
        mask = lambda o: None if o is None else np.ascontiguousarray(o.astype(np.uint8))       # noqa: E731
        im0, im1 = (np.ascontiguousarray(f if u8 else np.asarray(f, np.float32)) for f in frames[i:i + 2])
        out.append(R.interpolate_pair(im0, im1, fw, bw, mask(ofw), mask(obw), FH, FW, n, order)[:2])
    return out, both


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_estimator_is_the_mirror_on_its_own_flows(name, dev):
    from unflow_amd.core.inference import Interpolated
    seq, B, n, order, u8, _ = CONFIGS[name]
    mids = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    assert len(mids) == NFRAMES - 1 and all(isinstance(m, Interpolated) for m in mids)
    want, both = _mirror(name, est, frames)
    differs = 0
    for i, (m, (mid, holes)) in enumerate(zip(mids, want)):
        assert m.frames.shape == (n, FH, FW, 3) and m.frames.dtype == np.uint8 and m.holes.shape == (n,)
        bad = np.argwhere((m.frames != mid).any(-1))
        assert len(bad) == 0, (name, i, len(bad), bad[:4])
        assert np.array_equal(m.holes, holes), (name, i, m.holes, holes)
        fw, bw, ofw, obw = both[i]
        mask = lambda o: None if o is None else np.ascontiguousarray(o.astype(np.uint8))       # noqa: E731
        im0, im1 = (np.ascontiguousarray(f if u8 else np.asarray(f, np.float32)) for f in frames[i:i + 2])
        plain_mid, plain_holes, _ = M.interpolate_pair(im0, im1, fw, bw, mask(ofw), mask(obw), FH, FW, n)
        assert np.array_equal(plain_holes, holes)         # the holes are the unordered definition's
        differs += int((plain_mid != mid).any(-1).sum())
    assert differs > 100                                  # and the frames are not: the ordered entry ran
    # the flows are a plain estimator's, bit for bit
    plain = _estimator(name, dev, kind='plain')
    a, b = est.estimate_sequence(frames), plain.estimate_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    assert plain.interpolate_order == 0 and plain.mid_sums is None


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_eager_first_replay_and_later_replays_are_bit_identical(name, dev):
    ref = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    g = est.graph
    assert TG._same_mids(est.interpolate_sequence(iter(frames)), ref)       # later replays of the captured graph
    est.reset()
    got, n0 = [], 0
    for k in CONFIGS[name][5]:
        got += est.push_interpolated(frames[n0:n0 + k])
        n0 += k
    assert n0 == NFRAMES and TG._same_mids(got, ref) and est.graph is g
    eager = _estimator(name, dev, use_graph=False)
    assert TG._same_mids(eager.interpolate_sequence(frames), ref) and eager.graph is None
    assert not bool(est.mid_sums.any()) and not bool(eager.mid_sums.any())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_held_out_scores_the_ordered_frames(name, dev):
    """held_out=True on top: the frames are the ordered estimator's, and sse is numpy's squared error of those frames against the
    held-out ones."""
    seq, B, n, order, u8, _ = CONFIGS[name]
    full = SG.clip((NFRAMES - 1) * (n + 1) + 1, FH, FW, 81, u8=u8)
    net, truths = full[::n + 1], [None] + [full[p * (n + 1) + 1:(p + 1) * (n + 1)] for p in range(NFRAMES - 1)]
    held = _estimator(name, dev, kind='held')
    held.reset()
    got, n0 = [], 0
    for k in (B,) * (NFRAMES // B) + ((NFRAMES % B,) if NFRAMES % B else ()):
        got += held.push_held_out(net[n0:n0 + k], truths[n0:n0 + k])
        n0 += k
    _first(name, dev)
    ordered = _estimator(name, dev).interpolate_sequence(net)
    assert len(got) == len(ordered) == NFRAMES - 1
    for p, (g, m) in enumerate(zip(got, ordered)):
        assert g.frames.tobytes() == m.frames.tobytes() and np.array_equal(g.holes, m.holes)
        for j in range(n):
            t = np.asarray(truths[p + 1][j])
            # the truth's byte: the byte itself, or the quantised fp32 colour rounded to one, (q(c) + 128) / 256
            tb = t.astype(np.int64) if u8 else (R.quant(np.ascontiguousarray(t, np.float32)) + 128) // 256
            assert int(g.sse[j, 0]) == int(((g.frames[j].astype(np.int64) - tb) ** 2).sum()), (name, p, j)
        assert (g.sse[:, 0] > 0).all()


def test_the_option_is_checked(dev):
    from unflow_amd.core.inference import FlowEstimator
    with pytest.raises(ValueError, match="interpolate_order.*needs interpolate"):
        FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev, sequence=True, interpolate_order=2)
    for bad in (5, -1, 2.0, '1', True):
        with pytest.raises(ValueError, match="interpolate_order"):
            FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev, sequence=True, interpolate=1, interpolate_order=bad)


# ------------------------------------------------------------------------------------------------- 5. files and the command line
def test_export_writes_the_ordered_frames_through_the_three_writers(dev, tmp_path, checkpoint):  # noqa: F811
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence='bidirectional', interpolate=2, interpolate_order=3)
    mids = est.interpolate_sequence(frames)
    assert len(mids) == 3
    names = [n % ((i,) * n.count('%')) for i in range(3) for n in ('%06d_10.png', '%06d_10_occ.png', '%06d_mid1.png', '%06d_mid2.png')]
    host = est.export_sequence(frames, str(tmp_path / "host"), occlusion=True, interpolate=True)
    pool = est.export_sequence(iter(frames), str(tmp_path / "pool"), occlusion=True, interpolate=True, workers=2)
    dev_z = est.export_sequence(frames, str(tmp_path / "devz"), occlusion=True, interpolate=True, workers=2, deflate='device')
    for paths in (host, pool, dev_z):
        assert [os.path.basename(p) for p in paths] == names
        for i, m in enumerate(mids):
            for j in (1, 2):
                got = TG._decoded(os.path.join(os.path.dirname(paths[0]), '%06d_mid%d.png' % (i, j)))
                assert got.dtype == np.uint8 and np.array_equal(got, m.frames[j - 1]), (paths[0], i, j)


def test_the_command_line_takes_order(dev, tmp_path, checkpoint):  # noqa: F811
    """python -m unflow_amd.sequence --interpolate 1 --order 2, as a child process, one direction: the files of such an estimator,
    which are not the files of the unordered one."""
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    kw = dict(net_size=(H, W), max_frame=(FH, FW), device=dev, sequence=True, interpolate=1)
    want = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, interpolate_order=2, **kw).interpolate_sequence(frames)
    plain = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, **kw).interpolate_sequence(frames)
    assert not TG._same_mids(want, plain)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--out', str(tmp_path / "cli"),
                        '--batch', '2', '--net_size', str(H), str(W), '--config', cfg, '--interpolate', '1', '--order', '2'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(out)) == sorted(n % i for i in range(3) for n in ('%06d_10.png', '%06d_mid1.png'))
    for i, m in enumerate(want):
        assert np.array_equal(TG._decoded(os.path.join(out, '%06d_mid1.png' % i)), m.frames[0]), i
