"""-m gpu: temporal denoising along a clip — unflow_sequence_denoise at its entry point against the numpy definition of
tests/denoise_ref.py, byte for byte on out_den, out_stats and the state (equality: everything is an integer but the flow's
validity test and one rintf per component); what it leaves alone, and its histogram words zero again; reproducibility between
launches and between graph replay and eager; the history across launches; and FlowEstimator(..., sequence='bidirectional',
denoise=...) against the same definition applied to the estimator's own backward flows and masks, beside a plain estimator, with
track, interpolate and stabilise on, and through export_sequence's three writers and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import denoise_ref as R
import test_interpolate_gpu as TG       # the estimator shapes, _decoded and the checkpoint fixture of the in-between frames' tests
import test_sequence_gpu as SG          # clip(), _params() and the shared parameter cache of the sequence tests
from test_interpolate_gpu import checkpoint  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
CASES = R.entry_cases()
BY_ID = dict(CASES)
ERR_SHAPE, ERR_NULL = -5, -1
ROWS = 1                                 # sentinel rows behind every output and behind the state
SENTINELS = dict(den=0x5A, stats=-777)
DTYPES = dict(den=torch.uint8, stats=torch.int32)
STATE_SENTINEL = 0x3C3C


def _L():
    from unflow_amd import _lib
    return _lib


def _dev_state(state, dev):
    """A host state uint16 [Hmax, Wmax, 4] as the device buffer of a launch: int16 bits, a sentinel row behind it."""
    s = np.full((state.shape[0] + ROWS,) + state.shape[1:], STATE_SENTINEL, np.uint16)
    s[:state.shape[0]] = state
    return torch.from_numpy(s.view(np.int16)).to(dev)


def _host_state(t):
    """(the state uint16 [Hmax, Wmax, 4], the sentinel rows intact) of a device state buffer."""
    s = t.cpu().numpy().view(np.uint16)
    return s[:-ROWS], bool((s[-ROWS:] == STATE_SENTINEL).all())


class Launch:
    """The device buffers of one case, the outputs filled with sentinels (and a row of them behind each), and the call."""

    def __init__(self, case, dev, state=None):
        L, c = _L(), case
        self.case, self.dev = case, dev
        B, Hm, Wm = c['B'], c['Hmax'], c['Wmax']
        self.frames = torch.from_numpy(c['frames']).to(dev)
        self.tab = torch.from_numpy(c['tab']).to(dev)
        self.flow = torch.from_numpy(c['flow_bw']).to(dev)
        self.occ = torch.from_numpy(c['occ']).to(dev)
        self.state = _dev_state(c['state'], dev) if state is None else state
        nbytes = int(L.lib().unflow_sequence_denoise_workspace_bytes(B, Hm, Wm))
        assert nbytes == B * 1024 + 2 * Hm * Wm * 8
        self.ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        self.ws[B * 256:] = 0x6B6B6B6B                    # the history slabs need not be zero
        shapes = dict(den=(B + ROWS, Hm, Wm, 3), stats=(B + ROWS, 8))
        self.out = {k: torch.full(shapes[k], SENTINELS[k], dtype=DTYPES[k], device=dev) for k in R.OUTPUTS}

    def call(self, **kw):
        L, c = _L(), self.case
        a = dict(frames=self.frames, tab=self.tab, B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], flow=self.flow, occ=self.occ,
                 tol=c['tol'], depth=c['depth'], state=self.state, ws=self.ws, **{'out_' + k: v for k, v in self.out.items()})
        a.update(kw)
        return L.lib().unflow_sequence_denoise(L.ptr(a['frames']), L.ptr(a['tab']), a['B'], a['Hmax'], a['Wmax'], L.ptr(a['flow']),
                                               L.ptr(a['occ']), a['tol'], a['depth'], L.ptr(a['state']), L.ptr(a['ws']),
                                               L.ptr(a['out_den']), L.ptr(a['out_stats']), L.stream())

    def run(self, **kw):
        st = self.call(**kw)
        torch.cuda.synchronize()
        return st

    def outputs(self):
        """{name: the output on the host, sentinel rows included}; the histogram words of the workspace are all zero."""
        assert not bool(self.ws[:self.case['B'] * 256].any()), "the histograms are not zero after the launch"
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def left(self):
        """The state the launch left, the sentinel row behind it checked."""
        s, intact = _host_state(self.state)
        assert intact, "the row behind the state was written"
        return s

    def fill(self):
        for k, v in self.out.items():
            v.fill_(SENTINELS[k])

    def untouched(self):
        return all(bool((v == SENTINELS[k]).all()) for k, v in self.out.items())


# ------------------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_kernel_equals_the_mirror_on_both_outputs_and_the_state(cid, dev):
    """Every case of denoise_ref.entry_cases.  out_den and out_stats equal the mirror on every valid slot; slots that are no pairs,
    pixels outside (h, w) and the rows behind the buffers keep their sentinels; the state equals the mirror's in every word; the
    histogram words are zero again."""
    case = BY_ID[cid]
    outs, new_state = R.mirror_of(cid)
    run = Launch(case, dev)
    assert run.run() == 0
    seen = R.compare(case, outs, run.outputs(), SENTINELS)
    left = run.left()
    bad = np.argwhere(left != new_state)
    assert len(bad) == 0, ("the state differs at %d words, first %s: got %s, mirror %s"
                           % (len(bad), bad[0], left[tuple(bad[0])], new_state[tuple(bad[0])]))
    print("%s: %d pixels equal, stats %s" % (cid, seen, {i: o['stats'][:6].tolist() for i, o in outs.items()}))
    assert seen > 0 or not case['valid']


def test_bad_arguments_write_nothing(dev):
    case = next(c for _, c in CASES if c['name'] == 'ragged' and c['pattern'] == 'full')
    run = Launch(case, dev)
    before, ws = run.state.clone(), run.ws.clone()
    for kw in (dict(B=0), dict(B=-3), dict(B=65536), dict(Hmax=0), dict(Wmax=-1), dict(Hmax=4097), dict(Wmax=4097),
               dict(Hmax=65536, Wmax=32768), dict(tol=-2), dict(tol=5), dict(depth=0), dict(depth=65), dict(tol=1 << 20)):
        assert run.run(**kw) == ERR_SHAPE, kw
    for name in ('frames', 'tab', 'flow', 'occ', 'state', 'ws', 'out_den', 'out_stats'):
        assert run.run(**{name: None}) == ERR_NULL, name
    assert run.untouched() and torch.equal(run.state, before) and torch.equal(run.ws, ws)
    L = _L().lib()
    assert int(L.unflow_sequence_denoise_workspace_bytes(0, 40, 64)) == 0
    assert int(L.unflow_sequence_denoise_workspace_bytes(3, 40, 4097)) == 0
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_graph_replay_give_identical_bytes(dev):
    """i.i.d. +-12 px with tol = -1: the histogram's atomics arrive in another order every time; the integer sums do not care.  A
    second launch on the same buffers (the histograms left zero by the first, the state put back) and a captured graph replayed
    twice all give the eager launch's bytes."""
    case = next(c for _, c in CASES if c['kind'] == 'iid12' and c['tol'] == -1 and c['pattern'] == 'full' and c['name'] == 'ragged')
    state = _dev_state(case['state'], dev)
    eager = Launch(case, dev)
    assert eager.run() == 0
    first = eager.outputs()
    left = eager.state.clone()
    eager.fill()
    eager.state.copy_(state)
    assert eager.run() == 0
    again = eager.outputs()
    assert all(first[k].tobytes() == again[k].tobytes() for k in R.OUTPUTS) and torch.equal(eager.state, left)
    cap = Launch(case, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert cap.call() == 0
    torch.cuda.current_stream(dev).wait_stream(s)
    assert cap.untouched()                                # captured, not run
    for _ in range(2):
        cap.fill()
        cap.state.copy_(state)
        g.replay()
        torch.cuda.synchronize()
        got = cap.outputs()
        assert all(first[k].tobytes() == got[k].tobytes() for k in R.OUTPUTS) and torch.equal(cap.state, left)
    R.compare(case, R.mirror_of(case['id'])[0], got, SENTINELS)
    assert np.array_equal(cap.left(), R.mirror_of(case['id'])[1])


# ------------------------------------------------------------------------------------------------- 3. the history across launches
@pytest.mark.parametrize("u8,tol,depth", [(True, -1, 8), (False, 2, 64)], ids=['u8-auto-d8', 'f32-t2-d64'])
def test_a_clip_pushed_in_replays_of_different_lengths(u8, tol, depth, dev):
    """Nine frames through B = 3 slots in pushes of 2, 3, 1, 1, 2: the history lives in ONE device buffer from launch to launch
    (poisoned before the first) — every pair's outputs and the state behind every launch equal the mirror's on the same flows, and
    the pairs equal those of the same clip pushed three at a time."""
    from unflow_amd.core.inference import sequence_tables
    shape = R.RAGGED
    B, Hm, Wm, h, w, T = shape['B'], shape['Hmax'], shape['Wmax'], shape['h'], shape['w'], 9
    rs = R.WP._rs('denoise-clip', u8, tol, depth)
    clip = R.draw_frames(rs, T, Hm, Wm, h, w, u8)
    bw = R.draw_flows(rs, T - 1, Hm, Wm, h, w, 'shift')
    bw[:, :h, :w] += (rs.rand(T - 1, h, w, 2).astype(np.float32) - np.float32(0.5)) * np.float32(0.75)
    occ = R.draw_occ(rs, T - 1, Hm, Wm, h, w, 'blobs')

    def pushed(pushes):
        got, mirror, carry, n0 = [], [], 0, 0
        host_state = R.draw_state(rs, Hm, Wm, depth, False)
        dev_state = _dev_state(host_state, dev)
        for k in pushes:
            tab, valid, nxt = sequence_tables((h, w), k, B, carry, u8=u8)
            fr = np.full((B, Hm, Wm, 3), 77, clip.dtype)             # slots beyond the new frames: stale bytes
            fr[:k] = clip[n0:n0 + k]
            idx = [min(max(n0 - 1 + i, 0), T - 2) for i in range(B)]        # pair slot i = pair n0 - 1 + i of the clip
            case = dict(B=B, Hmax=Hm, Wmax=Wm, h=h, w=w, u8=u8, k=k, carry=carry, tab=tab, valid=valid, frames=fr,
                        flow_bw=np.ascontiguousarray(bw[idx]), occ=np.ascontiguousarray(occ[idx]), tol=tol, depth=depth,
                        state=host_state)
            run = Launch(case, dev, state=dev_state)
            assert run.run() == 0
            outs, host_state = R.replay(case, host_state)
            R.compare(case, outs, run.outputs(), SENTINELS)
            assert np.array_equal(run.left(), host_state)
            got += [dict(den=run.outputs()['den'][i, :h, :w].copy(), stats=run.outputs()['stats'][i].astype(np.int64)) for i in valid]
            mirror += [outs[i] for i in valid]
            carry, n0 = nxt, n0 + k
        assert n0 == T and len(got) == T - 1
        return got, mirror

    def same(a, b):
        return len(a) == len(b) and all(all(np.array_equal(x[k], y[k]) for k in R.OUTPUTS) for x, y in zip(a, b))
    ragged, mirror = pushed((2, 3, 1, 1, 2))
    assert same(ragged, mirror)
    whole, _ = pushed((3, 3, 3))
    assert same(ragged, whole)
    assert max(int(g['stats'][5]) for g in whole) > 2 * h * w          # longer than one pair can make it: it grows along the clip


def test_the_first_replay_twice_gives_what_one_run_gives(dev):
    """A clip's first replay: the state holds whatever another clip left; running the launch again on the state it wrote (an
    estimator's first replay ever: the eager pass, then the graph's first replay) changes nothing; and poison reaches nothing."""
    case = next(c for _, c in CASES if c['pattern'] == 'first' and c['u8'])
    assert case['carry'] == 0 and case['valid'] == [1, 2]
    a = Launch(case, dev)
    assert a.run() == 0
    x, left = a.outputs(), a.state.clone()
    a.fill()
    assert a.run() == 0
    y = a.outputs()
    assert all(x[k].tobytes() == y[k].tobytes() for k in R.OUTPUTS) and torch.equal(a.state, left)
    other = np.full_like(case['state'], 0xFFFF)
    b = Launch(case, dev, state=_dev_state(other, dev))
    assert b.run() == 0
    z = b.outputs()
    h, w = case['h'], case['w']
    assert all(x[k].tobytes() == z[k].tobytes() for k in R.OUTPUTS) and np.array_equal(b.left()[:h, :w], a.left()[:h, :w])
    R.compare(case, R.mirror_of(case['id'])[0], z, SENTINELS)
    none = next(c for _, c in CASES if c['pattern'] == 'nopairs' and c['u8'])
    n = Launch(none, dev)
    assert n.run() == 0 and n.untouched() and np.array_equal(n.left(), R.mirror_of(none['id'])[1])
    assert n.run() == 0 and np.array_equal(n.left(), R.mirror_of(none['id'])[1])


def test_slot_zero_without_a_carried_frame_is_no_pair(dev):
    """Slot 0 marked a pair in the table while the carry source is 0 (a table no estimator writes): it is no pair, and the outputs
    are the first replay's."""
    case = next(c for _, c in CASES if c['pattern'] == 'first' and not c['u8'])
    B = case['B']
    tab = case['tab'].copy()
    tab[8 * B:8 * B + 8] = tab[8 * B + 8:8 * B + 16]
    run = Launch(dict(case, tab=tab), dev)
    assert run.run() == 0
    R.compare(case, R.mirror_of(case['id'])[0], run.outputs(), SENTINELS)
    assert np.array_equal(run.left(), R.mirror_of(case['id'])[1])


# ------------------------------------------------------------------------------------------------- 4. the estimator
H, W, FH, FW, MAXF = TG.H, TG.W, TG.FH, TG.FW, TG.MAXF
NFRAMES, BATCH = 7, 3
CONFIGS = {                             # uint8 frames, the pushes of the short-push run (7 frames), the option
    'B3-u8': (True, (2, 3, 1, 1), True),
    'B3-f32': (False, (1, 3, 3), dict(tol=2, depth=4)),
}
_EST, _FIRST = {}, {}


def _static_clip(T, seed, u8):
    """T frames of one smooth, lightly textured picture, each with noise of its own (sigma 4): the frame and its prediction stay
    within the tolerance, so the history grows along the clip — on the moving random clips of the other sequence tests every
    history would be rejected and the denoised frame would be the frame."""
    rs = R.WP._rs('denoise-static', seed)
    base = R.draw_frames(rs, 1, FH, FW, FH, FW, False, sigma=0.0)[0].astype(np.float64)
    fr = [np.clip(base + rs.randn(FH, FW, 3) * 4.0, 0, 255) for _ in range(T)]
    return [np.rint(f).astype(np.uint8) if u8 else f.astype(np.float32) for f in fr]


def _frames(name):
    return _static_clip(NFRAMES, 73, CONFIGS[name][0])


def _estimator(name, dev, use_graph=True, kind='den'):
    """The estimator of a configuration, built once.  kind: 'den'; 'plain' (no option); 'all' (denoise, track, interpolate and
    stabilise); 'others' (track, interpolate and stabilise alone)."""
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, kind)
    if key not in _EST:
        opt = CONFIGS[name][2]
        others = dict(track=4, interpolate=1, stabilise=True)
        opts = dict(plain={}, den=dict(denoise=opt), all=dict(denoise=opt, **others), others=others)[kind]
        est = FlowEstimator(dict(flownet='C'), BATCH, net_size=(H, W), max_frame=MAXF, device=dev, sequence='bidirectional',
                            use_graph=use_graph, **opts)
        tfp = SG._params(est, 'C')      # flow heads at a tenth leave both occluded and visible pixels (tests/test_track_gpu.py)
        est.load_tf_params({k: (v * TG.HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                            for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _first(name, dev):
    """denoise_sequence of the whole clip as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, 'den') not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None
        _FIRST[name] = est.denoise_sequence(_frames(name))
        assert est.graph is not None
    return _FIRST[name]


def _same_den(a, b):
    return len(a) == len(b) and all(np.array_equal(x.frame, y.frame) and (x.noise, x.tol, x.counts) == (y.noise, y.tol, y.counts)
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_estimator_is_the_mirror_on_its_own_flows(name, dev):
    from unflow_amd.core.inference import DENOISE_DEFAULTS, Denoised
    u8, _, opt = CONFIGS[name]
    o = dict(DENOISE_DEFAULTS, **(opt if isinstance(opt, dict) else {}))
    got = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    assert len(got) == NFRAMES - 1 and all(isinstance(s, Denoised) for s in got) and est.denoise == o
    both = est.estimate_sequence_bidirectional(frames)
    print("%s: occluded %s" % (name, [round(float(b.occ_bw.mean()), 4) for b in both]))
    as_f32 = lambda f: np.ascontiguousarray(f if u8 else np.asarray(f, np.float32))     # noqa: E731
    hist = R.initial(np.zeros((FH, FW, 4), np.int64), as_f32(frames[0]), FH, FW, FH, FW)
    tol = -1 if o['tol'] == 'auto' else o['tol']
    for i, (s, b) in enumerate(zip(got, both)):
        want, hist = R.denoise_pair(as_f32(frames[i + 1]), b.flow_bw, b.occ_bw.astype(np.uint8), FH, FW, tol, o['depth'], hist)
        st = want['stats']
        assert s.frame.shape == (FH, FW, 3) and s.frame.dtype == np.uint8
        assert (s.tol, s.noise) == (int(st[0]), int(st[1])), (name, i, s.tol, s.noise, st)
        assert s.counts == dict(eligible=int(st[2]), fresh=int(st[3]), rejected=int(st[4]), history=int(st[5]) / float(FH * FW)), (name, i)
        assert np.array_equal(s.frame, want['den']), (name, i, int((s.frame != want['den']).sum()))
        print("%s pair %d: tol %d noise %d counts %s" % (name, i, s.tol, s.noise, s.counts))
    assert got[-1].counts['history'] > 1.5                                    # the history grew: something was averaged
    # the state on the device is the mirror's history
    state = est.den_state.cpu().numpy().view(np.uint16)
    assert np.array_equal(state[:FH, :FW].astype(np.int64), hist)
    # the flows and masks are a plain estimator's, bit for bit
    plain = _estimator(name, dev, kind='plain')
    mine = plain.estimate_sequence_bidirectional(frames)
    assert len(mine) == NFRAMES - 1
    for x, y in zip(both, mine):
        assert all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8)) for p, q in zip(x, y))
    assert plain.denoise is None and plain.den_ws is None and plain.den_state is None and plain.out_den is None
    for call in (lambda: plain.push_denoised(frames[:2]), lambda: plain.denoise_sequence(frames)):
        with pytest.raises(RuntimeError, match="without denoising.*denoise=True"):
            call()
    with pytest.raises(ValueError, match="denoised frames need"):
        plain.export_sequence(frames, "unused", denoise=True)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pushes_reset_and_eager_are_bit_identical_to_the_whole_clip(name, dev):
    ref = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    g = est.graph
    assert _same_den(est.denoise_sequence(iter(frames)), ref)                 # the same clip again: reset() inside, no memset
    est.reset()
    got, n0 = [], 0
    for k in CONFIGS[name][1]:
        out = est.push_denoised(frames[n0:n0 + k])
        assert len(out) == (k if n0 else k - 1)
        got += out
        n0 += k
    assert n0 == NFRAMES and _same_den(got, ref) and est.graph is g           # one graph, never re-captured
    # without reset() the history goes on: the same frames pushed again are filtered with a longer history
    more = est.push_denoised(frames[:2])
    assert len(more) == 2 and more[1].counts['history'] > ref[0].counts['history']
    est.reset()
    assert _same_den(est.push_denoised(frames[:3]), ref[:2])                  # reset() starts a new history
    eager = _estimator(name, dev, use_graph=False)
    assert _same_den(eager.denoise_sequence(frames), ref) and eager.graph is None
    other = est.denoise_sequence(_static_clip(3, 74, CONFIGS[name][0]))
    assert len(other) == 2 and not _same_den(other, ref[:2])
    assert _same_den(est.denoise_sequence(frames), ref)                       # another clip in between leaves nothing behind
    assert not bool(est.den_ws[:BATCH * 256].any()) and not bool(eager.den_ws[:BATCH * 256].any())


def test_the_option_combines_with_track_interpolate_and_stabilise_and_changes_none(dev):
    name = 'B3-u8'
    ref = _first(name, dev)
    both, others = _estimator(name, dev, kind='all'), _estimator(name, dev, kind='others')
    frames = _frames(name)
    assert _same_den(both.denoise_sequence(frames), ref)
    a, b = both.track_sequence(frames), others.track_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(np.array_equal(x.disp.view(np.int32), y.disp.view(np.int32)) and
                                         np.array_equal(x.alive, y.alive) for x, y in zip(a, b))
    assert TG._same_mids(both.interpolate_sequence(frames), others.interpolate_sequence(frames))
    a, b = both.stabilise_sequence(frames), others.stabilise_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))
    assert others.denoise is None and others.out_den is None


# ------------------------------------------------------------------------------------------------- 5. files and the command line
def test_export_writes_the_returned_frames_through_the_three_writers(dev, tmp_path, checkpoint):  # noqa: F811
    from unflow_amd.core.inference import FlowEstimator
    _, fdir, ckpt_dir, cfg = checkpoint
    frames = _static_clip(4, 75, True)
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence='bidirectional', denoise=dict(depth=4))
    den = est.denoise_sequence(frames)
    assert len(den) == 3 and all(not np.array_equal(d.frame, f) for d, f in zip(den, frames[1:]))     # something was averaged
    names = [n % i for i in range(3) for n in ('%06d_10.png', '%06d_10_occ.png', '%06d_den.png')]
    host = est.export_sequence(frames, str(tmp_path / "host"), occlusion=True, denoise=True)
    pool = est.export_sequence(iter(frames), str(tmp_path / "pool"), occlusion=True, denoise=True, workers=2)
    dev_z = est.export_sequence(frames, str(tmp_path / "devz"), occlusion=True, denoise=True, workers=2, deflate='device')
    for paths in (host, pool, dev_z):
        assert [os.path.basename(p) for p in paths] == names
        folder = os.path.dirname(paths[0])
        for i, d in enumerate(den):
            got = TG._decoded(os.path.join(folder, '%06d_den.png' % i))
            assert got.dtype == np.uint8 and np.array_equal(got, d.frame), (folder, i)
    for a, b, c in zip(host, pool, dev_z):                                    # every file decodes to identical pixels
        assert np.array_equal(TG._decoded(a), TG._decoded(b)) and np.array_equal(TG._decoded(a), TG._decoded(c)), a
    # without denoise=True the files are the ones of an estimator without the option
    plain = est.export_sequence(frames, str(tmp_path / "plain"), occlusion=True)
    assert [os.path.basename(p) for p in plain] == [n for n in names if 'den' not in n]


def test_the_command_line_writes_the_den_files(dev, tmp_path, checkpoint):  # noqa: F811
    """python -m unflow_amd.sequence --occlusion --denoise --denoise_tol 3 --denoise_depth 4, as a child process: the files of such an
    estimator; and --denoise on a command that would build a one-direction estimator says what it needs."""
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    one = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence='bidirectional', denoise=dict(tol=3, depth=4))
    want = one.denoise_sequence(frames)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--out', str(tmp_path / "cli"),
                        '--batch', '2', '--net_size', str(H), str(W), '--config', cfg, '--occlusion', '--denoise', '--denoise_tol', '3',
                        '--denoise_depth', '4'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(out)) == sorted(n % i for i in range(3) for n in ('%06d_10.png', '%06d_10_occ.png', '%06d_den.png'))
    for i, d in enumerate(want):
        assert np.array_equal(TG._decoded(os.path.join(out, '%06d_den.png' % i)), d.frame), i
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--config', cfg, '--denoise'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and '--output_backward or --occlusion' in r.stderr
