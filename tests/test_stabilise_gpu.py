"""-m gpu: camera motion along a clip — unflow_sequence_stabilise at its entry point against the numpy definition of
tests/stabilise_ref.py, word for word and pixel for pixel on all five outputs (equality: the sums and every decision are integers,
the solve is the same sequence of correctly rounded fp64 operations on both sides); what it leaves alone, and its workspace zero
again; reproducibility between launches and between graph replay and eager; the path state across launches; and
FlowEstimator(..., sequence=..., stabilise=...) against the same definition applied to the estimator's own flows and masks, beside a
plain estimator, with track and interpolate on, and through export_sequence's three writers and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stabilise_ref as R
import test_interpolate_gpu as TG       # the estimator shapes, _decoded and the checkpoint fixture of the in-between frames' tests
import test_sequence_gpu as SG          # clip(), _params() and the shared parameter cache of the sequence tests
from test_interpolate_gpu import checkpoint  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
CASES = R.entry_cases()
BY_ID = dict(CASES)
ERR_SHAPE, ERR_NULL = -5, -1
ROWS = 1                                 # sentinel rows behind every output
SENTINELS = dict(motion=-(0x5A5A5A5A5A5A5A5A), path=0x3C3C3C3C3C3C3C3C, resid=0xA5, stab=0x5A, counts=-777)
DTYPES = dict(motion=torch.int64, path=torch.int64, resid=torch.uint8, stab=torch.uint8, counts=torch.int32)


def _L():
    from unflow_amd import _lib
    return _lib


class Launch:
    """The device buffers of one case, the outputs filled with sentinels (and a row of them behind each), and the call."""

    def __init__(self, case, dev, path=None):
        L, c = _L(), case
        self.case, self.dev = case, dev
        B, Hm, Wm = c['B'], c['Hmax'], c['Wmax']
        self.frames = torch.from_numpy(c['frames']).to(dev)
        self.tab = torch.from_numpy(c['tab']).to(dev)
        self.flow_fw = torch.from_numpy(c['flow_fw']).to(dev)
        self.occ = None if c['occ'] is None else torch.from_numpy(c['occ']).to(dev)
        self.path = torch.from_numpy(np.asarray(c['path'], np.int64).copy()).to(dev) if path is None else path
        nbytes = int(L.lib().unflow_sequence_stabilise_workspace_bytes(B))
        assert nbytes > 0 and nbytes % 8 == 0
        self.ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
        shapes = dict(motion=(B + ROWS, 8), path=(B + ROWS, 8), resid=(B + ROWS, Hm, Wm), stab=(B + ROWS, Hm, Wm, 3),
                      counts=(B + ROWS, 4))
        self.out = {k: torch.full(shapes[k], SENTINELS[k], dtype=DTYPES[k], device=dev) for k in R.OUTPUTS}

    def call(self, **kw):
        L, c = _L(), self.case
        a = dict(frames=self.frames, tab=self.tab, B=c['B'], Hmax=c['Hmax'], Wmax=c['Wmax'], flow=self.flow_fw, occ=self.occ,
                 tol=c['tol'], iters=c['iters'], follow=c['follow'], state=self.path, ws=self.ws,
                 **{'out_' + k: v for k, v in self.out.items()})
        a.update(kw)
        return L.lib().unflow_sequence_stabilise(L.ptr(a['frames']), L.ptr(a['tab']), a['B'], a['Hmax'], a['Wmax'], L.ptr(a['flow']),
                                                 L.ptr(a['occ']), a['tol'], a['iters'], a['follow'], L.ptr(a['state']), L.ptr(a['ws']),
                                                 L.ptr(a['out_motion']), L.ptr(a['out_path']), L.ptr(a['out_resid']),
                                                 L.ptr(a['out_stab']), L.ptr(a['out_counts']), L.stream())

    def run(self, **kw):
        st = self.call(**kw)
        torch.cuda.synchronize()
        return st

    def outputs(self):
        """{name: the output on the host, sentinel rows included}; the workspace is all zero."""
        assert not bool(self.ws.any()), "the workspace is not zero after the launch"
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def fill(self):
        for k, v in self.out.items():
            v.fill_(SENTINELS[k])

    def untouched(self):
        return all(bool((v == SENTINELS[k]).all()) for k, v in self.out.items())


def _same(a, b):
    return len(a) == len(b) and all(all(np.array_equal(x[k], y[k]) for k in R.OUTPUTS) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_kernel_equals_the_mirror_on_all_five_outputs(cid, dev):
    """Every case of stabilise_ref.entry_cases.  out_motion, out_path, out_resid, out_stab and out_counts equal the mirror on every
    valid slot; slots that are no pairs, pixels outside (h, w) and the rows behind the buffers keep their sentinels; the path state
    equals the mirror's (untouched without a pair); the workspace is zero again."""
    case = BY_ID[cid]
    outs, new_path, _ = R.mirror_of(cid)
    run = Launch(case, dev)
    assert run.run() == 0
    seen = R.compare(case, outs, run.outputs(), SENTINELS)
    assert np.array_equal(run.path.cpu().numpy(), new_path), (run.path.cpu().numpy(), new_path)
    print("%s: %d pixels equal, motion %s" % (cid, seen, {i: o['motion'].tolist() for i, o in outs.items()}))
    assert seen > 0 or not case['valid']


def test_bad_arguments_write_nothing(dev):
    case = BY_ID['odd-u8-fw-affine-full-k0R0s0']
    run = Launch(case, dev)
    before = run.path.clone()
    for kw in (dict(B=0), dict(B=-3), dict(Hmax=0), dict(Wmax=-1), dict(Hmax=4097), dict(Wmax=4097), dict(Hmax=65536, Wmax=32768),
               dict(tol=-1), dict(tol=5), dict(iters=-1), dict(iters=5), dict(follow=-1), dict(follow=9), dict(tol=1 << 20)):
        assert run.run(**kw) == ERR_SHAPE, kw
    for name in ('frames', 'tab', 'flow', 'state', 'ws', 'out_motion', 'out_path', 'out_resid', 'out_stab', 'out_counts'):
        assert run.run(**{name: None}) == ERR_NULL, name
    assert run.untouched() and torch.equal(run.path, before) and not bool(run.ws.any())
    L = _L().lib()
    assert int(L.unflow_sequence_stabilise_workspace_bytes(0)) == 0
    # a pair slot whose frame exceeds the buffers is no pair; the path goes on through the others
    tab = case['tab'].copy()
    tab[8 * case['B'] + 8 + 1] = case['Wmax'] + 1
    odd = dict(case, tab=tab, valid=[0, 2])
    got = Launch(odd, dev)
    assert got.run() == 0
    outs, new_path, _ = R.replay(odd, odd['path'])
    R.compare(odd, outs, got.outputs(), SENTINELS)
    assert np.array_equal(got.path.cpu().numpy(), new_path)
    assert run.run() == 0 and not run.untouched()


# ------------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_graph_replay_give_identical_bytes(dev):
    """i.i.d. +-12 px at k = 4, R = 3: every weight occurs and the atomics arrive in another order every time; the
    integer sums do not care.  A second launch on the same buffers (the workspace left zero by the first, the path put back) and a
    captured graph replayed twice all give the eager launch's bytes."""
    case = next(c for _, c in CASES if c['kind'] == 'iid12' and c['tol'] == 4 and c['iters'] == 3)
    path = torch.from_numpy(case['path'].copy()).to(dev)
    eager = Launch(case, dev)
    assert eager.run() == 0
    first = eager.outputs()
    left = eager.path.clone()
    eager.fill()
    eager.path.copy_(path)
    assert eager.run() == 0
    again = eager.outputs()
    assert all(first[k].tobytes() == again[k].tobytes() for k in R.OUTPUTS) and torch.equal(eager.path, left)
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
        cap.path.copy_(path)
        g.replay()
        torch.cuda.synchronize()
        got = cap.outputs()
        assert all(first[k].tobytes() == got[k].tobytes() for k in R.OUTPUTS) and torch.equal(cap.path, left)
    R.compare(case, R.mirror_of(case['id'])[0], got, SENTINELS)


# ------------------------------------------------------------------------------------------------- 3. the path across launches
@pytest.mark.parametrize("u8,bidir,follow", [(True, False, 0), (False, True, 3)], ids=['u8-fw-lock', 'f32-bidir-follow3'])
def test_a_clip_pushed_in_replays_of_different_lengths(u8, bidir, follow, dev):
    """Nine frames through B = 3 slots in pushes of 2, 3, 1, 1, 2: the path lives in ONE device buffer from launch to launch
    (poisoned before the first) — every pair's outputs equal the mirror's on the same flows, and equal those of the same clip
    pushed three at a time."""
    from unflow_amd.core.inference import sequence_tables
    shape = R.SHAPES['odd']
    B, Hm, Wm, h, w, T = shape['B'], shape['Hmax'], shape['Wmax'], shape['h'], shape['w'], 9
    rs = R.WP._rs('stabilise-clip', u8, bidir)
    clip = R.M.draw_frames(rs, T - 1, Hm, Wm, h, w, u8)
    fw = R.draw_flows(rs, T - 1, Hm, Wm, h, w, 'smooth')
    occ = R.T.draw_occ(rs, T - 1, Hm, Wm, h, w) if bidir else None

    def pushed(pushes):
        got, mirror, carry, n0 = [], [], 0, 0
        dev_path = torch.full((8,), -(1 << 62) + 99, dtype=torch.int64, device=dev)
        host_path = dev_path.cpu().numpy()
        for k in pushes:
            tab, valid, nxt = sequence_tables((h, w), k, B, carry, u8=u8)
            fr = np.full((B, Hm, Wm, 3), 77, clip.dtype)             # slots beyond the new frames: stale bytes
            fr[:k] = clip[n0:n0 + k]
            idx = [min(max(n0 - 1 + i, 0), T - 2) for i in range(B)]        # pair slot i = pair n0 - 1 + i of the clip
            case = dict(B=B, Hmax=Hm, Wmax=Wm, h=h, w=w, u8=u8, k=k, carry=carry, tab=tab, valid=valid, frames=fr,
                        flow_fw=np.ascontiguousarray(fw[idx]), occ=None if occ is None else np.ascontiguousarray(occ[idx]),
                        tol=2, iters=3, follow=follow, path=host_path)
            run = Launch(case, dev, path=dev_path)
            assert run.run() == 0
            outs, host_path, _ = R.replay(case, host_path)
            R.compare(case, outs, run.outputs(), SENTINELS)
            assert np.array_equal(dev_path.cpu().numpy(), host_path)
            got += [{name: (v[i, :h, :w] if name in ('resid', 'stab') else v[i]).copy() for name, v in run.outputs().items()}
                    for i in valid]
            mirror += [outs[i] for i in valid]
            carry, n0 = nxt, n0 + k
        assert n0 == T and len(got) == T - 1
        return got, mirror
    ragged, mirror = pushed((2, 3, 1, 1, 2))
    assert _same(ragged, mirror)
    whole, _ = pushed((3, 3, 3))
    assert _same(ragged, whole)
    assert all(int(g['motion'][6]) >> 8 == 4 for g in whole)        # every pair was fitted, four iterations each


def test_a_poisoned_path_with_carry_source_zero_reaches_nothing(dev):
    """A clip's first replay: the state holds the sentinel of another clip (or of no clip); the outputs are those of the identity."""
    case = next(c for _, c in CASES if c['pattern'] == 'first' and c['bidir'])
    assert case['carry'] == 0 and case['valid'] == [1, 2] and int(case['path'][0]) < -(1 << 61)
    a, b = Launch(case, dev), Launch(case, dev, path=torch.full((8,), (1 << 62) + 7, dtype=torch.int64, device=dev))
    assert a.run() == 0 and b.run() == 0
    x, y = a.outputs(), b.outputs()
    assert all(x[k].tobytes() == y[k].tobytes() for k in R.OUTPUTS) and torch.equal(a.path, b.path)
    R.compare(case, R.mirror_of(case['id'])[0], y, SENTINELS)


# ------------------------------------------------------------------------------------------------- 4. the estimator
H, W, FH, FW, NFRAMES, MAXF = TG.H, TG.W, TG.FH, TG.FW, TG.NFRAMES, TG.MAXF
CONFIGS = {                             # sequence, batch, uint8 frames, the pushes of the short-push run (5 frames), the option
    'fw-B2-u8': (True, 2, True, (2, 1, 2), True),
    'bi-B2-f32': ('bidirectional', 2, False, (1, 2, 2), dict(tol=3, iters=2, follow=3)),
}
_EST, _FIRST = {}, {}


def _frames(name):
    return SG.clip(NFRAMES, FH, FW, 71, u8=CONFIGS[name][2])


def _estimator(name, dev, use_graph=True, kind='stab'):
    """The estimator of a configuration, built once.  kind: 'stab'; 'plain' (no option); 'all' (stabilise, track and interpolate);
    'others' (track and interpolate alone)."""
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, kind)
    if key not in _EST:
        seq, B, _, _, opt = CONFIGS[name]
        others = dict(track=4, interpolate=1)
        opts = dict(plain={}, stab=dict(stabilise=opt), all=dict(stabilise=opt, **others), others=others)[kind]
        est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=MAXF, device=dev, sequence=seq, use_graph=use_graph, **opts)
        tfp = SG._params(est, 'C')
        if seq == 'bidirectional':      # flow heads at a tenth leave both occluded and visible pixels (tests/test_track_gpu.py)
            est.load_tf_params({k: (v * TG.HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                                for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _first(name, dev):
    """stabilise_sequence of the whole clip as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, 'stab') not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None
        _FIRST[name] = est.stabilise_sequence(_frames(name))
        assert est.graph is not None
    return _FIRST[name]


def _same_stab(a, b):
    return len(a) == len(b) and all(all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_estimator_is_the_mirror_on_its_own_flows(name, dev):
    from unflow_amd.core.inference import STABILISE_DEFAULTS, Stabilised
    seq, B, u8, _, opt = CONFIGS[name]
    o = dict(STABILISE_DEFAULTS, **(opt if isinstance(opt, dict) else {}))
    got = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    assert len(got) == NFRAMES - 1 and all(isinstance(s, Stabilised) for s in got) and est.stabilise == o
    if seq == 'bidirectional':
        both = [(b.flow_fw, b.occ_fw) for b in est.estimate_sequence_bidirectional(frames)]
        assert any(0.02 < occ.mean() < 0.98 for _, occ in both)               # occluded and eligible pixels both occur
    else:
        both = [(f, None) for f in est.estimate_sequence(frames)]
    D = list(R.IDENTITY)
    for i, (s, (fw, occ)) in enumerate(zip(got, both)):
        frame = np.ascontiguousarray(frames[i + 1] if u8 else np.asarray(frames[i + 1], np.float32))
        want, _ = R.stabilise_pair(frame, fw, None if occ is None else occ.astype(np.uint8), FH, FW, o['tol'], o['iters'], o['follow'], D)
        D = want['path'][:6].tolist()
        assert s.frame.shape == (FH, FW, 3) and s.frame.dtype == np.uint8 and s.residual.shape == (FH, FW)
        assert np.array_equal(s.motion, want['motion']), (name, i, s.motion, want['motion'])
        assert np.array_equal(s.path, want['path']), (name, i, s.path, want['path'])
        assert np.array_equal(s.counts, want['counts']), (name, i, s.counts, want['counts'])
        assert np.array_equal(s.residual, want['resid']) and np.array_equal(s.frame, want['stab']), (name, i)
        print("%s pair %d: motion %s counts %s" % (name, i, s.motion.tolist(), s.counts.tolist()))
    assert any(int(s.motion[6]) >> 8 for s in got)                            # a fit succeeded
    # the flows are a plain estimator's, bit for bit
    plain = _estimator(name, dev, kind='plain')
    a, b = est.estimate_sequence(frames), plain.estimate_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    assert plain.stabilise is None and plain.stab_ws is None and plain.stab_path is None and plain.out_stab is None
    for call in (lambda: plain.push_stabilised(frames[:2]), lambda: plain.stabilise_sequence(frames)):
        with pytest.raises(RuntimeError, match="without camera motion.*stabilise=True"):
            call()
    with pytest.raises(ValueError, match="stabilised frames need"):
        plain.export_sequence(frames, "unused", stabilise=True)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pushes_reset_and_eager_are_bit_identical_to_the_whole_clip(name, dev):
    ref = _first(name, dev)
    est = _estimator(name, dev)
    frames = _frames(name)
    g = est.graph
    assert _same_stab(est.stabilise_sequence(iter(frames)), ref)              # the same clip again: reset() inside, no memset
    est.reset()
    got, n0 = [], 0
    for k in CONFIGS[name][3]:
        out = est.push_stabilised(frames[n0:n0 + k])
        assert len(out) == (k if n0 else k - 1)
        got += out
        n0 += k
    assert n0 == NFRAMES and _same_stab(got, ref) and est.graph is g          # one graph, never re-captured
    eager = _estimator(name, dev, use_graph=False)
    assert _same_stab(eager.stabilise_sequence(frames), ref) and eager.graph is None
    other = est.stabilise_sequence(SG.clip(3, FH, FW, 72, u8=CONFIGS[name][2]))
    assert len(other) == 2 and not _same_stab(other, ref[:2])
    assert _same_stab(est.stabilise_sequence(frames), ref)                    # another clip in between leaves nothing behind
    assert not bool(est.stab_ws.any()) and not bool(eager.stab_ws.any())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_option_combines_with_track_and_interpolate_and_changes_neither(name, dev):
    ref = _first(name, dev)
    both, others = _estimator(name, dev, kind='all'), _estimator(name, dev, kind='others')
    frames = _frames(name)
    assert _same_stab(both.stabilise_sequence(frames), ref)
    a, b = both.track_sequence(frames), others.track_sequence(frames)
    assert len(a) == NFRAMES - 1 and all(np.array_equal(x.disp.view(np.int32), y.disp.view(np.int32)) and
                                         np.array_equal(x.alive, y.alive) for x, y in zip(a, b))
    assert TG._same_mids(both.interpolate_sequence(frames), others.interpolate_sequence(frames))
    assert others.stabilise is None and others.out_stab is None


# ------------------------------------------------------------------------------------------------- 5. files and the command line
def test_export_writes_the_returned_frames_through_the_three_writers(dev, tmp_path, checkpoint):  # noqa: F811
    from unflow_amd.core.inference import FlowEstimator, camera_matrix
    frames, fdir, ckpt_dir, cfg = checkpoint
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence='bidirectional', stabilise=dict(follow=2))
    stab = est.stabilise_sequence(frames)
    assert len(stab) == 3 and any(s.residual.any() for s in stab)
    names = [n % i for i in range(3) for n in ('%06d_10.png', '%06d_10_occ.png', '%06d_stab.png', '%06d_motion.png')] + ['camera.npz']
    host = est.export_sequence(frames, str(tmp_path / "host"), occlusion=True, stabilise=True)
    pool = est.export_sequence(iter(frames), str(tmp_path / "pool"), occlusion=True, stabilise=True, workers=2)
    dev_z = est.export_sequence(frames, str(tmp_path / "devz"), occlusion=True, stabilise=True, workers=2, deflate='device')
    for paths in (host, pool, dev_z):
        assert [os.path.basename(p) for p in paths] == names
        folder = os.path.dirname(paths[0])
        for i, s in enumerate(stab):
            got = TG._decoded(os.path.join(folder, '%06d_stab.png' % i))
            assert got.dtype == np.uint8 and np.array_equal(got, s.frame), (folder, i)
            got = TG._decoded(os.path.join(folder, '%06d_motion.png' % i))
            assert got.dtype == np.uint8 and np.array_equal(got.reshape(FH, FW), s.residual), (folder, i)
        cam = np.load(paths[-1])
        assert sorted(cam.files) == ['counts', 'matrix', 'motion', 'path']
        assert np.array_equal(cam['motion'], np.stack([s.motion for s in stab])) and cam['motion'].dtype == np.int64
        assert np.array_equal(cam['path'], np.stack([s.path for s in stab]))
        assert np.array_equal(cam['counts'], np.stack([s.counts for s in stab]))
        assert np.array_equal(cam['matrix'], np.stack([camera_matrix(s.motion, FH, FW) for s in stab]))
    for a, b, c in zip(host[:-1], pool[:-1], dev_z[:-1]):                     # every file decodes to identical pixels
        assert np.array_equal(TG._decoded(a), TG._decoded(b)) and np.array_equal(TG._decoded(a), TG._decoded(c)), a
    # without stabilise=True the files are the ones of an estimator without the option
    plain = est.export_sequence(frames, str(tmp_path / "plain"), occlusion=True)
    assert [os.path.basename(p) for p in plain] == [n for n in names if 'stab' not in n and 'motion' not in n and 'camera' not in n]


def test_the_command_line_writes_the_same_files(dev, tmp_path, checkpoint):  # noqa: F811
    """python -m unflow_amd.sequence --stabilise --stabilise_tol 3 --stabilise_follow 1, as a child process, one direction: the
    files of such an estimator."""
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    one = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence=True, stabilise=dict(tol=3, follow=1))
    want = one.stabilise_sequence(frames)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--out', str(tmp_path / "cli"),
                        '--batch', '2', '--net_size', str(H), str(W), '--config', cfg, '--stabilise', '--stabilise_tol', '3',
                        '--stabilise_follow', '1'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(out)) == sorted([n % i for i in range(3) for n in ('%06d_10.png', '%06d_stab.png', '%06d_motion.png')] +
                                             ['camera.npz'])
    for i, s in enumerate(want):
        assert np.array_equal(TG._decoded(os.path.join(out, '%06d_stab.png' % i)), s.frame), i
        assert np.array_equal(TG._decoded(os.path.join(out, '%06d_motion.png' % i)).reshape(FH, FW), s.residual), i
    assert np.array_equal(np.load(os.path.join(out, 'camera.npz'))['path'], np.stack([s.path for s in want]))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--config', cfg,
                        '--stabilise', '--stabilise_iters', '5'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and '0..4' in r.stderr


def test_slot_zero_without_a_carried_frame_is_no_pair(dev):
    """Slot 0 marked a pair in the table while the carry source is 0 (a table no estimator writes): it is no pair, as for the
    in-between frames, and the outputs are the first replay's."""
    case = next(c for _, c in CASES if c['pattern'] == 'first' and not c['bidir'])
    B = case['B']
    tab = case['tab'].copy()
    tab[8 * B:8 * B + 8] = tab[8 * B + 8:8 * B + 16]
    run = Launch(dict(case, tab=tab), dev)
    assert run.run() == 0
    R.compare(case, R.mirror_of(case['id'])[0], run.outputs(), SENTINELS)
