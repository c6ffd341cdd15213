"""-m gpu: bidirectional sequence inference — the mirror kernel on the engine's own buffers, both directions of
FlowEstimator(..., sequence='bidirectional') against the fp64 oracle and against pair-mode bidirectional, the occlusion masks
against losses.occlusion, short pushes / reset / graph and eager, export and the command line, and the engine's memory."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_sequence_gpu as SG          # clip(), _bound(), _params() and the shared parameter cache of the one-direction tests

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
_ORACLE = {}


def _oracle_both(key, spec, frames, H, W):
    """oracle.model_ref.flownet(..., backward_flow=True) on every (f_i, f_i+1) in fp64 -> (fw, bw), frame-size final flows
    [T-1, h, w, 2] each (the evaluation chain of SG._oracle_flows).  Computed once per key and shared."""
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import model_ref as M
    tf64 = {k: v.double() for k, v in SG._TFP[spec].items()}
    x = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32) for f in frames]))
    h, w = x.shape[1:3]
    if (h, w) != (H, W):
        x = M.resize_bilinear_tf1(x, H, W)
    mean = torch.tensor(SG.CHANNEL_MEAN) / 255.0
    x = (x / 255.0 - mean).double()
    out = []
    with torch.no_grad():
        for flows in M.flownet(tf64, x[:-1], x[1:], spec, backward_flow=True):
            f = M.resize_bilinear_tf1(flows[-1][0], H, W) * 20
            if (h, w) != (H, W):
                f = M.resize_bilinear_tf1(f, h, w)
                f = torch.stack([f[..., 0] * (w / float(W)), f[..., 1] * (h / float(H))], 3)
            out.append(f.numpy())
    _ORACLE[key] = tuple(out)
    return _ORACLE[key]


def _estimator(spec, B, H, W, dev, **kw):
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator(dict(flownet=spec), B, net_size=(H, W), device=dev, sequence='bidirectional', **kw)
    SG._params(est, spec)
    return est


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for x, y in zip(a, b) for u, v in zip(x, y))


# ------------------------------------------------------------------------------------------------- 1. mirror kernel
def test_mirror_copies_the_conv2_segment_of_the_tower_rows_and_nothing_else(dev):
    from unflow_amd.core.engine import FlowNetEngine
    B = 2
    eng = FlowNetEngine(B, 64, 128, params=dict(flownet='C'), device=dev, seed=None, inference=True, sequence='bidirectional')
    st = eng.stages[0]
    assert eng.final_flow.shape == (2 * B, 64, 128, 2) and eng.x0.shape[0] == B + 1
    assert st.A['cat2'].t.shape[:3] == (2 * B + 1, 16, 32) and st.A['c3'].t.shape[0] == B + 1 and st.A['cat3'].t.shape[0] == 2 * B
    g = torch.Generator(device=dev).manual_seed(5)
    tensors = {'x0': eng.X0, 'c1': st.A['c1'], 'c3': st.A['c3'], 'cat2': st.A['cat2'], 'cat3': st.A['cat3'], 'catc': st.A['catc']}
    for pt in tensors.values():
        pt.t.copy_(torch.randn(pt.t.shape, generator=g, device=dev))
        if pt.pl is not None:
            pt.pl.copy_(torch.randint(-30000, 30000, pt.pl.shape, generator=g, device=dev, dtype=torch.int16))
    lo, n = st.bufs['cat2'][1]['conv2']
    assert (lo, n) == (0, 128) and tensors['cat2'].t.shape[3] > 128
    snap = lambda: {k: (pt.t.clone(), None if pt.pl is None else pt.pl.clone()) for k, pt in tensors.items()}   # noqa: E731
    before = snap()
    st.sequence_mirror()
    torch.cuda.synchronize()
    after = snap()
    for k in tensors:
        if k != 'cat2':
            assert torch.equal(after[k][0], before[k][0]) and (after[k][1] is None or torch.equal(after[k][1], before[k][1])), k
    t, pl = after['cat2']
    bt, bpl = before['cat2']
    # rows [0, B) <- rows [B + 1, 2B + 1), the conv2 channels alone; every other row as it was
    assert torch.equal(t[:B, ..., :128], bt[B + 1:, ..., :128]) and torch.equal(t[:B, ..., 128:], bt[:B, ..., 128:])
    assert torch.equal(t[B:], bt[B:]) and not torch.equal(t[:B, ..., :128], bt[:B, ..., :128])
    if pl is not None:
        assert torch.equal(pl[:, :B, ..., :128], bpl[:, B + 1:, ..., :128]) and torch.equal(pl[:, :B, ..., 128:], bpl[:, :B, ..., 128:])
        assert torch.equal(pl[:, B:], bpl[:, B:])


def test_mirror_takes_a_narrow_unaligned_segment_and_refuses_overlap(dev):
    """The C entry on its own: 3 of 5 two-byte channels in pixels 10 bytes apart (the 2-byte path) beside a 16-byte buffer, for
    n = 2 and n = 1; overlapping ranges and rows the buffers do not have return UNFLOW_ERR_SHAPE and write nothing."""
    L = SG._lib()
    a = torch.randint(-30000, 30000, (6, 37, 5), dtype=torch.int16, device=dev)
    b = torch.randn(6, 50, 8, device=dev)
    bufs = (L.CarryBuf * 2)(L.CarryBuf(a[0, 0, 1:].data_ptr(), 37, 6, 10), L.CarryBuf(b.data_ptr(), 50, 16, 32))

    def run(src0, dst0, n, max_row=5):
        st = L.lib().unflow_sequence_mirror(bufs, 2, src0, dst0, n, max_row, L.stream())
        torch.cuda.synchronize()
        return st
    for src0, dst0, n in ((3, 0, 2), (1, 5, 1), (0, 2, 2)):
        a0, b0 = a.clone(), b.clone()
        assert run(src0, dst0, n) == 0
        d, s = slice(dst0, dst0 + n), slice(src0, src0 + n)
        assert torch.equal(a[d, :, 1:4], a0[s, :, 1:4]) and torch.equal(a[d, :, 0], a0[d, :, 0]) and torch.equal(a[d, :, 4], a0[d, :, 4])
        assert torch.equal(b[d, :, :4], b0[s, :, :4]) and torch.equal(b[d, :, 4:], b0[d, :, 4:])
        keep = [r for r in range(6) if not dst0 <= r < dst0 + n]
        assert torch.equal(a[keep], a0[keep]) and torch.equal(b[keep], b0[keep])
        assert not torch.equal(a[d, :, 1:4], a0[d, :, 1:4])
    a0, b0 = a.clone(), b.clone()
    for src0, dst0, n, max_row in ((0, 1, 2, 5), (2, 1, 2, 5), (3, 3, 1, 5), (0, 4, 3, 5), (4, 0, 2, 4), (0, 2, 0, 5), (-1, 2, 1, 5)):
        assert run(src0, dst0, n, max_row) == -5, (src0, dst0, n, max_row)       # UNFLOW_ERR_SHAPE
    assert torch.equal(a, a0) and torch.equal(b, b0)


# ------------------------------------------------------------------------------------------------- 2. both directions vs the oracle
@pytest.mark.parametrize("spec,B,H,W,T", SG.ORACLE_CASES, ids=['C-B2', 'C-B3-even-F', 'CS-B1'])
def test_both_directions_vs_fp64_oracle(spec, B, H, W, T, dev):
    est = _estimator(spec, B, H, W, dev)
    frames = SG.clip(T, H, W, 32)
    got = est.estimate_sequence_bidirectional(frames)
    assert len(got) == T - 1 and all(g.flow_fw.shape == (H, W, 2) and g.flow_bw.shape == (H, W, 2) for g in got)
    assert all(g.occ_fw.shape == (H, W) and g.occ_bw.shape == (H, W) for g in got)
    fw, bw = _oracle_both((spec, H, W, T), spec, frames, H, W)
    e_fw = [SG._epe(g.flow_fw, r) for g, r in zip(got, fw)]
    e_bw = [SG._epe(g.flow_bw, r) for g, r in zip(got, bw)]
    print("bidirectional sequence %s B=%d %dx%d: EPE per pair vs fp64 oracle fw %s bw %s (bound %g)"
          % (spec, B, H, W, ["%.2e" % e for e in e_fw], ["%.2e" % e for e in e_bw], SG._bound()))
    assert max(e_fw) < SG._bound() and max(e_bw) < SG._bound(), (e_fw, e_bw)
    # neighbouring pairs, and the two directions of one pair, are pixels apart: a wrong row pairing or swapped blocks are far
    # outside the bound
    assert SG._epe(fw[0], fw[1]) > 1.0 and SG._epe(bw[0], bw[1]) > 1.0
    assert all(SG._epe(a, b) > 1.0 for a, b in zip(fw, bw))


# ------------------------------------------------------------------------------------------------- 3. against pair-mode bidirectional
def test_agrees_with_pair_mode_bidirectional_and_masks_are_the_flows_own(dev):
    from unflow_amd.core import losses
    from unflow_amd.core.inference import FlowEstimator
    B, H, W, T = 2, 64, 128, 5
    frames = SG.clip(T, 90, 151, 33, u8=True)
    seq = _estimator('C', B, H, W, dev, max_frame=(90, 151))
    pair = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=(90, 151), device=dev, bidirectional=True)
    SG._params(pair, 'C')
    a = seq.estimate_sequence_bidirectional(frames)
    b = pair.estimate_bidirectional(frames[:-1], frames[1:])
    fw, bw = _oracle_both(('C', H, W, T, 90, 151), 'C', frames, H, W)
    assert len(a) == len(b) == T - 1 and a[0].flow_bw.shape == (90, 151, 2) and a[0].occ_fw.shape == (90, 151)
    bound = SG._bound()
    for i in range(T - 1):
        for name, ref in (('flow_fw', fw[i]), ('flow_bw', bw[i])):
            x, y = getattr(a[i], name), getattr(b[i], name)
            ea, eb, ab = SG._epe(x, ref), SG._epe(y, ref), SG._epe(x, y)
            print("pair %d %s: sequence vs oracle %.2e, pair mode vs oracle %.2e, sequence vs pair mode %.2e" % (i, name, ea, eb, ab))
            assert ea < bound and eb < bound and ab < 2 * bound, (i, name, ea, eb, ab)
        # the masks are losses.occlusion of this pair's own returned flows, bit for bit
        f = torch.from_numpy(a[i].flow_fw).to(dev)[None].contiguous()
        r = torch.from_numpy(a[i].flow_bw).to(dev)[None].contiguous()
        ref_fw, ref_bw = losses.occlusion(f, r)
        torch.cuda.synchronize()
        r_fw, r_bw = ref_fw[0, ..., 0].cpu().numpy().astype(bool), ref_bw[0, ..., 0].cpu().numpy().astype(bool)
        assert a[i].occ_fw.dtype == np.bool_ and np.array_equal(a[i].occ_fw, r_fw), (i, int((a[i].occ_fw != r_fw).sum()))
        assert np.array_equal(a[i].occ_bw, r_bw), (i, int((a[i].occ_bw != r_bw).sum()))
        shares = (float(a[i].occ_fw.mean()), float(a[i].occ_bw.mean()))
        print("pair %d: occluded share fw %.3f bw %.3f" % ((i,) + shares))
        assert all(0.0 < s < 1.0 for s in shares), (i, shares)       # both outcomes on this clip
    # the methods of the other modes
    for call in (lambda: pair.push_bidirectional(frames[:1]), lambda: pair.estimate_sequence_bidirectional(frames)):
        with pytest.raises(RuntimeError, match="sequence='bidirectional'"):
            call()
    with pytest.raises(RuntimeError, match="sequence"):
        seq.estimate_bidirectional(frames[:-1], frames[1:])


# ------------------------------------------------------------------------------------------------- 4. short pushes and reset
def test_short_pushes_reset_graph_and_eager(dev):
    from unflow_amd.core.inference import FlowEstimator
    B, H, W = 3, 64, 128
    frames = SG.clip(8, H, W, 32)                         # a frame more than test 2's 64 x 128 clip: pushes of 2, 3, 1, 2
    est, eager = _estimator('C', B, H, W, dev), _estimator('C', B, H, W, dev, use_graph=False)
    whole = est.estimate_sequence_bidirectional(frames)
    assert len(whole) == 7
    for _ in range(2):                                    # the same clip again after a reset
        est.reset()
        got, n0 = [], 0
        for k, want in ((2, 1), (3, 3), (1, 1), (2, 2)):
            out = est.push_bidirectional(frames[n0:n0 + k])
            assert len(out) == want, (k, len(out))
            got += out
            n0 += k
        assert _same(got, whole)
    assert est.graph is not None
    assert eager.graph is None and _same(eager.estimate_sequence_bidirectional(iter(frames)), whole) and eager.graph is None
    # push / estimate_sequence: the forward flows alone
    est.reset()
    fwd = est.push(frames[:3]) + est.push(frames[3:4])
    assert len(fwd) == 3 and all(np.array_equal(f, w.flow_fw) for f, w in zip(fwd, whole))
    fwd = est.estimate_sequence(frames)
    assert len(fwd) == 7 and all(isinstance(f, np.ndarray) and np.array_equal(f, w.flow_fw) for f, w in zip(fwd, whole))
    one = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), device=dev, sequence=True)
    for call in (lambda: one.push_bidirectional(frames[:2]), lambda: one.estimate_sequence_bidirectional(frames)):
        with pytest.raises(RuntimeError, match="one-direction sequence estimator"):
            call()


# ------------------------------------------------------------------------------------------------- 5. export and CLI
def test_export_sequence_backward_occlusion_and_cli(dev, tmp_path):
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import decode_png, read_flo, read_kitti_flow_png, write_png_rgb8
    from unflow_amd.core.train import Trainer
    H, W = 64, 128
    frames = SG.clip(5, H, W, 50, u8=True)
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
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), device=dev, sequence='bidirectional')
    res = est.estimate_sequence_bidirectional(frames)
    assert len(res) == 4 and max(float(np.abs(r.flow_bw).max()) for r in res) > 0.05
    names = lambda ext: [n for i in range(4) for n in ('%06d_10.%s' % (i, ext), '%06d_01.%s' % (i, ext), '%06d_10_occ.png' % i)]   # noqa: E731

    def check_pngs(folder):
        for i, r in enumerate(res):
            for tag, f in (('10', r.flow_fw), ('01', r.flow_bw)):
                back, mask = read_kitti_flow_png(os.path.join(folder, '%06d_%s.png' % (i, tag)))
                q = np.clip(np.float32(f) * np.float32(64) + np.float32(32768), 0, 65535).astype(np.uint16)
                assert np.array_equal(back.numpy(), (q.astype(np.float32) - 2 ** 15) / 64.0) and (mask.numpy() == 1).all(), (i, tag)
            with open(os.path.join(folder, '%06d_10_occ.png' % i), 'rb') as fh:
                occ = np.asarray(decode_png(fh.read()))
            assert np.array_equal(occ.reshape(H, W), r.occ_fw.astype(np.uint8) * 255), i
    for sub, kw in (('host', dict(workers=0)), ('device', dict(workers=2, deflate='device'))):
        paths = est.export_sequence(iter(frames), str(tmp_path / sub), fmt='png', backward=True, occlusion=True, **kw)
        assert sorted(os.path.basename(p) for p in paths) == sorted(names('png')) and len(paths) == 12
        if not kw['workers']:
            assert [os.path.basename(p) for p in paths] == names('png')      # per pair: _10, _01, _10_occ
        check_pngs(str(tmp_path / sub))
    # only one of the two, and the flows as .flo through the pool
    paths = est.export_sequence(frames, str(tmp_path / "occ_only"), fmt='flo', workers=2, occlusion=True)
    assert sorted(os.listdir(str(tmp_path / "occ_only"))) == sorted(n for n in names('flo') if '_01' not in n) and len(paths) == 8
    # the command line, as a child process
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp_path / "log", tmp_path / "ckpts"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', str(fdir), '--out',
                        str(tmp_path / "cli"), '--flo', '--batch', '2', '--net_size', str(H), str(W), '--config', str(cfg),
                        '--output_backward', '--occlusion'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cli = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(cli)) == sorted(names('flo'))
    for i, rr in enumerate(res):
        for tag, f in (('10', rr.flow_fw), ('01', rr.flow_bw)):
            back, _ = read_flo(os.path.join(cli, '%06d_%s.flo' % (i, tag)))
            assert np.array_equal(np.asarray(back), f), (i, tag)
        with open(os.path.join(cli, '%06d_10_occ.png' % i), 'rb') as fh:
            assert np.array_equal(np.asarray(decode_png(fh.read())).reshape(H, W), rr.occ_fw.astype(np.uint8) * 255), i
    # a one-direction sequence estimator has neither file
    one = FlowEstimator(dict(flownet='C'), 2, net_size=(H, W), device=dev, sequence=True)
    for kw in (dict(backward=True), dict(occlusion=True)):
        with pytest.raises(ValueError, match="sequence='bidirectional'"):
            one.export_sequence(frames, str(tmp_path / "unused"), **kw)


# ------------------------------------------------------------------------------------------------- 6. memory
def test_engine_memory_is_below_pair_mode_bidirectional(dev):
    """Behind the tower both engines hold 2B rows; the tower holds B + 1 frame rows (cat2: 2B + 1) where the pair engine holds 2B."""
    from unflow_amd.core.engine import FlowNetEngine
    B, H, W = 4, 384, 1280
    requested = lambda: torch.cuda.memory_stats(dev)['requested_bytes.all.current']   # noqa: E731

    def built(**kw):
        import gc
        gc.collect()
        torch.cuda.synchronize()
        a, r = torch.cuda.memory_allocated(dev), requested()
        e = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=None, inference=True, **kw)
        torch.cuda.synchronize()
        return e, torch.cuda.memory_allocated(dev) - a, requested() - r
    pair, m_pair, r_pair = built(bidirectional=True)
    seq, m_seq, r_seq = built(sequence='bidirectional')
    st = pair.stages[0]
    row = lambda pt: pt.t[0].numel() * 4 + (0 if pt.pl is None else pt.pl[:, 0].numel() * 2)   # noqa: E731
    derived = (B - 1) * sum(row(pt) for pt in (pair.X0, st.A['c1'], st.A['c3'])) - row(st.A['cat2'])
    print("engine memory: bidirectional sequence %.1f MB, pair-mode bidirectional %.1f MB" % (m_seq / 1e6, m_pair / 1e6))
    print("requested bytes: sequence %d, pair mode %d, saving %d, derived %d" % (r_seq, r_pair, r_pair - r_seq, derived))
    assert seq.stages[0].A['cat2'].t.shape[0] == 2 * B + 1 and seq.stages[0].A['cat3'].t.shape[0] == 2 * B
    assert m_seq < m_pair and r_seq < r_pair and r_pair - r_seq >= derived, (m_pair, m_seq, r_pair, r_seq, derived)
