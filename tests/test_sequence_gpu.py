"""-m gpu: sequence inference — the frames input kernel against the pair input kernel, the carry kernel on the engine's own
buffers, FlowEstimator(..., sequence=True) against the fp64 oracle and against pair mode, reproducibility across reset() and
graph / eager, short pushes, export and the command line, and the engine's memory."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNEL_MEAN = [104.920005, 110.1753, 114.785955]


def _lib():
    from unflow_amd import _lib as L
    return L


def _bound():
    """The pair-mode bound of tests/test_inference_gpu.py::test_inference_engine_flows_vs_fp64_oracle."""
    from unflow_amd.core.engine import conv_math_mode
    return 5e-2 if conv_math_mode() == 'f16' else 1e-3


def clip(T, h, w, seed, u8=False):
    """parity_util.images along a clip: every frame is the one before shifted, attenuated, plus noise."""
    g = torch.Generator().manual_seed(seed)
    fr = [torch.rand(h, w, 3, generator=g) * 255]
    for _ in range(T - 1):
        fr.append(torch.roll(fr[-1], shifts=(2, -3), dims=(0, 1)) * 0.9 + torch.rand(h, w, 3, generator=g) * 25)
    fr = [f.numpy() for f in fr]
    return [np.clip(np.rint(f), 0, 255).astype(np.uint8) for f in fr] if u8 else fr


_TFP, _ORACLE = {}, {}


def _params(est, spec):
    """The parameters of test_inference_engine_flows_vs_fp64_oracle (seed 31, stacked flow heads * 0.3), loaded into est."""
    if spec not in _TFP:
        tfp = est.engine.init_params(seed=31)
        if len(spec) > 1:
            tfp = {k: (v * 0.3 if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v) for k, v in tfp.items()}
        _TFP[spec] = {k: v.cpu() for k, v in tfp.items()}
    est.load_tf_params(_TFP[spec])
    return _TFP[spec]


def _oracle_flows(key, spec, frames, H, W):
    """oracle.model_ref.flownet(..., backward_flow=False) on every (f_i, f_i+1) in fp64, as frame-size final flows [T-1,h,w,2]:
    frames of another size than the network's go through the evaluation chain (resize in, resize out, per-axis rescale).
    Computed once per key and shared."""
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import model_ref as M
    tf64 = {k: v.double() for k, v in _TFP[spec].items()}
    x = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32) for f in frames]))
    h, w = x.shape[1:3]
    if (h, w) != (H, W):
        x = M.resize_bilinear_tf1(x, H, W)
    mean = torch.tensor(CHANNEL_MEAN) / 255.0
    x = (x / 255.0 - mean).double()
    with torch.no_grad():
        ref = M.flownet(tf64, x[:-1], x[1:], spec, backward_flow=False)
        f = M.resize_bilinear_tf1(ref[-1][0], H, W) * 20
        if (h, w) != (H, W):
            f = M.resize_bilinear_tf1(f, h, w)
            f = torch.stack([f[..., 0] * (w / float(W)), f[..., 1] * (h / float(H))], 3)
    _ORACLE[key] = f.numpy()
    return _ORACLE[key]


def _epe(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).sum(-1)).mean())


# ------------------------------------------------------------------------------------------------- 1. input kernel
@pytest.mark.parametrize("u8", [False, True], ids=['fp32', 'uint8'])
def test_input_frames_kernel_equals_the_pair_input_kernel(u8, dev):
    from unflow_amd.core.inference import pack_desc
    L = _lib()
    B, Hm, Wm, H, W = 3, 96, 160, 64, 128
    sizes = [(96, 160), (90, 151)]
    rs = np.random.RandomState(7)
    dt = np.uint8 if u8 else np.float32
    staged = np.zeros((2, B, Hm, Wm, 3), dt)
    for i, (h, w) in enumerate(sizes):
        fr = rs.randint(0, 256, size=(h, w, 3)).astype(np.float32)
        if not u8:
            fr += rs.rand(h, w, 3).astype(np.float32) * 0.5
        staged[0, i, :h, :w] = fr.astype(dt)
    staged[0, 2] = rs.randint(0, 256, size=(Hm, Wm, 3)).astype(dt)          # the h = 0 slot: its bytes must not be read
    desc = torch.from_numpy(pack_desc(sizes, B, u8=u8)).to(dev)
    frames = torch.from_numpy(staged).to(dev)
    mean = (L.ctypes.c_float * 3)(*CHANNEL_MEAN)
    # the pair kernel's rows [0, B): frame 0 of every sample
    ref = torch.full((2 * B, H, W, 4), 7.0, device=dev)
    ref_pl = torch.full((3, 2 * B, H, W, 4), 0x1234, dtype=torch.int16, device=dev)
    L.check(L.lib().unflow_inference_input(L.ptr(frames), L.ptr(desc), B, Hm, Wm, H, W, L.ptr(ref), mean, L.planes_of(ref_pl),
                                           L.stream()), "inference_input")
    # rows [1, 4) of a 4-row input; a fifth row stands for the bytes behind it
    x0 = torch.full((5, H, W, 4), 7.0, device=dev)
    pl = torch.full((3, 5, H, W, 4), 0x1234, dtype=torch.int16, device=dev)
    L.check(L.lib().unflow_inference_input_frames(L.ptr(frames[0]), L.ptr(desc), B, Hm, Wm, H, W, L.ptr(x0[1:]), mean,
                                                  L.planes_of(pl[:, 1:]), L.stream()), "inference_input_frames")
    torch.cuda.synchronize()
    assert torch.equal(x0[1:4], ref[:B]) and torch.equal(pl[:, 1:4], ref_pl[:, :B])
    assert ref[0].abs().max().item() > 0.1 and (ref[2] == 0).all() and (x0[3] == 0).all() and (pl[:, 3] == 0).all()
    for r in (0, 4):                                                         # row 0 and what lies behind row 3: untouched
        assert (x0[r] == 7.0).all() and (pl[:, r] == 0x1234).all()


# ------------------------------------------------------------------------------------------------- 2. carry
def _carry_engine(dev):
    from unflow_amd.core.engine import FlowNetEngine
    eng = FlowNetEngine(2, 64, 128, params=dict(flownet='C'), device=dev, seed=None, inference=True, sequence=True)
    st = eng.stages[0]
    g = torch.Generator(device=dev).manual_seed(3)
    tensors = {'x0': eng.X0, 'c1': st.A['c1'], 'c3': st.A['c3'], 'cat2': st.A['cat2'], 'cat3': st.A['cat3']}
    for pt in tensors.values():
        pt.t.copy_(torch.randn(pt.t.shape, generator=g, device=dev))
        if pt.pl is not None:
            pt.pl.copy_(torch.randint(-30000, 30000, pt.pl.shape, generator=g, device=dev, dtype=torch.int16))
    return eng, tensors


def test_carry_moves_one_row_of_the_listed_buffers_and_nothing_else(dev):
    eng, tensors = _carry_engine(dev)
    assert eng.x0.shape == (3, 64, 128, 4) and tensors['c3'].t.shape == (3, 8, 16, 256) and tensors['cat2'].t.shape[:3] == (3, 16, 32)
    lo, n = eng.stages[0].bufs['cat2'][1]['conv2']
    assert (lo, n) == (0, 128) and tensors['cat2'].t.shape[3] > 128
    snap = lambda: {k: (pt.t.clone(), None if pt.pl is None else pt.pl.clone()) for k, pt in tensors.items()}   # noqa: E731
    src = torch.zeros(4, dtype=torch.int32, device=dev)

    def run(s):
        src[0] = s
        eng.sequence_carry(src)
        torch.cuda.synchronize()
    before = snap()
    run(0)                                                                   # nothing to carry: nothing changes
    for k, (t, pl) in snap().items():
        assert torch.equal(t, before[k][0]) and (pl is None or torch.equal(pl, before[k][1])), k
    for s in (2, 1):
        before = snap()
        run(s)
        after = snap()
        for k in ('x0', 'c3'):                                               # the whole row, planes of c3 included
            t, pl = after[k]
            assert torch.equal(t[0], before[k][0][s]) and torch.equal(t[1:], before[k][0][1:]), (k, s)
            if k == 'c3' and pl is not None:
                assert torch.equal(pl[:, 0], before[k][1][:, s]) and torch.equal(pl[:, 1:], before[k][1][:, 1:]), (k, s)
        assert not torch.equal(after['c3'][0][0], before['c3'][0][0])
        t, pl = after['cat2']                                                # the conv2 segment alone
        bt, bpl = before['cat2']
        assert torch.equal(t[0, ..., :128], bt[s, ..., :128]) and torch.equal(t[0, ..., 128:], bt[0, ..., 128:])
        assert torch.equal(t[1:], bt[1:])
        if pl is not None:
            assert torch.equal(pl[:, 0, ..., :128], bpl[:, s, ..., :128]) and torch.equal(pl[:, 0, ..., 128:], bpl[:, 0, ..., 128:])
            assert torch.equal(pl[:, 1:], bpl[:, 1:])
        for k in ('c1', 'cat3'):                                             # not in the list
            assert torch.equal(after[k][0], before[k][0]) and (after[k][1] is None or torch.equal(after[k][1], before[k][1]))
        if eng.X0.pl is not None:
            assert torch.equal(after['x0'][1], before['x0'][1])              # conv1 reads the planes of rows [1, F) only
    run(3)                                                                   # a row the buffers do not have: a no-op
    before = after
    for k, (t, pl) in snap().items():
        assert torch.equal(t, before[k][0]) and (pl is None or torch.equal(pl, before[k][1])), k


def test_carry_takes_a_narrow_unaligned_segment(dev):
    """The C entry on its own: a 2-byte-aligned segment of 6 bytes in pixels 10 bytes apart (the 2-byte path), beside a
    16-byte one, in one launch."""
    L = _lib()
    a = torch.randint(-30000, 30000, (3, 37, 5), dtype=torch.int16, device=dev)
    b = torch.randn(3, 50, 8, device=dev)
    a0, b0 = a.clone(), b.clone()
    bufs = (L.CarryBuf * 2)(L.CarryBuf(a[0, 0, 1:].data_ptr(), 37, 6, 10), L.CarryBuf(b.data_ptr(), 50, 16, 32))
    src = torch.tensor([2], dtype=torch.int32, device=dev)
    L.check(L.lib().unflow_sequence_carry(bufs, 2, L.ptr(src), 2, L.stream()), "sequence_carry")
    torch.cuda.synchronize()
    assert torch.equal(a[0, :, 1:4], a0[2, :, 1:4]) and torch.equal(a[0, :, 0], a0[0, :, 0]) and torch.equal(a[0, :, 4], a0[0, :, 4])
    assert torch.equal(a[1:], a0[1:])
    assert torch.equal(b[0, :, :4], b0[2, :, :4]) and torch.equal(b[0, :, 4:], b0[0, :, 4:]) and torch.equal(b[1:], b0[1:])


# ------------------------------------------------------------------------------------------------- 3. flows vs the oracle
ORACLE_CASES = [('C', 2, 128, 192, 5), ('C', 3, 64, 128, 7), ('CS', 1, 64, 128, 4)]


@pytest.mark.parametrize("spec,B,H,W,T", ORACLE_CASES, ids=['C-B2', 'C-B3-even-F', 'CS-B1'])
def test_sequence_flows_vs_fp64_oracle(spec, B, H, W, T, dev):
    from unflow_amd.core.inference import FlowEstimator
    est = FlowEstimator(dict(flownet=spec), B, net_size=(H, W), device=dev, sequence=True)
    _params(est, spec)
    frames = clip(T, H, W, 32)
    flows = est.estimate_sequence(frames)
    assert len(flows) == T - 1 and all(f.shape == (H, W, 2) for f in flows)
    ref = _oracle_flows((spec, H, W, T), spec, frames, H, W)
    epes = [_epe(f, r) for f, r in zip(flows, ref)]
    print("sequence %s B=%d %dx%d: EPE per pair vs fp64 oracle %s (bound %g)" % (spec, B, H, W, ["%.2e" % e for e in epes], _bound()))
    assert max(epes) < _bound(), epes
    # the flows of neighbouring pairs are pixels apart: a pair given the wrong first frame is far outside the bound
    assert _epe(ref[0], ref[1]) > 1.0


def test_engine_set_frames_eager(dev):
    """The engine on its own, without estimator or graph: set_frames carries row `carry` and fills rows [1, k + 1)."""
    from unflow_amd.core.engine import FlowNetEngine
    B, H, W = 2, 64, 128
    frames = clip(7, H, W, 32)                            # test 3's 64 x 128 clip and its oracle flows
    eng = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=None, inference=True, sequence=True)
    if 'C' not in _TFP:
        _TFP['C'] = {k: v.cpu() for k, v in eng.init_params(seed=31).items()}
    eng.load_tf_params(_TFP['C'])
    ref = _oracle_flows(('C', H, W, 7), 'C', frames, H, W)
    with pytest.raises(RuntimeError, match="set_frames"):
        eng.set_input(torch.zeros(B, H, W, 3), torch.zeros(B, H, W, 3))
    with pytest.raises(ValueError):
        eng.set_frames(np.stack(frames[:3]))
    eng.set_frames(np.stack(frames[0:2]))                 # rows 1, 2 = f0, f1: pair slot 1 = (f0, f1)
    eng.forward_net()
    fw, bw = eng.final_flows()
    assert bw is None and fw.shape == (B, H, W, 2)
    assert _epe(fw[1].cpu().numpy(), ref[0]) < _bound()
    eng.set_frames(np.stack(frames[2:3]), carry=2)        # a short one: row 0 = f1, row 1 = f2
    eng.forward_net()
    fw, _ = eng.final_flows()
    assert _epe(fw[0].cpu().numpy(), ref[1]) < _bound()
    eng.set_frames(np.stack(frames[3:5]), carry=1)        # row 0 = f2, rows 1, 2 = f3, f4
    eng.forward_net()
    fw, _ = eng.final_flows()
    torch.cuda.synchronize()
    assert _epe(fw[0].cpu().numpy(), ref[2]) < _bound() and _epe(fw[1].cpu().numpy(), ref[3]) < _bound()


# ------------------------------------------------------------------------------------------------- 4. against pair mode
def test_sequence_agrees_with_pair_mode(dev):
    from unflow_amd.core.inference import FlowEstimator
    B, H, W, T = 2, 64, 128, 5
    frames = clip(T, 90, 151, 33, u8=True)
    seq = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=(90, 151), device=dev, sequence=True)
    pair = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=(90, 151), device=dev)
    _params(seq, 'C')
    _params(pair, 'C')
    a = seq.estimate_sequence(frames)
    b = pair.estimate(frames[:-1], frames[1:])
    ref = _oracle_flows(('C', H, W, T, 90, 151), 'C', frames, H, W)
    assert len(a) == len(b) == T - 1 and a[0].shape == (90, 151, 2)
    for i in range(T - 1):
        ea, eb, ab = _epe(a[i], ref[i]), _epe(b[i], ref[i]), _epe(a[i], b[i])
        print("pair %d: sequence vs oracle %.2e, pair mode vs oracle %.2e, sequence vs pair mode %.2e" % (i, ea, eb, ab))
        assert ea < _bound() and eb < _bound() and ab < 2 * _bound(), (i, ea, eb, ab)
    with pytest.raises(RuntimeError, match="sequence"):
        seq.estimate(frames[:-1], frames[1:])
    with pytest.raises(RuntimeError, match="sequence"):
        seq.export(iter(()), "unused")
    for call in (lambda: pair.push(frames[:1]), lambda: pair.reset(), lambda: pair.estimate_sequence(frames),
                 lambda: pair.export_sequence(frames, "unused")):
        with pytest.raises(RuntimeError, match="sequence=True"):
            call()


# ------------------------------------------------------------------------------------------------- 5. reproducibility
def test_sequence_is_reproducible_across_reset_and_graph(dev):
    from unflow_amd.core.inference import FlowEstimator
    B, H, W, T = 2, 64, 128, 5
    mk = lambda **kw: FlowEstimator(dict(flownet='C'), B, net_size=(H, W), device=dev, sequence=True, **kw)   # noqa: E731
    est, fresh, eager = mk(), mk(), mk(use_graph=False)
    for e in (est, fresh, eager):
        _params(e, 'C')
    A, Bc = clip(T, H, W, 40), clip(T, H, W, 41)
    a1 = est.estimate_sequence(A)
    a2 = est.estimate_sequence(A)                         # reset() inside
    assert all(np.array_equal(x, y) for x, y in zip(a1, a2))
    g = est.graph
    est.reset()
    b1 = est.estimate_sequence(iter(Bc))                  # clip A, reset, clip B: nothing of A may be carried into B
    b2 = fresh.estimate_sequence(Bc)
    assert len(b1) == T - 1 and all(np.array_equal(x, y) for x, y in zip(b1, b2))
    assert est.graph is g and g is not None               # one graph, never re-captured
    assert not np.array_equal(a1[0], b1[0])
    b3 = eager.estimate_sequence(Bc)
    assert eager.graph is None and all(np.array_equal(x, y) for x, y in zip(b1, b3))


# ------------------------------------------------------------------------------------------------- 6. short pushes
def test_short_pushes(dev):
    from unflow_amd.core.inference import FlowEstimator
    B, H, W = 2, 64, 128
    frames = clip(7, H, W, 32)[:6]                        # the first six frames of test 3's 64 x 128 clip: its oracle flows
    ref = _oracle_flows(('C', H, W, 7), 'C', clip(7, H, W, 32), H, W)
    est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), device=dev, sequence=True)
    _params(est, 'C')
    est.reset()
    got, n0 = [], 0
    for k, want in ((1, 0), (2, 2), (1, 1), (2, 2)):
        out = est.push(frames[n0:n0 + k])
        assert len(out) == want, (k, len(out))
        got += out
        n0 += k
    assert len(got) == 5
    epes = [_epe(f, r) for f, r in zip(got, ref)]
    print("short pushes: EPE per pair vs fp64 oracle %s (bound %g)" % (["%.2e" % e for e in epes], _bound()))
    assert max(epes) < _bound(), epes
    with pytest.raises(ValueError):
        est.push(frames[:B + 1])
    with pytest.raises(ValueError):
        est.push([])
    with pytest.raises(ValueError):
        est.push([np.zeros((32, 128, 3), np.float32)])    # another size than the clip's
    with pytest.raises(ValueError):
        est.estimate_sequence(frames[:1])


# ------------------------------------------------------------------------------------------------- 7. export and CLI
def test_export_sequence_and_cli(dev, tmp_path):
    from unflow_amd.core.inference import FlowEstimator
    from unflow_amd.core.input import read_flo, read_kitti_flow_png, write_png_rgb8
    from unflow_amd.core.train import Trainer
    H, W = 64, 128
    frames = clip(5, H, W, 50, u8=True)
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
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), device=dev, sequence=True)
    assert est.global_step == 7
    flows = est.estimate_sequence(frames)
    assert max(float(np.abs(f).max()) for f in flows) > 0.05
    paths = est.export_sequence(frames, str(tmp_path / "flo"), fmt='flo')
    assert [os.path.basename(p) for p in paths] == ['%06d_10.flo' % i for i in range(4)]
    for p, f in zip(paths, flows):
        back, _ = read_flo(p)
        assert np.array_equal(np.asarray(back), f)
    ppaths = est.export_sequence(iter(frames), str(tmp_path / "png"), fmt='png')
    assert [os.path.basename(p) for p in ppaths] == ['%06d_10.png' % i for i in range(4)]
    for p, f in zip(ppaths, flows):
        back, mask = read_kitti_flow_png(p)
        q = np.clip(np.float32(f) * np.float32(64) + np.float32(32768), 0, 65535).astype(np.uint16)
        assert np.array_equal(back.numpy(), (q.astype(np.float32) - 2 ** 15) / 64.0) and (mask.numpy() == 1).all()
    # the command line, as a child process: the same files
    cfg = tmp_path / "config.ini"
    cfg.write_text("[dirs]\nlog = %s\ncheckpoints = %s\n\n[train]\nflownet = C\n" % (tmp_path / "log", tmp_path / "ckpts"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', str(fdir), '--out',
                        str(tmp_path / "cli"), '--flo', '--batch', '2', '--net_size', str(H), str(W), '--config', str(cfg)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cli = sorted(os.listdir(str(tmp_path / "cli" / "clipnet")))
    assert cli == ['%06d_10.flo' % i for i in range(4)]
    for name, p in zip(cli, paths):
        with open(os.path.join(str(tmp_path / "cli" / "clipnet"), name), 'rb') as fa, open(p, 'rb') as fb:
            assert fa.read() == fb.read(), name


# ------------------------------------------------------------------------------------------------- 8. memory
def test_sequence_engine_memory(dev):
    """The sequence engine holds B + 1 rows of the network input and of FlowNetC's tower buffers where the pair engine holds 2B:
    at least B - 1 rows of x0, c1, cat2 and c3 (fp32 plus operand planes, from the pair engine's own layout) less."""
    from unflow_amd.core.engine import FlowNetEngine
    B, H, W = 4, 384, 1280

    # The bytes the engine asks for, from the allocator's own count: memory_allocated counts whole blocks — a large block is handed
    # out unsplit when less than 1 MiB of it would remain — and the two engines differ by exactly the derived bytes, so that
    # rounding (up to 1 MiB per tensor, either way) must not enter the comparison with them
    requested = lambda: torch.cuda.memory_stats(dev)['requested_bytes.all.current']   # noqa: E731

    def built(**kw):
        import gc
        gc.collect()
        torch.cuda.synchronize()
        a, r = torch.cuda.memory_allocated(dev), requested()
        e = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=None, inference=True, **kw)
        torch.cuda.synchronize()
        return e, torch.cuda.memory_allocated(dev) - a, requested() - r
    pair, m_pair, r_pair = built()
    seq, m_seq, r_seq = built(sequence=True)
    st = pair.stages[0]
    row = lambda pt: pt.t[0].numel() * 4 + (0 if pt.pl is None else pt.pl[:, 0].numel() * 2)   # noqa: E731
    derived = (B - 1) * sum(row(pt) for pt in (pair.X0, st.A['c1'], st.A['cat2'], st.A['c3']))
    print("engine memory: sequence %.1f MB, pair mode %.1f MB, derived saving %.1f MB" % (m_seq / 1e6, m_pair / 1e6, derived / 1e6))
    assert seq.x0.shape[0] == B + 1 and seq.stages[0].A['c3'].t.shape[0] == B + 1 and seq.stages[0].A['cat3'].t.shape[0] == B
    print("requested bytes: sequence %d, pair mode %d, saving %d, derived %d" % (r_seq, r_pair, r_pair - r_seq, derived))
    assert m_seq < m_pair and r_seq < r_pair and r_pair - r_seq >= derived, (m_pair, m_seq, r_pair, r_seq, derived)
