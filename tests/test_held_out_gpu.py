"""-m gpu: FlowEstimator(..., sequence=..., interpolate=n, held_out=True) — the scores of push_held_out against the
numpy definition of tests/mid_score_ref.py applied to the estimator's own in-between frames and the clip's frames; pushes, reset,
eager launches, the first replay ever and truths on the device bit-identical; beside an estimator without the option;
evaluate_interpolation against pushing by hand; and the command line against the API."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mid_score_ref as R
import test_interpolate_gpu as TI       # its configurations and the checkpoint fixture (not its estimators: they must stay fresh)
import test_sequence_gpu as SG
from test_interpolate_gpu import checkpoint  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = SG.ROOT
H, W, FH, FW, MAXF = TI.H, TI.W, TI.FH, TI.FW, TI.MAXF
NET = 5                                 # network frames per clip
CONFIGS = TI.CONFIGS                    # 'fw-B2-n1-u8', 'bi-B2-n3-f32': sequence, batch, n, uint8 frames, the pushes of 5 frames
GEOM = dict(Hmax=MAXF[0], Wmax=MAXF[1], h=FH, w=FW)
_EST, _FIRST = {}, {}


def _full(name, seed=81, extra=0):
    """A full-rate clip for NET network frames (and `extra` trailing frames that complete no pair)."""
    _, _, n, u8, _ = CONFIGS[name]
    return SG.clip((NET - 1) * (n + 1) + 1 + extra, FH, FW, seed, u8=u8)


def _split(name, full):
    """(network frames, truths per network frame: None, then the n frames before each)."""
    n = CONFIGS[name][2]
    pairs = (len(full) - 1) // (n + 1)
    return full[:pairs * (n + 1) + 1:n + 1], [None] + [full[p * (n + 1) + 1:(p + 1) * (n + 1)] for p in range(pairs)]


def _estimator(name, dev, use_graph=True, held_out=True):
    """The estimator of a configuration, built once; held_out=False: the same interpolating estimator without the option."""
    from unflow_amd.core.inference import FlowEstimator
    key = (name, use_graph, held_out)
    if key not in _EST:
        seq, B, n, _, _ = CONFIGS[name]
        est = FlowEstimator(dict(flownet='C'), B, net_size=(H, W), max_frame=MAXF, device=dev, sequence=seq, use_graph=use_graph,
                            interpolate=n, held_out=held_out)
        tfp = SG._params(est, 'C')
        if seq == 'bidirectional':
            est.load_tf_params({k: (v * TI.HEAD_SCALE if k.split('/')[-2].startswith('flow') and k.endswith('/weights') else v)
                                for k, v in tfp.items()})
        _EST[key] = est
    return _EST[key]


def _pushed(est, net, truths, pushes):
    est.reset()
    got, n0 = [], 0
    for k in pushes:
        out = est.push_held_out(net[n0:n0 + k], truths[n0:n0 + k])
        assert len(out) == (k if n0 else k - 1)
        got += out
        n0 += k
    assert n0 == len(net)
    return got


def _first(name, dev):
    """The whole clip in pushes of B as the estimator's first replay ever (the eager pass, the capture, the first replay)."""
    if name not in _FIRST:
        fresh = (name, True, True) not in _EST
        est = _estimator(name, dev)
        assert fresh and est.graph is None
        net, truths = _split(name, _full(name))
        B = CONFIGS[name][1]
        _FIRST[name] = _pushed(est, net, truths, [B] * (NET // B) + ([NET % B] if NET % B else []))
        assert est.graph is not None
    return _FIRST[name]


def _same(a, b):
    return len(a) == len(b) and all(x.frames.tobytes() == y.frames.tobytes() and np.array_equal(x.holes, y.holes) and
                                    x.sse.tobytes() == y.sse.tobytes() and x.psnr.tobytes() == y.psnr.tobytes() and
                                    x.ssim.tobytes() == y.ssim.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_scores_are_the_mirror_on_the_estimators_own_frames(name, dev):
    from unflow_amd.core.inference import HeldOut
    _, _, n, u8, _ = CONFIGS[name]
    got = _first(name, dev)
    net, truths = _split(name, _full(name))
    assert len(got) == NET - 1 and all(isinstance(g, HeldOut) for g in got)
    wins = 3 * (FH - 7) * (FW - 7)
    worst = 0.0
    for p, g in enumerate(got):
        assert g.frames.shape == (n, FH, FW, 3) and g.sse.shape == g.psnr.shape == g.ssim.shape == (n, 3) and g.sse.dtype == np.int64
        stage = lambda a: np.ascontiguousarray(a if u8 else np.asarray(a, np.float32))       # noqa: E731
        sse, ssim, mag = R.score_pair(stage(net[p]), stage(net[p + 1]), g.frames, np.stack([stage(t) for t in truths[p + 1]]), FH, FW, n)
        assert np.array_equal(g.sse, sse), (name, p, g.sse, sse)
        # the kernel's sum within R.ssim_bound of the exactly rounded sum; the mean and its product with the count below round twice
        err, bound = np.abs(g.ssim * wins - ssim), R.ssim_bound(GEOM, mag) + mag * 2.0 ** -52
        assert (err <= bound).all(), (name, p, g.ssim * wins, ssim, err, bound)
        worst = max(worst, float((err / bound).max()))
        with np.errstate(divide='ignore'):
            assert np.array_equal(g.psnr, 10.0 * np.log10(255.0 ** 2 * (3 * FH * FW) / sse.astype(np.float64)))
        assert (g.sse > 0).all() and (g.sse[:, 0] != g.sse[:, 1]).any()
    print("%s: worst |ssim sum - fsum| / bound = %.3g; pair 0: psnr %s ssim %s" % (name, worst, got[0].psnr[0], got[0].ssim[0]))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pushes_reset_eager_and_device_truths_are_bit_identical(name, dev):
    ref = _first(name, dev)
    est = _estimator(name, dev)
    net, truths = _split(name, _full(name))
    g = est.graph
    assert _same(_pushed(est, net, truths, CONFIGS[name][4]), ref) and est.graph is g
    # another clip in between leaves nothing behind
    other = _split(name, _full(name, seed=82))
    assert not _same(_pushed(est, other[0][:3], other[1][:3], (3,) if CONFIGS[name][1] >= 3 else (2, 1)), ref[:2])
    # frames and truths on the device, truths as one [n, h, w, 3] tensor
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    dnet, dtruths = [to(f) for f in net], [None if t is None else to(np.stack(t)) for t in truths]
    assert _same(_pushed(est, dnet, dtruths, CONFIGS[name][4]), ref)
    eager = _estimator(name, dev, use_graph=False)
    assert _same(_pushed(eager, net, truths, CONFIGS[name][4]), ref) and eager.graph is None
    assert not bool(est.mid_score_ws.any()) and not bool(est.mid_sums.any())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_a_scoring_estimator_returns_what_one_without_the_option_returns(name, dev):
    ref = _first(name, dev)
    est, plain = _estimator(name, dev), _estimator(name, dev, held_out=False)
    net, truths = _split(name, _full(name))
    assert not plain.held_out and plain.mid_truth is None and plain.mid_score_prev is None and plain.mid_score_ws is None
    assert plain.out_mid_sse is None and plain.out_mid_ssim is None
    want = plain.interpolate_sequence(net)
    assert all(np.array_equal(a.frames, b.frames) and np.array_equal(a.holes, b.holes) for a, b in zip(ref, want)) and len(want) == len(ref)
    # push_interpolated on the scoring estimator: held = 0, nothing scored, what it returns today
    est.out_mid_sse.fill_(-5)
    est.reset()
    mids = est.push_interpolated(net[:2]) + est.push_interpolated(net[2:4]) + est.push_interpolated(net[4:])
    assert TI._same_mids(mids, want) and bool((est.out_mid_sse == -5).all())
    assert int(est.tab[8 * est.B + 6].item()) == 0
    a, b = est.estimate_sequence(net), plain.estimate_sequence(net)
    assert len(a) == NET - 1 and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    for call in (lambda: plain.push_held_out(net[:2], truths[:2]), lambda: plain.evaluate_interpolation([net])):
        with pytest.raises(RuntimeError, match="without held-out frames.*held_out=True"):
            call()


def test_the_truths_are_checked_before_anything_is_staged(dev):
    name = 'fw-B2-n1-u8'
    _first(name, dev)
    est = _estimator(name, dev)
    net, truths = _split(name, _full(name))
    est.reset()
    k0 = est._seq_k
    for bad, msg in (([None], "2 frames, 1 sets"), ([None, None], "frame 1 has no held-out"), ([None, truths[1] * 2], "frame 1 comes with 2"),
                     ([None, [truths[1][0][:-1]]], "frame 1 have the clip's size"),
                     ([None, [truths[1][0].astype(np.float32)]], "frame 1 have the clip's size and type")):
        with pytest.raises(ValueError, match=msg):
            est.push_held_out(net[:2], bad)
        assert est._seq_k == k0 and est._carry == 0
        est.reset()
    assert len(est.push_held_out(net[:2], truths[:2])) == 1
    with pytest.raises(ValueError, match="frame 0 has no held-out"):
        est.push_held_out(net[2:3], [None])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_evaluate_interpolation_equals_pushing_each_clip_by_hand(name, dev):
    ref = _first(name, dev)
    est = _estimator(name, dev)
    n = CONFIGS[name][2]
    second = _full(name, seed=83, extra=n)[:(2 * (n + 1) + 1) + n]          # two pairs and n trailing frames
    out = est.evaluate_interpolation(iter([_full(name, extra=1), second]))
    net2, truths2 = _split(name, second)
    assert len(net2) == 3
    hand = ref + _pushed(est, net2, truths2, (2, 1))
    assert out['num_examples'] == len(hand) == NET + 1 and out['per_clip'] == [NET - 1, 2]
    assert all(np.array_equal(f['sse'], g.sse) and f['psnr'].tobytes() == g.psnr.tobytes() and f['ssim'].tobytes() == g.ssim.tobytes()
               and np.array_equal(f['holes'], g.holes) for f, g in zip(out['per_frame'], hand))
    sse = sum(g.sse for g in hand)
    px, wins = len(hand) * FH * FW, len(hand) * 3 * (FH - 7) * (FW - 7)
    for k, kind in enumerate(R.KINDS):
        assert out['psnr/' + kind] == 10.0 * np.log10(255.0 ** 2 * (3 * px * n) / float(sse[:, k].sum()))
        assert out['psnr_j/' + kind] == [10.0 * np.log10(255.0 ** 2 * (3 * px) / float(v)) for v in sse[:, k]]
        mean_j = np.mean([g.ssim[:, k] for g in hand], axis=0)              # equal sizes: the pooled mean is the mean of the means
        assert np.allclose(out['ssim_j/' + kind], mean_j, rtol=1e-13, atol=0) and abs(out['ssim/' + kind] - mean_j.mean()) < 1e-13
    assert out['holes'] == sum(int(g.holes.sum()) for g in hand) / (n * px)
    assert out['psnr/mid'] != out['psnr/blend'] and len(est.evaluate_interpolation([_full(name)], num=3)['per_frame']) == 3
    with pytest.raises(ValueError, match="holds no pair"):
        est.evaluate_interpolation([_full(name)[:n + 1]])


def test_the_command_line_prints_the_numbers_of_the_api(dev, tmp_path, checkpoint):  # noqa: F811
    """python -m unflow_amd.sequence --interpolate 1 --held_out on four frames: frames 0 and 2 go to the network, frame 1 is held
    out, frame 3 is dropped; the table is the API's, the files are those of the subsampled clip."""
    from unflow_amd import sequence as S
    from unflow_amd.core.inference import FlowEstimator
    frames, fdir, ckpt_dir, cfg = checkpoint
    est = FlowEstimator.from_checkpoint(ckpt_dir, dict(flownet='C'), 2, net_size=(H, W), max_frame=(FH, FW), device=dev,
                                        sequence=True, interpolate=1, held_out=True)
    scores = est.evaluate_interpolation([frames])
    assert scores['num_examples'] == 1
    want = est.interpolate_sequence(frames[:3:2])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'unflow_amd.sequence', '--ex', 'clipnet', '--frames', fdir, '--out', str(tmp_path / "cli"),
                        '--batch', '2', '--net_size', str(H), str(W), '--config', cfg, '--interpolate', '1', '--held_out'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "dropped 1 trailing frame(s) that complete no pair of 1 held-out frame(s)" in lines
    table = S.held_out_table(scores, 1)
    at = lines.index(table[0])
    assert lines[at:at + len(table)] == table, r.stdout
    out = str(tmp_path / "cli" / "clipnet")
    assert sorted(os.listdir(out)) == ['000000_10.png', '000000_mid1.png']
    assert np.array_equal(TI._decoded(os.path.join(out, '000000_mid1.png')), want[0].frames[0])
