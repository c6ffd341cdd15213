"""-m gpu: the supervised fine-tuning step (supervised.py:12-65) — the fused flow-upsampling + masked Charbonnier kernel, the
one-direction engine (FlowNetEngine(supervised=True)) against the oracle's flownet(backward_flow=False), the whole step against
the fp64 oracle, graphs, and the supervised Trainer.

Tolerances are the unsupervised parity tests': loss rel 1e-4, final-flow EPE 1e-3 px, parameter gradients 2e-4 of each
tensor's max against the fp64 oracle differentiated along the engine's leaky-ReLU branches (parity_util.BranchAligned);
fp16 mode against the fp32 oracle with tests/test_f16_gpu.py's stated bounds."""
import os

import numpy as np
import pytest
import torch

from parity_util import BranchAligned, check_grads, images, max_rel

pytestmark = pytest.mark.gpu

CHANNEL_MEAN = [104.920005, 110.1753, 114.785955]


# ------------------------------------------------------------------------------------------------------------------ kernel
def _kernel(flow, gt, mask, scale, weight, d_init=None, accumulate=0):
    from unflow_amd import _lib
    from unflow_amd._lib import ptr, cf, check, stream
    B, h, w, _ = flow.shape
    H, W = gt.shape[1:3]
    loss = torch.zeros(1, device=flow.device)
    d = torch.zeros_like(flow) if d_init is None else d_init.clone()
    check(_lib.lib().unflow_supervised_flow_loss(ptr(flow), h, w, ptr(gt), ptr(mask), cf(scale), cf(weight), ptr(loss), ptr(d),
                                                 accumulate, B, H, W, stream()), "supervised_flow_loss")
    torch.cuda.synchronize()
    return loss, d


@pytest.mark.parametrize("r,h,w,masked,accumulate", [(4, 13, 21, True, 0), (4, 17, 19, False, 1), (4, 20, 48, True, 1),
                                                     (1, 37, 45, True, 1), (1, 29, 70, False, 0), (2, 11, 35, True, 0),
                                                     (8, 9, 13, True, 1)])
def test_supervised_flow_loss_kernel_vs_fp64_autograd(r, h, w, masked, accumulate, dev):
    from oracle import model_ref as M
    g = torch.Generator().manual_seed(100 * r + h)
    B, H, W = 2, h * r, w * r
    flow = torch.randn(B, h, w, 2, generator=g) * 0.7
    gt = torch.randn(B, H, W, 2, generator=g) * 10
    mask = (torch.rand(B, H, W, 1, generator=g) > 0.3).float() if masked else None
    scale, weight = 20.0, 0.5
    d0 = torch.randn(B, h, w, 2, generator=g) if accumulate else None
    f64 = flow.double().requires_grad_()
    ref = weight * M.charbonnier_loss(M.resize_bilinear_tf1(f64, H, W) * scale - gt.double(),
                                      None if mask is None else mask.double())
    ref.backward()
    dref = f64.grad + (d0.double() if accumulate else 0.0)
    md = None if mask is None else mask.to(dev)
    loss, d = _kernel(flow.to(dev), gt.to(dev), md, scale, weight, None if d0 is None else d0.to(dev), accumulate)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    assert max_rel(d, dref) <= 1e-5, max_rel(d, dref)
    _, d2 = _kernel(flow.to(dev), gt.to(dev), md, scale, weight, None if d0 is None else d0.to(dev), accumulate)
    assert torch.equal(d, d2)                                      # a gather: bit-reproducible
    # the flow the loss sees is unflow_resize_bilinear_tf1's, bit for bit: with that as the GT every difference is exactly 0
    from unflow_amd._lib import ptr, cf, check, stream
    from unflow_amd import _lib
    up = torch.empty(B, H, W, 2, device=dev)
    check(_lib.lib().unflow_resize_bilinear_tf1(ptr(flow.to(dev)), ptr(up), B, h, w, 2, H, W, cf(scale), stream()), "resize")
    loss0, dz = _kernel(flow.to(dev), up, md, scale, weight)
    assert torch.count_nonzero(dz).item() == 0
    n_on = float(mask.sum()) * 2 if masked else B * H * W * 2.0
    assert abs(loss0.item() - weight * n_on * 1e-6 ** 0.45 / (B * H * W * 2)) <= 1e-5 * loss0.item()


def test_supervised_flow_loss_rejects_other_factors(dev):
    from unflow_amd import _lib
    from unflow_amd._lib import ptr, cf, stream
    f = torch.zeros(1, 8, 8, 2, device=dev)
    gt = torch.zeros(1, 24, 24, 2, device=dev)
    loss = torch.zeros(1, device=dev)
    assert _lib.lib().unflow_supervised_flow_loss(ptr(f), 8, 8, ptr(gt), ptr(None), cf(20), cf(1), ptr(loss), ptr(None), 0,
                                                  1, 24, 24, stream()) == -5
    assert _lib.lib().unflow_supervised_flow_loss(ptr(f), 8, 8, ptr(gt), ptr(None), cf(20), cf(1), ptr(loss), ptr(None), 0,
                                                  1, 32, 16, stream()) == -5


# ------------------------------------------------------------------------------------------------------------------ oracle
def _sup_order(eng):
    """Leaky-ReLU call order of the oracle's flownet(backward_flow=False) for the one-direction engine: FlowNetC features of im1
    (rows 0:B), of im2 (rows B:2B), then flownet_c on rows 0:B; a FlowNetS on rows 0:B (+ deconv1 / deconv0 with full_res)."""
    from parity_util import _FEATURE_ACTS, _FLOWNETC_ACTS, _FLOWNETS_ACTS
    B = eng.B
    out = []
    for st in eng.stages:
        if st.is_c:
            out += [(a, slice(0, B), st.act) for a in _FEATURE_ACTS] + [(a, slice(B, 2 * B), st.act) for a in _FEATURE_ACTS]
            out += [(a, slice(0, B), st.act) for a in _FLOWNETC_ACTS]
        else:
            acts = list(_FLOWNETS_ACTS)
            if st.full_res:
                acts[0] = ('cat1', 0, 64)
                lo1, n1 = st.bufs['cat1'][1]['deconv1']
                lo0, n0 = st.bufs['cat0'][1]['deconv0']
                acts += [('cat1', lo1, lo1 + n1), ('cat0', lo0, lo0 + n0)]
            out += [(a, slice(0, B), st.act) for a in acts]
    return out


def _oracle(tfp, im1, im2, fgt, mgt, params, aug=None, dtype=torch.float64, backward=True):
    """supervised_loss (supervised.py:12-65) on the oracle: (loss, final flow of the last network, grads)."""
    from oracle import model_ref as M
    P = {k: v.clone().to(dtype) for k, v in tfp.items()}
    for v in P.values():
        v.requires_grad_(backward)
    mean = torch.tensor(CHANNEL_MEAN, dtype=dtype) / 255.0
    a, b = im1.to(dtype) / 255.0, im2.to(dtype) / 255.0
    if aug is not None:
        a, b = M.random_photometric_apply([a, b], *(aug[k].to(dtype) for k in ('contrast', 'gamma', 'colour', 'noise', 'brightness')))
    spec, full_res, train_all = params['flownet'], bool(params.get('full_res')), bool(params.get('train_all'))
    with torch.set_grad_enabled(backward):
        flows = M.flownet(P, a - mean, b - mean, spec, backward_flow=False, train_all=train_all, full_resolution=full_res)
        if not train_all:
            flows = [flows[-1]]
        H, W = im1.shape[1:3]
        loss, finals = 0.0, []
        for i, nf in enumerate(reversed(flows)):
            final = nf[0] * 20 if full_res else M.resize_bilinear_tf1(nf[0], H, W) * 20
            finals.append(final)
            loss = loss + M.charbonnier_loss(final - fgt.to(dtype), mgt.to(dtype)) / 2 ** i
        loss = loss + M.regularization_loss(P)
    grads = None
    if backward:
        loss.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()}
    return loss.item(), finals[0].detach(), grads


def _init(eng, seed):
    """Parameters of the engine's spec; stacks with their flow heads scaled by 0.3, as tests/test_engine_gpu.py does: random
    stacks blow the flow up to hundreds of pixels, where the warp's sample points sit within fp32 noise of pixel boundaries."""
    tfp = eng.init_params(seed=seed)
    if len(eng.spec) > 1:
        for k in tfp:
            if k.split('/')[-2].startswith('flow') and k.endswith('/weights'):
                tfp[k] = tfp[k] * 0.3
        eng.load_tf_params(tfp)
    return tfp


def _gt(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    base = torch.stack([3.0 + 2.0 * torch.sin(xx / 37.0), -1.0 + 1.5 * torch.cos(yy / 23.0)], -1)
    flow = base[None].repeat(B, 1, 1, 1) + torch.randn(B, H, W, 2, generator=g) * 0.5
    mask = (torch.rand(B, H, W, 1, generator=g) > 0.4).float()
    return flow, mask


@pytest.mark.parametrize("spec", ['C', 'S', 'CSS'])
def test_one_direction_flows_vs_oracle(spec, dev):
    """The engine's flows of every network against M.flownet(..., backward_flow=False); decoder buffers have B rows, the
    FlowNetC feature tower 2B."""
    from unflow_amd.core.engine import FlowNetEngine, flow_error_avg
    from oracle import model_ref as M
    B, H, W = 2, 128, 192
    eng = FlowNetEngine(B, H, W, params=dict(flownet=spec), device=dev, seed=None, supervised=True)
    tfp = _init(eng, 21)
    im1, im2 = images(B, H, W, 22)
    fgt, mgt = _gt(B, H, W, 23)
    eng.set_input(im1, im2, target=(fgt, mgt))
    eng.forward_net()
    torch.cuda.synchronize()
    mean = torch.tensor(CHANNEL_MEAN) / 255.0
    ref = M.flownet(tfp, im1 / 255.0 - mean, im2 / 255.0 - mean, spec, backward_flow=False)
    for st, rf in zip(eng.stages, ref):
        for lvl, r in zip(st.flow_levels, rf):
            got = st.act['flow%d' % lvl]
            assert got.shape[0] == B
            epe = flow_error_avg(got * 20, (r * 20).to(dev)).item()
            assert epe < 1e-3, (st.kind, st.index, lvl, epe)
        for name in ('cat3', 'c4', 'cat4', 'cat5', 'c6_1'):
            assert st.A[name].t.shape[0] == B
        assert st.A['cat2'].t.shape[0] == (2 * B if st.is_c else B)
        if st.is_c:
            assert st.A['c1'].t.shape[0] == 2 * B and st.A['c3'].t.shape[0] == 2 * B and st.A['catc'].t.shape[0] == B
    fw, bw = eng.final_flows()
    assert bw is None and fw.shape == (B, H, W, 2)


STEP_CASES = [('C', 2, 128, 192, dict(), True), ('CSS', 1, 64, 128, dict(), False),
              ('CSS', 1, 64, 128, dict(train_all=True), False), ('S', 1, 64, 128, dict(full_res=True), False),
              ('C', 4, 320, 768, dict(), False)]


@pytest.mark.parametrize("spec,B,H,W,extra,aug", STEP_CASES, ids=['C-aug', 'CSS', 'CSS-train_all', 'S-full_res', 'C-kitti_ft'])
def test_supervised_step_vs_fp64_oracle(spec, B, H, W, extra, aug, dev):
    from unflow_amd.core.engine import FlowNetEngine, flow_error_avg
    from unflow_amd.core.supervised import supervised_loss
    from unflow_amd.core.augment import draw_supervised_augmentation
    params = dict(flownet=spec, **extra)
    eng = FlowNetEngine(B, H, W, params=params, device=dev, seed=None, supervised=True)
    tfp = _init(eng, 31)
    im1, im2 = images(B, H, W, 32)
    fgt, mgt = _gt(B, H, W, 33)
    draws = draw_supervised_augmentation(B, torch.Generator().manual_seed(34)) if aug else False
    loss, fw = supervised_loss((im1.to(dev), im2.to(dev), fgt.to(dev), mgt.to(dev)), params, augment=draws, engine=eng,
                               backward=True, return_flow=True)
    loss = loss.item()
    got = eng.export_tf_grads()
    with BranchAligned(None, _sup_order(eng)) as al:
        loss_ref, ffw, grads = _oracle(tfp, im1, im2, fgt, mgt, params, aug=draws or None)
    print("%s: leaky units flipped in fp64: %d of %d" % (spec, al.flips, al.units))
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref), (loss, loss_ref)
    epe = flow_error_avg(fw, ffw.float().to(dev)).item()
    assert epe < 1e-3, epe
    if len(spec) == 1:
        check_grads(got, grads, tfp, 2e-4, 2e-4, label=spec)
    else:
        # the stacked bound of tests/test_engine_gpu.py::test_flownet_s_and_stacks_vs_oracle: the refinement input (warp by the
        # previous network's fp32 flow, |.|, leaky kinks) amplifies fp32 noise; 5x for the 2-element biases
        check_grads(got, grads, tfp, 1e-2, 1e-2, small_tol=5e-2, label=spec)
    if not eng.train_all:
        for st in eng.stages[:-1]:                     # frozen networks: no data gradient
            for l in st.layers:
                assert torch.count_nonzero(l.dw).item() == 0


def test_supervised_step_f16_vs_fp32_oracle(dev, monkeypatch):
    """fp16 mode, the small FlowNetC case, with the bounds stated in tests/test_f16_gpu.py (loss 1e-2 rel, EPE 5e-2 px, gradient
    cosine > 0.99, per tensor 2 x 3e-2 of the max at this size against the branch-aligned fp32 oracle, 5x below 1024 elements)."""
    from unflow_amd.core.engine import FlowNetEngine, flow_error_avg
    monkeypatch.setenv("UNFLOW_CONV_MATH", "f16")
    B, H, W = 2, 128, 192
    params = dict(flownet='C')
    eng = FlowNetEngine(B, H, W, params=params, device=dev, seed=None, supervised=True)
    assert eng.n_planes == 1
    tfp = eng.init_params(seed=41)
    im1, im2 = images(B, H, W, 42)
    fgt, mgt = _gt(B, H, W, 43)
    loss = eng.fwd_bwd(im1.to(dev), im2.to(dev), target=(fgt, mgt)).item()
    fw, _ = eng.final_flows()
    got = eng.export_tf_grads()
    with BranchAligned(None, _sup_order(eng)):
        loss_ref, ffw, grads = _oracle(tfp, im1, im2, fgt, mgt, params, dtype=torch.float32)
    assert abs(loss - loss_ref) <= 1e-2 * abs(loss_ref)
    assert flow_error_avg(fw, ffw.to(dev)).item() <= 5e-2
    l2 = lambda k: 0.0004 * tfp[k].double() if k.endswith('/weights') else 0.0      # noqa: E731
    a = torch.cat([got[k].flatten().double() for k in grads])
    b = torch.cat([(grads[k].double() - l2(k)).flatten() for k in grads])
    assert torch.nn.functional.cosine_similarity(a, b, dim=0).item() > 0.99
    bad = []
    for k in grads:
        ref = grads[k].double() - l2(k)
        d = (got[k].double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)
        if d > (2 * 3e-2 if ref.numel() >= 1024 else 5 * 2 * 3e-2):
            bad.append((k, d))
    assert not bad, bad


@pytest.mark.parametrize("math", ['fp32'])
def test_supervised_step_fp32_mode(math, dev, monkeypatch):
    """UNFLOW_CONV_MATH=fp32 (fp32 MFMA everywhere, no operand planes): the small FlowNetC case against the fp64 oracle."""
    from unflow_amd.core.engine import FlowNetEngine
    monkeypatch.setenv("UNFLOW_CONV_MATH", math)
    B, H, W = 2, 128, 192
    eng = FlowNetEngine(B, H, W, params=dict(flownet='C'), device=dev, seed=None, supervised=True)
    assert eng.n_planes == 0
    tfp = eng.init_params(seed=51)
    im1, im2 = images(B, H, W, 52)
    fgt, mgt = _gt(B, H, W, 53)
    loss = eng.fwd_bwd(im1.to(dev), im2.to(dev), target=(fgt, mgt)).item()
    got = eng.export_tf_grads()
    with BranchAligned(None, _sup_order(eng)):
        loss_ref, _, grads = _oracle(tfp, im1, im2, fgt, mgt, dict(flownet='C'))
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref)
    check_grads(got, grads, tfp, 2e-4, 2e-4, label='fp32')


# ------------------------------------------------------------------------------------------------------------------ runner
def test_supervised_step_runner_graph_matches_eager(dev):
    from unflow_amd.core.engine import FlowNetEngine
    from unflow_amd.core.train import StepRunner
    B, H, W = 2, 128, 192
    im1, im2 = images(B, H, W, 61)
    fgt, mgt = _gt(B, H, W, 62)
    out = []
    for use_graph in (False, True):
        # (not train_all: its stack-input gradient accumulates with float atomics, like the bidirectional one, so it is not
        # bit-reproducible)
        eng = FlowNetEngine(B, H, W, params=dict(flownet='CS'), device=dev, seed=63, supervised=True)
        run = StepRunner(eng, use_graph=use_graph)
        losses = []
        for t in range(2):
            losses.append(run.step(im1.to(dev), im2.to(dev), 1e-4, target=(fgt.to(dev), mgt.to(dev))).clone())
        torch.cuda.synchronize()
        out.append((torch.cat(losses).cpu(), eng.P.clone().cpu()))
    # parameters bit-identical (every gradient is a gather or a fixed-order reduction); the loss value is a sum of
    # block partials added with float atomics (csrc/loss.hip convention), equal up to its summation order
    assert torch.equal(out[0][1], out[1][1])
    assert torch.allclose(out[0][0], out[1][0], rtol=1e-6, atol=0), (out[0][0], out[1][0])


def test_supervised_trainer_runs_saves_and_resumes_identically(tmp_path, dev):
    import shutil
    from unflow_amd.core.train import Trainer
    from unflow_amd.kitti.input import KITTIInput
    from kitti_gt_fixture import Data, make_gt_tree
    make_gt_tree(tmp_path / "kitti", n_per_dataset=(3, 3), size=(80, 140), seed=4)
    H, W = 64, 128
    inp = KITTIInput(Data(tmp_path / "kitti"), 1, (H, W), normalize=False)
    params = dict(flownet='S', learning_rate=1e-4, manual_decay_lrs=[1e-4, 5e-5], manual_decay_iters=[2, 2], save_interval=2,
                  display_interval=1)

    def batches(iter_offset):
        return inp.input_train_gt(1, seed=9, shift=iter_offset)

    ck_a, ck_b = str(tmp_path / "a"), str(tmp_path / "b")
    tr = Trainer(1, H, W, params, device=dev, seed=3, augment=False, use_graph=True, supervised=True)
    log = tr.run(0, 4, batches, ck_a)
    assert [i for i, _ in log] == [1, 2, 3, 4] and all(np.isfinite(l) for _, l in log)
    assert tr.checkpoint_step(ck_a) == 4
    final = tr.engine.export_tf_params()
    os.makedirs(ck_b)
    for f in os.listdir(ck_a):
        if 'model.ckpt-2' in f:
            shutil.copy(os.path.join(ck_a, f), ck_b)
    with open(os.path.join(ck_b, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "model.ckpt-2"\n')
    tr2 = Trainer(1, H, W, params, device=dev, seed=99, augment=False, use_graph=True, supervised=True)
    tr2.run(0, 4, batches, ck_b)
    got = tr2.engine.export_tf_params()
    for k in final:
        assert torch.equal(final[k], got[k]), k


def test_supervised_trainer_finetunes_from_unsupervised_checkpoint(tmp_path, dev):
    """A supervised CS run takes its frozen FlowNetC from an unsupervised run's checkpoint (params['finetune']) and keeps it."""
    from unflow_amd.core.train import Trainer
    from unflow_amd.core import tf_checkpoint as T
    H, W = 64, 64
    base = dict(learning_rate=1e-4, decay_interval=100000, save_interval=2, display_interval=1)
    c_dir = str(tmp_path / "C")
    trc = Trainer(1, H, W, dict(base, flownet='C'), device=dev, seed=11, augment=False, use_graph=False)
    trc.save(c_dir, 5)
    c_params = trc.engine.export_tf_params()
    del trc
    im1, im2 = images(1, H, W, 71)
    fgt, mgt = _gt(1, H, W, 72)

    def batches(iter_offset):
        while True:
            yield im1, im2, fgt, mgt

    tr = Trainer(1, H, W, dict(base, flownet='CS', finetune=[T.latest_checkpoint(c_dir)]), device=dev, seed=3, augment=True,
                 use_graph=True, supervised=True)
    ck = str(tmp_path / "a")
    os.makedirs(ck)
    log = tr.run(0, 2, batches, ck)
    assert len(log) == 2 and all(np.isfinite(l) for _, l in log)
    got = tr.engine.export_tf_params()
    for k, v in c_params.items():
        # frozen: only the L2 term moves it (the reference's optimizer spans all variables); Adam's first steps move every
        # weight by ~lr, biases not at all
        assert (got[k] - v).abs().max().item() <= 3e-4, k
        if k.endswith('/biases'):
            assert torch.equal(got[k], v), k
