"""-m gpu: the kernels of csrc/conv_igemm.hip that are no GEMM at all — the Cout <= 4 flow heads (tile, strip and per-pixel forms), the
2 -> 2 upsamplers, pointwise32_dgrad_kernel and flow_wgrad_batched — on the case table of tests/head_cases.py.

They work in plain fp32 (fused multiply-adds, fixed-order sums), so on the exact-input regimes of tests/exact_inputs.py they must equal
the fp64 result BIT FOR BIT in any summation order: (a) runs forward, data gradient (overwrite / accumulate / accumulate with a real
leaky derivative: run_dgrad) and filter gradient of every case through the fp32 entries and the operand-plane entries, in 'dense' (a
lost tap, strip, row, quad group or pass) and 'A3' (24 significant bits in one operand: a value taken through a 16-bit plane).  (b)
flow_wgrad_batched with one layer of each kind, (c) the refusals, (d) random data of six decades against the theorem bound
|got - fp64| <= gamma(n) sum |terms| (reference_pin.gamma; nothing tuned), (e) run-to-run determinism of the filter gradients.

Which kernel form a case reaches is stated in the table and asserted against the dispatch mirror before the GPU is asked
(HC.check_case); profiles/heads_kernel_trace.txt is the kernel trace of this file.

Measured on an MI355X: 249 tests in 13 s, the slowest 1.0 s (tile8_spw4).  Largest |got - fp64| / bound of (d): forward 0.0017 (tile8),
7e-5 (strip4), 0.0009 (skinny), 0.50 (2 -> 2: nine terms); data gradient 0.18 - 0.43 in every form; filter gradient 5e-5 (tile8), 0.047
(strip4), 0.031 (skinny), 1e-4 (2 -> 2), batched 4e-5 / 0.053 / 4e-5 (every figure is printed with -s)."""
import functools

import pytest
import torch

import dgrad_epilogue as D
import exact_inputs as E
import head_cases as HC
from test_exact_terms_gpu import _wgrad_problem, assert_exact, run_dgrad, run_forward, run_wgrad
from test_planes_gpu import lib_option  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
REGIMES = ('dense', 'A3')
UNSUPPORTED = -7


def _entries(c):
    return ('f32',) if c.kind == 'tiny' else ('f32', 'pl')


def _params(cases):
    return [pytest.param(c, entry, regime, id="%s-%s-%s" % (c.id, entry, regime)) for c in cases for regime in REGIMES for entry in _entries(c)]


def _hi(c):
    return 2 if c.kind != 'tiny' and c.shape[3] == 4 else None               # one quad: a range that ends inside it


# ----------------------------------------------------------------------------------------------------------------------------
# (a) exact
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,entry,regime", _params(HC.HEADS + HC.TEMPLATES + HC.TINY))
def test_forward_exact(c, entry, regime, dev):
    HC.check_case(c)
    run_forward(regime, HC.conv7(c), dev, 3, deconv=c.kind == 'tiny', entry=entry)


@pytest.mark.parametrize("c,entry,regime", _params(HC.ALL))
def test_data_gradient_exact(c, entry, regime, dev):
    HC.check_case(c)
    run_dgrad(regime, HC.conv7(c), dev, 3, deconv=c.kind == 'tiny', entry=entry, hi=_hi(c))


@pytest.mark.parametrize("c,entry,regime", _params(HC.HEADS + HC.TINY))
def test_filter_gradient_exact(c, entry, regime, dev):
    HC.check_case(c)
    B, H, W, Cin, Cout, k, stride = HC.conv7(c)
    tiny = c.kind == 'tiny'
    run_wgrad(regime, (B, 2 * H, 2 * W, Cin, Cout, k, stride, True) if tiny else (B, H, W, Cin, Cout, k, stride, False), dev, 3, entry=entry)


# ----------------------------------------------------------------------------------------------------------------------------
# (b) flow_wgrad_batched
# ----------------------------------------------------------------------------------------------------------------------------
def _batch_jobs(ids, regime, dev):
    jobs, refs, guards = [], [], []
    for cid in ids:
        c = HC.BY_ID[cid]
        x, dz, ref = _wgrad_problem(regime, HC.conv7(c), c.kind == 'tiny')
        guard = torch.full((ref.numel() + 128,), float('nan'), device=dev)
        jobs.append((HC.batch_kind(c), x.float().to(dev), dz.float().to(dev), guard[64:64 + ref.numel()].view(tuple(ref.shape))))
        refs.append(ref)
        guards.append(guard)
    return jobs, refs, guards


def _check_batch(ids, jobs, refs, guards, regime):
    for cid, j, ref, guard in zip(ids, jobs, refs, guards):
        assert_exact(j[3], ref, "flow_wgrad_batched %s %s" % (cid, regime))
        assert torch.isnan(guard[:64]).all() and torch.isnan(guard[64 + ref.numel():]).all(), cid


@pytest.mark.parametrize("regime", REGIMES)
def test_flow_wgrad_batched_one_layer_of_each_kind(regime, dev):
    """tile8_ragged (kind 0: strips of 8), strip4_1028 (kind 1: strips of 4) and the 2 -> 2 layer whose blocks stride (kind 2) in ONE batch."""
    from unflow_amd.core import layers as L
    ids = [b[0] for b in HC.BATCH]
    for cid, kind, spw, blocks in HC.BATCH:
        c = HC.BY_ID[cid]
        assert HC.flow_wgrad_plan(HC.batch_kind(c), *c.shape[:3], c.shape[3] if c.kind == 'head' else 2) == (kind, spw, blocks), cid
    jobs, refs, guards = _batch_jobs(ids, regime, dev)
    L.flow_wgrad_batched(jobs)
    _check_batch(ids, jobs, refs, guards, regime)


@pytest.mark.parametrize("regime", REGIMES)
def test_flow_wgrad_batched_per_layer_fallback(regime, dev):
    """A batch with a level that has no strip form (skinny_5x7): the library plans nothing, layers.flow_wgrad_batched runs every layer on
    its own entry."""
    import ctypes
    from unflow_amd import _lib
    from unflow_amd.core import layers as L
    ids = HC.BATCH_FALLBACK
    shapes = [HC.BY_ID[i].shape for i in ids]
    assert HC.flow_wgrad_plan('conv', *shapes[1]) is None and HC.flow_wgrad_plan('conv', *shapes[0]) is not None
    n = len(ids)
    arr = lambda j: (ctypes.c_int * n)(*[s[j] for s in shapes])                 # noqa: E731
    lib = _lib.lib()
    lib.unflow_flow_wgrad_batched_workspace_bytes.restype = ctypes.c_size_t
    assert lib.unflow_flow_wgrad_batched_workspace_bytes(n, (ctypes.c_int * n)(0, 0), arr(0), arr(1), arr(2), arr(3)) == 0
    jobs, refs, guards = _batch_jobs(ids, regime, dev)
    L.flow_wgrad_batched(jobs)
    _check_batch(ids, jobs, refs, guards, regime)


def test_library_plans_what_the_mirror_plans():
    """The one place where the library SAYS which strip form it takes: the scratch of a one-layer flow_wgrad_batched is blocks x filter
    size, and blocks follows from head_strip's strip size.  Every case with a strip form (both sides of the 16384-pixel threshold among
    them) and every 2 -> 2 case must get the bytes the mirror computes; a case without a strip form gets 0."""
    import ctypes
    from unflow_amd import _lib
    lib = _lib.lib()
    lib.unflow_flow_wgrad_batched_workspace_bytes.restype = ctypes.c_size_t
    one = lambda v: (ctypes.c_int * 1)(v)                                      # noqa: E731
    for c in HC.HEADS + HC.TINY:
        B, H, W = c.shape[:3]
        Cin = c.shape[3] if c.kind == 'head' else 2
        plan = HC.flow_wgrad_plan(HC.batch_kind(c), B, H, W, Cin)
        want = 0 if plan is None else (plan[2] * (64 if c.kind == 'tiny' else 18 * Cin) * 4 + 255) // 256 * 256
        got = lib.unflow_flow_wgrad_batched_workspace_bytes(1, one(1 if c.kind == 'tiny' else 0), one(B), one(H), one(W), one(Cin))
        assert got == want, "%s: the library plans %d bytes of partials, the mirror %d (%s)" % (c.id, got, want, plan)
        assert (plan is None) == (c.facts['form'] == 'skinny')


# ----------------------------------------------------------------------------------------------------------------------------
# (c) refusals write nothing
# ----------------------------------------------------------------------------------------------------------------------------
def _refused(call, *buffers):
    """call() must raise UNFLOW_ERR_UNSUPPORTED and leave every byte of the buffers as it was."""
    from unflow_amd._lib import UnflowError
    before = [b.clone() for b in buffers]
    with pytest.raises(UnflowError) as e:
        call()
    torch.cuda.synchronize()
    assert e.value.status == UNSUPPORTED
    for b, a in zip(buffers, before):
        assert torch.equal(b.view(torch.int32) if b.dtype == torch.float32 else b, a.view(torch.int32) if a.dtype == torch.float32 else a)


def test_refusals_write_nothing(dev):
    from unflow_amd.core import layers as L
    from test_planes_gpu import make_pt, weight_planes
    g = E.gen('refusals')
    B, H, W, Cin = 2, 6, 8, 12
    x = make_pt(E.ints((B, H, W, Cin), g, -2, 2).float(), dev, 3)
    act = torch.ones(B, H, W, Cin, device=dev)
    for Cout in (1, 2, 4):
        wd, w_dir, w_tr = weight_planes(E.ints((3, 3, Cin, Cout), g, -1, 1).float(), dev, 3)
        bias = torch.ones(Cout, device=dev)
        y = L.PT.alloc((B, H, W, Cout + 4), dev, 3)
        y.t.fill_(7.0)
        y.pl.fill_(D.SENTINEL)
        y2 = L.PT.alloc((B, H // 2, W // 2, Cout + 4), dev, 3)
        y2.t.fill_(7.0)
        y2.pl.fill_(D.SENTINEL)
        dx = L.PT.alloc((B, H, W, Cin + 4), dev, 3)
        dx.t.fill_(3.0)
        dx.pl.fill_(D.SENTINEL)
        yv, y2v, dxv = y.sl(0, Cout), y2.sl(0, Cout), dx.sl(0, Cin)
        # forward: stride 2, leaky
        _refused(lambda: L.conv2d_fwd(x.t, wd, bias, y2v.t, 2, False), y2.t)
        _refused(lambda: L.conv_fwd(x, wd, w_tr, bias, y2v, 2, False), y2.t, y2.pl)
        _refused(lambda: L.conv2d_fwd(x.t, wd, bias, yv.t, 1, True), y.t)
        _refused(lambda: L.conv_fwd(x, wd, w_tr, bias, yv, 1, True), y.t, y.pl)
        # data gradient: stride 2 (dz at half size)
        dz2 = make_pt(E.ints((B, H // 2, W // 2, Cout), g, -2, 2).float(), dev, 3, extra=8)
        for acc in (False, True):
            _refused(lambda: L.conv2d_bwd_data(dz2.t, wd, dxv.t, 2, accumulate=acc), dx.t)
            _refused(lambda: L.conv_bwd_data(dz2, wd, w_dir, dxv, 2, accumulate=acc, act_src=act, act_lo=0, act_hi=4), dx.t, dx.pl)
        # filter gradient: Cout 1 and 4, and k != 3
        dz = make_pt(E.ints((B, H, W, Cout), g, -2, 2).float(), dev, 3, extra=8)
        dws = [torch.full((3, 3, Cin, Cout), float('nan'), device=dev)] if Cout != 2 else \
            [torch.full((k, k, Cin, Cout), float('nan'), device=dev) for k in (1, 5)]
        for dw in dws:
            _refused(lambda: L.conv2d_bwd_filter(x.t, dz.t, dw, None, 1), dw)
            _refused(lambda: L.conv_bwd_filter(x, dz, dw, 1), dw)
        if Cout == 2:
            dw = torch.full((3, 3, Cin, 2), float('nan'), device=dev)
            _refused(lambda: L.conv2d_bwd_filter(x.t, dz2.t, dw, None, 2), dw)
    # 2 -> 2 conv_transpose: leaky, a derivative
    x2 = E.ints((B, H, W, 2), g, -2, 2).float().to(dev)
    w2 = E.ints((4, 4, 2, 2), g, -1, 1).float().to(dev)
    y = torch.full((B, 2 * H, 2 * W, 6), 7.0, device=dev)
    _refused(lambda: L.conv2d_transpose_fwd(x2, w2, torch.ones(2, device=dev), y[..., :2], True), y)
    dz = E.ints((B, 2 * H, 2 * W, 2), g, -2, 2).float().to(dev)
    dx = torch.full((B, H, W, 6), 3.0, device=dev)
    for acc in (False, True):
        _refused(lambda: L.conv2d_transpose_bwd_data(dz, w2, dx[..., :2], accumulate=acc, act_src=torch.ones(B, H, W, 2, device=dev), act_lo=0,
                                                     act_hi=2), dx)


# ----------------------------------------------------------------------------------------------------------------------------
# (d) random data against the theorem bound, (e) determinism
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _random(cid, direction):
    return HC.random_problem(HC.BY_ID[cid], direction)


def _slice_of(t, dev, extra=4, fill=0.0):
    """t (NHWC, fp64 holding fp32 values) on the device as the channel slice [0, C) of a wider buffer."""
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), fill, device=dev)
    buf[..., :t.shape[-1]] = t.float().to(dev)
    return buf, buf[..., :t.shape[-1]]


def _report(c, what, got, v, S, n):
    r = HC.bound_ratio(got.detach().cpu(), v, S, n)
    print("%-18s %-8s %-26s max |got - fp64| / bound = %.3g   (n = %d)" % (c.id, c.facts['form'], what, r, n))
    assert r <= 1.0, (c.id, what, r)


@pytest.mark.parametrize("cid", [i for i in HC.RANDOM_IDS if HC.BY_ID[i].kind != 'pointwise'])
def test_random_forward_within_the_fp32_bound(cid, dev):
    from unflow_amd.core import layers as L
    c = HC.BY_ID[cid]
    HC.check_case(c)
    p = _random(cid, 'fwd')
    _, x = _slice_of(p['x'], dev, extra=4 if c.kind == 'head' else 0)
    ybuf = torch.full(tuple(p['v'].shape[:-1]) + (c.Cout + 4,), float('nan'), device=dev)
    y, w, b = ybuf[..., :c.Cout], p['w'].float().to(dev), p['b'].float().to(dev)
    if c.kind == 'tiny':
        L.conv2d_transpose_fwd(x, w, b, y, False)
    else:
        L.conv2d_fwd(x, w, b, y, 1, False)
    _report(c, "forward", y, p['v'], p['S'], p['n'])
    assert torch.isnan(ybuf[..., c.Cout:]).all()


@pytest.mark.parametrize("cid", HC.RANDOM_IDS)
def test_random_data_gradient_within_the_fp32_bound(cid, dev):
    from unflow_amd.core import layers as L
    c = HC.BY_ID[cid]
    HC.check_case(c)
    p = _random(cid, 'dgrad')
    tiny = c.kind == 'tiny'
    Cin = p['base'].shape[-1]
    _, dz = _slice_of(p['dz'], dev, extra=4 if c.kind == 'pointwise' else 2)
    w = p['w'].float().to(dev)
    d0buf = torch.full(tuple(p['base'].shape[:-1]) + (Cin + 4,), float('nan'), device=dev)
    d1buf, d1 = _slice_of(p['base'], dev, fill=float('nan'))
    act = p['act'].float().to(dev)
    kw = {} if tiny else dict(act_src=act, act_lo=0, act_hi=p['hi'])
    if tiny:
        L.conv2d_transpose_bwd_data(dz, w, d0buf[..., :Cin], accumulate=False)
        L.conv2d_transpose_bwd_data(dz, w, d1, accumulate=True)
    else:
        L.conv2d_bwd_data(dz, w, d0buf[..., :Cin], 1, accumulate=False)
        L.conv2d_bwd_data(dz, w, d1, 1, accumulate=True, **kw)
    _report(c, "data gradient", d0buf[..., :Cin], p['v0'], p['S0'], p['n0'])
    _report(c, "data gradient, acc + slope", d1, p['v'], p['S'], p['n'])
    assert torch.isnan(d0buf[..., Cin:]).all() and torch.isnan(d1buf[..., Cin:]).all()


def _random_wgrad(c, p, dev):
    from unflow_amd.core import layers as L
    _, x = _slice_of(p['x'], dev, extra=4 if c.kind == 'head' else 0)
    _, dz = _slice_of(p['dz'], dev, extra=2)
    dw = torch.full(tuple(p['v'].shape), float('nan'), device=dev)
    if c.kind == 'tiny':
        L.conv2d_transpose_bwd_filter(x, dz, dw, None)
    else:
        L.conv2d_bwd_filter(x, dz, dw, None, 1)
    return dw, x, dz


@pytest.mark.parametrize("cid", [i for i in HC.RANDOM_IDS if HC.BY_ID[i].kind != 'pointwise'])
def test_random_filter_gradient_within_the_fp32_bound_and_bit_stable(cid, dev):
    """(d) the bound; (e) a second run — and the same layer through flow_wgrad_batched where it has a plan, twice — gives the same bits."""
    from unflow_amd.core import layers as L
    c = HC.BY_ID[cid]
    HC.check_case(c)
    p = _random(cid, 'wgrad')
    dw, x, dz = _random_wgrad(c, p, dev)
    _report(c, "filter gradient", dw, p['v'], p['S'], p['n'])
    again = _random_wgrad(c, p, dev)[0]
    assert torch.equal(dw.view(torch.int32), again.view(torch.int32)), "filter gradient differs run to run"
    if c.facts['form'] == 'skinny':
        return
    outs = []
    for _ in range(2):
        o = torch.full_like(dw, float('nan'))
        L.flow_wgrad_batched([(HC.batch_kind(c), x, dz, o)])
        outs.append(o)
    _report(c, "flow_wgrad_batched", outs[0], p['v'], p['S'], p['n'])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "flow_wgrad_batched differs run to run"
