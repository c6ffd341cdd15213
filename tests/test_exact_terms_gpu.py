"""-m gpu: every bf16 x 3 / fp16 matrix-core kernel path on the exact-input regimes of tests/exact_inputs.py — the result must equal the
fp64 reference BIT FOR BIT (torch.equal after .double()).  A lost product term (regimes 'A3', 'B3', 'two'), tap, K tail, tile tail,
split-K slice or parity class ('dense'), a mis-staged mid / lo plane or an 11th fp16 bit ('f16') is a mismatch here, where the
max-norm tolerances of tests/test_planes_gpu.py see a 1e-6 wobble.  tests/test_exact_inputs_cpu.py proves that on an emulation.

The shapes are the case tables of tests/test_planes_gpu.py (correlation: those with C a power of two); the kernel path
is selected with lib_option like there and named in the test id (path-case-regime).  The CPU side of every test asserts the
regime's condition (sum |a b| + |bias| <= 2^21 granules) before the GPU is asked anything.

The accumulating call of every data gradient (run_dgrad) applies a REAL leaky-ReLU derivative on [0, hi) — the activation field, the
np.float32 model and the comparators of tests/dgrad_epilogue.py — once from the fp32 activation and, on the operand-plane entries, once
from the activation's first plane."""
import functools

import numpy as np
import pytest
import torch

import dgrad_epilogue as D
import exact_inputs as E
from test_planes_gpu import (CONV_CASES, CORR_BWD_CASES, CORR_PL_CASES, DECONV_CASES, SPLITK_CASES, STREAMK_CASES, WGRAD_CASES,
                             lib_option, make_pt, planes_value, weight_planes)  # noqa: F401  (lib_option: fixture)

pytestmark = pytest.mark.gpu


def _flops(c):
    B, H, W, Cin, Cout, k, s = c[:7]
    return 2.0 * B * -(-H // s) * -(-W // s) * k * k * Cin * Cout


def _cid(c):
    return "x".join(str(int(v)) if not isinstance(v, dict) else "d%d_p%d_s%d" % (v['max_displacement'], v['pad'], v['stride_2']) for v in c)


def _set(lib_option, opts):
    for k, v in opts.items():
        lib_option(k, v)


def assert_exact(got, ref, what):
    """Bit-exact or a message that locates the loss: how many outputs, how far (in granules is up to the reader), where."""
    got = got.detach().cpu().double()
    if torch.equal(got, ref):
        return
    bad = got != ref
    idx = bad.nonzero()
    per_axis = [len(torch.unique(idx[:, d])) for d in range(idx.shape[1])]
    raise AssertionError("%s: %d of %d outputs (%d non-zero) differ from the exact result; max |diff| %.3g = 2^%.1f; first at %s (got %r, exact "
                         "%r); distinct indices per axis %s of shape %s" %
                         (what, bad.sum().item(), bad.numel(), (ref != 0).sum().item(), (got - ref).abs().max().item(),
                          np.log2((got - ref).abs().max().item()), idx[0].tolist(), got[tuple(idx[0])].item(),
                          ref[tuple(idx[0])].item(), per_axis, list(ref.shape)))


def assert_gpu_planes(pt, x, regime, side):
    """The operand planes the LIBRARY made (unflow_planes_from_f32 / unflow_weight_planes_batched): the three-plane operand of a
    regime has three non-zero planes wherever it is non-zero, the two-plane operands two, the +-1 operand one."""
    want = E.kinds(regime)[2 + side]
    if want is None:
        return
    pl = pt if isinstance(pt, torch.Tensor) else pt.pl
    if pl.shape[0] != 3:
        return
    C = x.shape[-1]
    n = ((pl[..., :C] & 0x7fff) != 0).sum(0).cpu()
    assert torch.equal(n, want * (x != 0).long()), (regime, side)


@functools.lru_cache(maxsize=8)
def _fwd_problem(regime, case, deconv):
    return E.conv_forward_problem(regime, *case, deconv=deconv)


@functools.lru_cache(maxsize=8)
def _dgrad_problem(regime, case, deconv):
    return E.conv_dgrad_problem(regime, *case, deconv=deconv)


@functools.lru_cache(maxsize=8)
def _wgrad_problem(regime, case, deconv):
    return E.conv_wgrad_problem(regime, *case, deconv=deconv)


def _leaky32(ref):
    v = ref.float()
    return torch.maximum(torch.tensor(0.1, dtype=torch.float32) * v, v).double()


def scaled_pt(x, dev, scale, extra=0):
    """fp16 planes of a GRADIENT tensor: they hold scale * value (a power of two), the consumers divide their sums."""
    from unflow_amd import _lib
    from unflow_amd._lib import check, cl, ptr, stream
    from unflow_amd.core import layers as L
    B, H, W, C = x.shape
    buf = L.PT.alloc((B, H, W, C + extra), dev, 1, scale=scale)
    buf.t[..., :C] = x.to(dev)
    pt = buf.sl(0, C) if extra else buf
    check(_lib.lib().unflow_planes_from_f32(ptr(pt.t), pt.t.stride(2), cl(B * H * W), C, min(L.round8(C), pt.pl.shape[-1]),
                                            _lib.planes_of(pt.pl, scale), stream()), "planes_from_f32")
    assert torch.equal(pt.pl[0, ..., :C].view(torch.float16).cpu().double(), x.double() * scale)
    return pt


def run_forward(regime, case, dev, P, deconv=False, leaky=False, entry='pl'):
    from unflow_amd.core import layers as L
    B, H, W, Cin, Cout, k, stride = case
    x, w, b, ref = _fwd_problem(regime, case, deconv)
    want = _leaky32(ref) if leaky else ref
    X = make_pt(x.float(), dev, P, extra=8)
    wd, w_dir, w_tr = weight_planes(w.float(), dev, P)
    assert_gpu_planes(X, x, regime, 0)
    assert_gpu_planes(w_dir, w.reshape(w_dir.shape[1], w_dir.shape[2], -1), regime, 1)
    Ho, Wo = (2 * H, 2 * W) if deconv else L.out_hw(H, W, stride)
    Y = L.PT.alloc((B, Ho, Wo, Cout + 8), dev, P)
    Y.t.fill_(7.0)
    Yv = Y.sl(0, Cout)
    bd = b.float().to(dev)
    if entry == 'pl' and deconv:
        L.deconv_fwd(X, wd, w_dir, bd, Yv, leaky)
    elif entry == 'pl':
        L.conv_fwd(X, wd, w_tr, bd, Yv, stride, leaky)
    elif deconv:
        L.conv2d_transpose_fwd(X.t, wd, bd, Yv.t, leaky)
    else:
        L.conv2d_fwd(X.t, wd, bd, Yv.t, stride, leaky)
    assert_exact(Yv.t, want, "forward %s" % regime)
    assert torch.all(Y.t[..., Cout:] == 7.0)                                  # neighbours of the written slice untouched
    if entry == 'pl' and Cout <= 4 and not deconv:                            # the flow heads (conv_igemm.hip) write no planes at all
        assert not Y.pl.any()
    elif entry == 'pl':                                                       # the output planes re-sum to the fp32 output
        got_pl = planes_value(Y.pl.cpu())[..., :Cout]
        if P == 3:
            assert torch.equal(got_pl, want)
        else:
            assert torch.equal(got_pl.float(), want.float().half().float())


def run_dgrad(regime, case, dev, P, deconv=False, entry='pl', scale=0.0, hi=None):
    """hi: end of the activated range [0, hi) — default the aligned half of the channels (a four-channel flow-head case passes 2)."""
    from unflow_amd.core import layers as L
    B, H, W, Cin, Cout, k, stride = case
    dz, w, ref = _dgrad_problem(regime, case, deconv)
    DZ = scaled_pt(dz.float(), dev, scale, extra=8) if scale else make_pt(dz.float(), dev, P, extra=8)
    wd, w_dir, w_tr = weight_planes(w.float(), dev, P)
    assert_gpu_planes(DZ, dz, regime, 0)
    g = E.gen('base', regime, case)
    base = E.ints((B, H, W, Cin), g, -3, 3) * E.GRANULE[regime]
    hi = Cin // 2 // 4 * 4 if hi is None else hi
    tiny = deconv and Cin == 2 and Cout == 2                                  # the 2 -> 2 conv_transpose refuses a derivative
    s = base + ref                                                            # |base + ref| stays below 2^22 granules: exact
    # a real derivative (tests/dgrad_epilogue.py): about half of the activations negative, the specials planted in channels 0, hi - 1, hi
    act, _, special = D.act_field((B, H, W, Cin), 0, hi, (regime, case))
    if not tiny:                                                              # (its activation is never passed)
        D.assert_conditions(act, s, 0, hi, "%s %s" % (regime, case))
    want = D.expected(s, D.slope_f32(act), 0, hi)                             # inside [0, hi): fl32((base + ref) * slope), one fp32 multiply
    A = make_pt(torch.from_numpy(act), dev, P) if entry == 'pl' else L.PT(torch.from_numpy(act).to(dev))

    def dest(fill):
        d = L.PT.alloc((B, H, W, Cin + 4), dev, P)
        d.t.fill_(3.0)
        d.pl.fill_(D.SENTINEL)                                                # planes: 'untouched' is not 'wrote zero'
        if fill:
            d.t[..., :Cin] = base.float().to(dev)
        return d, d.sl(0, Cin)
    (DX, v), (DX2, v2) = dest(False), dest(True)
    if entry == 'pl' and deconv:
        call = lambda d, **kw: L.deconv_bwd_data(DZ, wd, w_tr, d, **kw)                     # noqa: E731
    elif entry == 'pl':
        call = lambda d, **kw: L.conv_bwd_data(DZ, wd, w_dir, d, stride, **kw)              # noqa: E731
    elif deconv:
        call = lambda d, **kw: L.conv2d_transpose_bwd_data(DZ.t, wd, d.t, **kw)             # noqa: E731
    else:
        call = lambda d, **kw: L.conv2d_bwd_data(DZ.t, wd, d.t, stride, **kw)               # noqa: E731
    call(v, accumulate=False)
    call(v2, accumulate=True, **({} if tiny else dict(act_src=A.t, act_lo=0, act_hi=hi)))
    assert_exact(v.t, ref, "data gradient %s" % regime)
    D.assert_output(DX2.t, D.f32_exact(s) if tiny else want, Cin, 3.0, "accumulating data gradient %s, fp32 derivative" % regime)
    assert torch.all(DX.t[..., Cin:] == 3.0)
    if entry != 'pl':
        return
    # planes only for the activated range (final after this call): the exact split / the fp16 cast of the product
    D.assert_planes(DX2.pl, D.expected_planes(want, P), 0, hi, "accumulating data gradient %s, fp32 derivative" % regime)
    # the derivative from the first operand plane of an activation that has no fp32 copy: the reference is slope_bits of the plane bits
    # the kernel reads
    DX3, v3 = dest(True)
    if not deconv and (Cout <= 4 or (k == 1 and stride == 1 and Cout == 32)) and hi:   # the fp32-operand kernels of conv_igemm.hip (pointwise, flow heads) read no planes
        with pytest.raises(_lib_error()) as e:
            call(v3, accumulate=True, act_src=A, act_lo=0, act_hi=hi, act_planes=True)
        assert e.value.status == -7                                           # UNFLOW_ERR_UNSUPPORTED, nothing launched
        D.assert_output(DX3.t, D.f32_exact(base), Cin, 3.0, "refused call")
        return
    call(v3, accumulate=True, act_src=A, act_lo=0, act_hi=hi, act_planes=True)
    bits = A.pl[0, ..., :Cin].cpu().numpy()
    want3 = D.expected(s, D.slope_bits(bits), 0, hi)
    what = "accumulating data gradient %s, plane derivative" % regime
    D.assert_output(DX3.t, want3, Cin, 3.0, what)
    D.assert_planes(DX3.pl, D.expected_planes(want3, P), 0, hi, what)
    same = ~torch.from_numpy(special).to(dev)
    assert torch.equal(DX3.t[..., :Cin][same], DX2.t[..., :Cin][same]), "plane source != fp32 source away from the specials"


def _lib_error():
    from unflow_amd._lib import UnflowError
    return UnflowError


def run_wgrad(regime, case, dev, P, entry='pl', scale=0.0):
    from unflow_amd.core import layers as L
    B, H, W, Cin, Cout, k, stride, deconv = case
    if deconv:
        H, W = H // 2, W // 2                                                  # WGRAD_CASES give the conv_transpose OUTPUT size
    x, dz, ref = _wgrad_problem(regime, (B, H, W, Cin, Cout, k, stride), deconv)
    X = make_pt(x.float(), dev, P)
    DZ = scaled_pt(dz.float(), dev, scale) if scale else make_pt(dz.float(), dev, P)
    assert_gpu_planes(X, x, regime, 0)
    assert_gpu_planes(DZ, dz, regime, 1)
    guard = torch.full((ref.numel() + 128,), float('nan'), device=dev)        # every element must be written, and nothing beside them
    dw = guard[64:64 + ref.numel()].view(tuple(ref.shape))
    if entry == 'pl' and deconv:
        L.deconv_bwd_filter(X, DZ, dw)
    elif entry == 'pl':
        L.conv_bwd_filter(X, DZ, dw, stride)
    elif deconv:
        L.conv2d_transpose_bwd_filter(X.t, DZ.t, dw, None)
    else:
        L.conv2d_bwd_filter(X.t, DZ.t, dw, None, stride)
    assert_exact(dw, ref, "filter gradient %s" % regime)
    assert torch.isnan(guard[:64]).all() and torch.isnan(guard[64 + ref.numel():]).all()


# ----------------------------------------------------------------------------------------------------------------------------
# conv forward + data gradient, bf16 x 3: one entry per kernel path
# ----------------------------------------------------------------------------------------------------------------------------
LIGHT = 5e10           # flops of the layer: every case of the tables fits (conv3 at the step's shape: 4e10, its fp64 references take seconds)
_light = lambda cases: [c for c in cases if _flops(c) <= LIGHT]                # noqa: E731
_s2 = lambda cases: [c for c in cases if c[6] == 2]                           # noqa: E731
GATHER = dict(halo=0, gather_pp=0, streamk=0)
_s1 = lambda cases: [c for c in cases if c[6] == 1]                           # noqa: E731
FWD, DGRAD, BOTH = ('fwd',), ('dgrad',), ('fwd', 'dgrad')
CONV_PATHS = [
    # path id, options, cases, entry, the directions the path is about
    ("gather_halo0", GATHER, _light(CONV_CASES)[:11], 'pl', BOTH),                                       # plain gather kernel everywhere
    ("gather_pp2", dict(halo=0, gather_pp=2, streamk=0), [CONV_CASES[1], CONV_CASES[2], CONV_CASES[3], CONV_CASES[5]], 'pl', BOTH),
    ("halo_streamk0", dict(streamk=0, halo_s2=2), _s1(_light(CONV_CASES)[9:]), 'pl', BOTH),             # one-shot halo kernel, source stride 1
    ("streamk2", dict(streamk=2, halo_s2=2), _light(STREAMK_CASES), 'pl', BOTH),                         # persistent stream-K
    ("halo_s2_2", dict(streamk=0, halo_s2=2), _light(_s2(CONV_CASES)), 'pl', FWD),                        # forward of stride-2 layers: four ACCUMULATING parity classes
    ("dgrad_s2_parity_streamk0", dict(streamk=0), _light(_s2(CONV_CASES)), 'pl', DGRAD),                 # stride-2 data gradients: four parity classes, one-shot kernels
    ("dgrad_s2_parity", dict(), _light(_s2(CONV_CASES)), 'pl', DGRAD),                                   # ... under the default rules (stream-K where it pays)
    ("splitk_reduce", dict(), [SPLITK_CASES[3], CONV_CASES[6]], 'pl', BOTH),                             # 16 slices -> the reduce kernel
    ("pointwise_1x1", dict(), [c for c in CONV_CASES if c[5] == 1], 'pl', DGRAD),                        # 1 x 1: pointwise dgrad kernel
    ("inline_split", dict(), [CONV_CASES[2], CONV_CASES[5], CONV_CASES[9], CONV_CASES[10]], 'f32', BOTH),  # conv_igemm.hip: split in the kernel
    ("inline_split_gather", GATHER, [CONV_CASES[3], CONV_CASES[11]], 'f32', BOTH),
    ("conv_math_fp32", dict(conv_math_fp32=1), [CONV_CASES[3], CONV_CASES[9], CONV_CASES[11], CONV_CASES[16]], 'pl', BOTH),   # fp32 MFMA: exact too
]


def _conv_params(direction):
    """Flat (options, case, entry) list of one direction, sorted by case (like every flat list below): the problems cached by
    lru_cache are then reused by all paths of a case."""
    return sorted([pytest.param(opts, case, entry, id="%s-%s" % (name, _cid(case))) for name, opts, cases, entry, dirs in CONV_PATHS
                   if direction in dirs for case in cases], key=lambda p: _cid(p.values[1]))


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("opts,case,entry", _conv_params('fwd'))
def test_conv_forward_exact(opts, case, entry, regime, dev, lib_option):
    from unflow_amd import _lib
    _set(lib_option, opts)
    _lib.lib().unflow_debug_streamk_timeouts()
    run_forward(regime, case, dev, 3, entry=entry)
    assert _lib.lib().unflow_debug_streamk_timeouts() == 0


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("opts,case,entry", _conv_params('dgrad'))
def test_conv_data_gradient_exact(opts, case, entry, regime, dev, lib_option):
    from unflow_amd import _lib
    _set(lib_option, opts)
    _lib.lib().unflow_debug_streamk_timeouts()
    run_dgrad(regime, case, dev, 3, entry=entry)
    assert _lib.lib().unflow_debug_streamk_timeouts() == 0


@pytest.mark.parametrize("opts,case", [pytest.param(GATHER, CONV_CASES[9], id="gather"), pytest.param(dict(streamk=0), CONV_CASES[14], id="halo"),
                                        pytest.param(dict(streamk=2), CONV_CASES[14], id="streamk"),
                                        pytest.param(dict(streamk=0, halo_s2=2), CONV_CASES[16], id="halo_s2")])
def test_conv_forward_leaky_is_fp32_maximum_of_the_exact_value(opts, case, dev, lib_option):
    """Leaky ReLU on top of an exact v: the fp32 torch.maximum(0.1f v, v), bit for bit."""
    _set(lib_option, opts)
    for regime in ('A3', 'dense'):
        run_forward(regime, case, dev, 3, leaky=True)


# ----------------------------------------------------------------------------------------------------------------------------
# FlowNetC's first layer on its own kernel (conv_first.hip): rgb4 planes in, planes only out
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,leaky", [(r, False) for r in E.REGIMES3] + [('A3', True), ('dense', True)])
@pytest.mark.parametrize("direct", [1, 0], ids=["conv1_direct1", "conv1_direct0"])
@pytest.mark.parametrize("case", [(2, 64, 128), (1, 50, 76)], ids=_cid)
def test_conv_first_exact(case, direct, regime, leaky, dev, lib_option):
    import ctypes
    from unflow_amd import _lib
    from unflow_amd._lib import check, stream
    from unflow_amd.core import layers as L
    B, H, W = case
    Cout = 64
    x, w, b, _ = _fwd_problem(regime, (B, H, W, 4, Cout, 7, 2), False)
    x = x.clone()
    x[..., 3] = 0                                                             # rgb4: the fourth input channel is padding
    ref = E._conv_ref(x, w, b, 2, False)                                      # fewer products than the checked problem: still exact
    assert torch.equal(ref, ref.float().double())
    want = _leaky32(ref) if leaky else ref
    lib_option("conv1_direct", direct)
    X = L.PT(x.float().to(dev), torch.zeros(3, B, H, W, 4, dtype=torch.int16, device=dev))
    L.planes_from_f32(X.t, X.pl, C=4)
    assert_gpu_planes(X, x, regime, 0)
    wd = w.float().to(dev).contiguous()
    w_dir = torch.zeros(3, 7, 28, Cout, dtype=torch.int16, device=dev)
    w_tr = torch.zeros(3, 7, Cout, 32, dtype=torch.int16, device=dev)
    check(_lib.lib().unflow_weight_planes_batched(1, (ctypes.c_void_p * 1)(wd.data_ptr()), (ctypes.c_int * 1)(7), (ctypes.c_int * 1)(28),
                                                  (ctypes.c_int * 1)(Cout), (ctypes.c_void_p * 1)(w_dir.data_ptr()),
                                                  (ctypes.c_void_p * 1)(w_tr.data_ptr()), 3, stream()), "weight_planes")
    Ho, Wo = L.out_hw(H, W, 2)
    Y = L.PT.alloc((B, Ho, Wo, Cout), dev, 3)
    Y.pl.fill_(0x7fc0)                                                        # bf16 NaN: every plane element must be written
    L.conv_fwd(X, wd, w_tr, b.float().to(dev), Y, 2, leaky, planes_only=True)
    assert_exact(planes_value(Y.pl.cpu())[..., :Cout], want, "conv_first %s" % regime)


# ----------------------------------------------------------------------------------------------------------------------------
# conv_transpose: forward, data gradient, filter gradient; stream-K on and off
# ----------------------------------------------------------------------------------------------------------------------------
def _deconv7(c):
    B, H, W, Cin, Cout = c
    return (B, H, W, Cin, Cout, 4, 2)


DECONV_PARAMS = [pytest.param(sk, _deconv7(c), id="streamk%d-%s" % (sk, _cid(c))) for c in DECONV_CASES for sk in (0, 2)
                 if 2.0 * c[0] * c[1] * c[2] * 16 * c[3] * c[4] <= LIGHT]


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("sk,case", DECONV_PARAMS)
def test_deconv_exact(sk, case, regime, dev, lib_option):
    from unflow_amd import _lib
    lib_option("streamk", sk)
    lib_option("halo_s2", 2)
    _lib.lib().unflow_debug_streamk_timeouts()
    run_forward(regime, case, dev, 3, deconv=True)
    run_dgrad(regime, case, dev, 3, deconv=True)
    if sk == 0:                                                               # the filter gradient does not depend on streamk
        B, H, W, Cin, Cout = case[:5]
        run_wgrad(regime, (B, 2 * H, 2 * W, Cin, Cout, 4, 2, True), dev, 3)
    assert _lib.lib().unflow_debug_streamk_timeouts() == 0


def test_deconv_forward_leaky_and_inline_split(dev, lib_option):
    case = _deconv7(DECONV_CASES[3])
    for regime in ('A3', 'dense'):
        run_forward(regime, case, dev, 3, deconv=True, leaky=True)
        run_forward(regime, case, dev, 3, deconv=True, entry='f32')
        run_dgrad(regime, case, dev, 3, deconv=True, entry='f32')


# ----------------------------------------------------------------------------------------------------------------------------
# filter gradients
# ----------------------------------------------------------------------------------------------------------------------------
WGRAD_PATHS = [("dma1_pp1", dict(wgrad_dma=1, wgrad_pp=1)), ("dma1_pp0", dict(wgrad_dma=1, wgrad_pp=0)), ("dma1_pp3", dict(wgrad_dma=1, wgrad_pp=3)),
               ("dma0_pp0", dict(wgrad_dma=0, wgrad_pp=0)), ("dma0_pp3", dict(wgrad_dma=0, wgrad_pp=3)),
               ("wgrad_math_fp32", dict(wgrad_math_fp32=1))]
WGRAD_EXACT_CASES = WGRAD_CASES + [(2, 24, 32, 64, 128, 5, 2, False), (2, 12, 16, 256, 32, 1, 1, False)]


@pytest.mark.parametrize("path", [pytest.param(o, id=n) for n, o in WGRAD_PATHS])
@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("case", WGRAD_EXACT_CASES, ids=_cid)
def test_filter_gradient_exact(case, regime, path, dev, lib_option):
    _set(lib_option, path)
    run_wgrad(regime, case, dev, 3)


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("case", [WGRAD_CASES[4], (2, 24, 32, 64, 128, 5, 2, False)], ids=_cid)
def test_filter_gradient_inline_split_exact(case, regime, dev):
    run_wgrad(regime, case, dev, 3, entry='f32')


# Cout = 2 flow heads (3 x 3, C -> 2; the engine pads their input channels to a multiple of 4: 1026 -> 1028, 194 -> 196, 98 -> 100) and
# their 2 -> 2 upsamplers
HEAD_CASES = [(2, 12, 16, 1028, 2, 3, 1, False), (2, 24, 32, 196, 2, 3, 1, False), (1, 48, 64, 100, 2, 3, 1, False), (2, 48, 64, 2, 2, 4, 2, True)]


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("case", HEAD_CASES, ids=_cid)
def test_flow_head_filter_gradient_exact(case, regime, dev):
    run_wgrad(regime, case, dev, 3)


@pytest.mark.parametrize("regime", E.REGIMES3)
def test_flow_wgrad_batched_exact(regime, dev):
    """unflow_flow_wgrad_batched: all Cout = 2 filter gradients of a decoder in one batch."""
    from unflow_amd.core import layers as L
    jobs, refs = [], []
    for case in HEAD_CASES:
        B, H, W, Cin, Cout, k, stride, deconv = case
        if deconv:
            H, W = H // 2, W // 2
        x, dz, ref = E.conv_wgrad_problem(regime, B, H, W, Cin, Cout, k, stride, deconv)
        dw = torch.full(tuple(ref.shape), float('nan'), device=dev)
        jobs.append(('deconv' if deconv else 'conv', x.float().to(dev), dz.float().to(dev), dw))
        refs.append(ref)
    L.flow_wgrad_batched(jobs)
    for j, ref in zip(jobs, refs):
        assert_exact(j[3], ref, "flow_wgrad_batched %s %s" % (j[0], regime))


# ----------------------------------------------------------------------------------------------------------------------------
# fp16 (n_planes = 1)
# ----------------------------------------------------------------------------------------------------------------------------
F16_HALO = [(2, 48, 64, 128, 128, 3, 1), (1, 16, 32, 388, 64, 3, 1), (1, 38, 70, 40, 96, 3, 2), (2, 8, 32, 256, 256, 3, 1), (1, 12, 16, 476, 256, 3, 1)]
F16_TALL = [(1, 12, 16, 476, 256, 3, 1), (1, 10, 40, 388, 160, 3, 1), (1, 38, 70, 136, 264, 3, 2), (2, 8, 32, 256, 256, 3, 1)]
F16_PATHS = [("f16_halo", dict(f16_k64=0, halo_s2=2), F16_HALO), ("f16_k64_2", dict(f16_k64=2, halo_s2=2), F16_HALO),
             ("f16_tall2", dict(f16_tall=2, f16_db=0, f16_k64=0, halo_s2=2), F16_TALL),
             ("f16_tall2_db1", dict(f16_tall=2, f16_db=1, f16_k64=0, halo_s2=2), F16_TALL[:2]),
             ("f16_db1", dict(f16_db=1, f16_k64=0, halo_s2=2), F16_HALO), ("f16_gather", dict(halo=0), [CONV_CASES[9], CONV_CASES[5]])]
F16_PARAMS = sorted([pytest.param(opts, case, id="%s-%s" % (name, _cid(case))) for name, opts, cases in F16_PATHS for case in cases],
                    key=lambda p: _cid(p.values[1]))
GRAD_SCALE = 4096.0     # the engine's power-of-two scale of fp16 gradient planes


@pytest.mark.parametrize("regime", E.REGIMES1)
@pytest.mark.parametrize("opts,case", F16_PARAMS)
def test_f16_forward_and_data_gradient_exact(opts, case, regime, dev, lib_option):
    _set(lib_option, opts)
    run_forward(regime, case, dev, 1)
    run_dgrad(regime, case, dev, 1, scale=GRAD_SCALE)


@pytest.mark.parametrize("case", [_deconv7(DECONV_CASES[3]), _deconv7(DECONV_CASES[6])], ids=_cid)
@pytest.mark.parametrize("regime", E.REGIMES1)
@pytest.mark.parametrize("k64", [0, 2], ids=["f16_k64_0", "f16_k64_2"])
def test_f16_deconv_exact(k64, regime, case, dev, lib_option):
    lib_option("f16_k64", k64)
    run_forward(regime, case, dev, 1, deconv=True)
    run_dgrad(regime, case, dev, 1, deconv=True, scale=GRAD_SCALE)


def test_f16_forward_leaky(dev, lib_option):
    lib_option("halo_s2", 2)
    run_forward('f16', F16_HALO[1], dev, 1, leaky=True)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["f16_wgrad_dma0", "f16_wgrad_dma1", "f16_wgrad_dma2_pp3"])
@pytest.mark.parametrize("regime", E.REGIMES1)
@pytest.mark.parametrize("case", WGRAD_EXACT_CASES[1:6], ids=_cid)
def test_f16_filter_gradient_exact(case, regime, mode, dev, lib_option):
    lib_option("f16_wgrad_dma", mode)
    if mode == 2:
        lib_option("wgrad_pp", 3)
    run_wgrad(regime, case, dev, 1, scale=GRAD_SCALE)


# ----------------------------------------------------------------------------------------------------------------------------
# correlation
# ----------------------------------------------------------------------------------------------------------------------------
def _pow2(c):
    return c & (c - 1) == 0


# C a power of two (the 1 / C scale is exact); the step's 8 x 256 x 48 x 64 cost volume (fp64 reference: 441 passes over 6 M elements,
# twice) runs on the default path only
# CORR_PL_CASES stops at C = 256: one C = 512 case of this file's own (two 256-channel K passes)
CORR_EXACT = [c for c in CORR_PL_CASES if _pow2(c[1]) and c[0] * c[1] * c[2] * c[3] < 2e6] + \
    [(2, 512, 6, 33, dict(kernel_size=1, max_displacement=8, pad=8, stride_1=1, stride_2=2))]
_rs = [c for c in CORR_EXACT if c[4]['stride_2'] == 1 and c[4]['max_displacement'] <= 4 and c[3] > 32]
_narrow = [c for c in CORR_EXACT if c[4]['max_displacement'] // c[4]['stride_2'] <= 6]
_wide = [c for c in CORR_EXACT if c[4]['max_displacement'] // c[4]['stride_2'] > 6]
CORR_FWD_PATHS = [("default", dict(), CORR_PL_CASES[:1] + CORR_EXACT), ("corr_rs0", dict(corr_rs=0), _rs), ("corr_rs1", dict(corr_rs=1), _rs),
                  ("corr_rs2", dict(corr_rs=2), _rs),
                  ("corr_rs0_nb0", dict(corr_rs=0, corr_nb=0), _narrow), ("corr_nb0", dict(corr_nb=0), _narrow),
                  ("corr_rw0", dict(corr_rw=0), _wide), ("corr_rw0_wb0", dict(corr_rw=0, corr_wb=0), _wide), ("corr_wb0", dict(corr_wb=0), _wide),
                  ("corr_math_fp32", dict(corr_math_fp32=1), CORR_EXACT[:4])]
CORR_FWD_PARAMS = sorted([pytest.param(opts, case, id="%s-%s" % (name, _cid(case))) for name, opts, cases in CORR_FWD_PATHS for case in cases],
                         key=lambda p: _cid(p.values[1]))


@functools.lru_cache(maxsize=8)
def _corr_fwd_problem(regime, N, C, H, W, md, pad, s2):
    return E.corr_forward_problem(regime, N, C, H, W, md, pad, s2)


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("opts,case", CORR_FWD_PARAMS)
def test_correlation_forward_exact(opts, case, regime, dev, lib_option):
    """unflow_correlation_nhwc_fwd_pl (operand planes) and unflow_correlation_nhwc_fwd (fp32 in, split in registers): regime a on
    in0, regime b on in1 — two tensors, paired by pair_shift like the step's one."""
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr, stream
    _set(lib_option, opts)
    N, C, H, W, a = case
    B = N // 2
    md, pad, s2 = a['max_displacement'], a['pad'], a['stride_2']
    f0, f1, ref = _corr_fwd_problem(regime, N, C, H, W, md, pad, s2)
    F0 = make_pt(f0.float(), dev, 3, extra=8)
    F1 = make_pt(torch.roll(f1, B, 0).float(), dev, 3, extra=8)               # the kernel pairs sample n with (n + B) % N of in1
    assert_gpu_planes(F0, f0, regime, 0)
    assert_gpu_planes(F1, torch.roll(f1, B, 0), regime, 1)
    oc, oh, ow = ref.shape[3], ref.shape[1], ref.shape[2]
    for pl in (True, False):
        for extra in (3, 0):                                                  # into a concat buffer / a dense cost volume
            out = torch.zeros(N, oh, ow, oc + extra, device=dev)
            out[..., :oc] = float('nan')
            if pl:
                check(_lib.lib().unflow_correlation_nhwc_fwd_pl(ptr(F0.t), ptr(F1.t), F0.t.stride(2), _lib.planes_of(F0.pl), _lib.planes_of(F1.pl),
                                                                B, ptr(out), oc + extra, N, C, H, W, 1, md, pad, 1, s2, stream()), "corr_pl")
            else:
                check(_lib.lib().unflow_correlation_nhwc_fwd(ptr(F0.t), ptr(F1.t), F0.t.stride(2), B, ptr(out), oc + extra, N, C, H, W, 1, md,
                                                             pad, 1, s2, stream()), "corr")
            assert_exact(out[..., :oc], ref, "correlation forward %s planes=%s" % (regime, pl))
            if extra:
                assert out[..., oc:].abs().max().item() == 0


CORR_BWD_PATHS = [("default", dict(), CORR_BWD_CASES), ("planes0", dict(corr_bwd_planes=0), CORR_BWD_CASES[:8:2] + CORR_BWD_CASES[8:]),
                  ("share0", dict(corr_bwd_share=0), [c for c in CORR_BWD_CASES if c[1] % 256 == 0]),
                  ("b128_0", dict(corr_bwd_b128=0), CORR_BWD_CASES[1::2]), ("rot0", dict(corr_bwd_rot=0), CORR_BWD_CASES[::2]),
                  ("rot1", dict(corr_bwd_rot=1), CORR_BWD_CASES[1::2]), ("corr_math_fp32", dict(corr_math_fp32=1), CORR_BWD_CASES[:3])]
CORR_BWD_PARAMS = sorted([pytest.param(opts, case, id="%s-%s" % (name, _cid(case))) for name, opts, cases in CORR_BWD_PATHS for case in cases],
                         key=lambda p: _cid(p.values[1]))


@functools.lru_cache(maxsize=8)
def _corr_bwd_problem(regime, N, C, H, W, md, pad, s2):
    return E.corr_backward_problem(regime, N, C, H, W, md, pad, s2)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "separate"])
@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("opts,case", CORR_BWD_PARAMS)
def test_correlation_backward_exact(opts, case, regime, fused, dev, lib_option):
    """unflow_correlation_nhwc_bwd_pl, fused g0 + g1 and the two gradients apart: operand a = dout (split in registers), operand b =
    the features (planes)."""
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr, stream
    _set(lib_option, opts)
    B, C, H, W, md, s2 = case
    N = 2 * B
    dout, f, refs = _corr_bwd_problem(regime, N, C, H, W, md, md, s2)
    if fused:
        refs = (refs[0] + refs[1],)
    Fp = make_pt(f.float(), dev, 3)
    assert_gpu_planes(Fp, f, regime, 1)
    d = dout.float().to(dev)
    oc = d.shape[-1]
    ga = torch.full((N, H, W, C), float('nan'), device=dev)
    gb = torch.full((N, H, W, C), float('nan'), device=dev)
    check(_lib.lib().unflow_correlation_nhwc_bwd_pl(ptr(d), oc, ptr(Fp.t), ptr(Fp.t), Fp.t.stride(2), _lib.planes_of(Fp.pl), _lib.planes_of(Fp.pl), B,
                                                    ptr(ga), ptr(None if fused else gb), C, fused, N, C, H, W, 1, md, md, 1, s2, stream()),
          "correlation_bwd_pl")
    for got, ref, name in zip((ga, gb), refs, ("g0 + g1" if fused else "g0", "g1")):
        assert_exact(got, ref, "correlation backward %s %s" % (name, regime))
