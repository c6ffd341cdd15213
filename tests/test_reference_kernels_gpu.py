"""-m gpu: the reference's OWN GPU kernels (ops/*_op.cu.cc compiled unmodified for gfx950: oracle/_ref/libref_ops.so, built by
__graft_entry__.build() through oracle/Makefile, oracle/ref_shim/ and oracle/ref_glue.hip) run next to
  (a) the CPU oracle oracle/ops_ref.c — every other parity test of this suite goes back to it, and this is what pins it — and
  (b) the HIP ops of this library, directly, so that the comparison survives a later change of the oracle.

Cases, inputs, the exact fp64 values and the bound gamma = (n + 2) 2^-24 sum|terms| per element are tests/reference_pin.py's (its
docstring derives the bound; tests/test_reference_build_cpu.py checks its conditions without a GPU).  Every fp32 side must lie
within gamma of the fp64 value and any two fp32 sides within 2 gamma of each other, element by element, no element excluded.
Kernels that form their products from bf16 x 3 operands (the plane path, and the default backward of the fp32-operand entry) are
not fp32 sums of the same products: they are held to the suite's bound for them, assert_fp32_class of tests/test_planes_gpu.py.

The library is loaded with ctypes after torch and after unflow_amd._lib.lib(): one HIP runtime in the process.  Nothing here
reads the reference checkout.  A missing library is a failure, not a skip."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import reference_pin as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ops.so")
UNSUPPORTED = -7
_P, _L, _I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int


@pytest.fixture(scope="module")
def reflib(dev):
    from unflow_amd import _lib
    _lib.lib()                                       # torch, then the library: the HIP runtime both bind to is loaded
    if not os.path.exists(REF_SO):
        pytest.fail("%s is missing: __graft_entry__.build() makes it where the reference checkout is present; the tree that "
                    "runs on the GPU must carry the built library" % REF_SO)
    L = ctypes.CDLL(REF_SO)
    L.ref_glue_correlation.argtypes = [_P] * 5 + [_L] * 2 + [_I] * 9 + [ctypes.POINTER(ctypes.c_int)]
    L.ref_glue_correlation_grad.argtypes = [_P] * 5 + [_L] * 3 + [_I] * 9
    L.ref_glue_backward_warp.argtypes = [_P] * 3 + [_L] * 2 + [_I] * 4
    L.ref_glue_backward_warp_grad.argtypes = [_P] * 4 + [_L] * 2 + [_I] * 4
    L.ref_glue_forward_warp.argtypes = [_P] * 2 + [_L] * 2 + [_I] * 3
    L.ref_glue_forward_warp_grad.argtypes = [_P] * 3 + [_L] * 2 + [_I] * 3
    L.ref_glue_downsample.argtypes = [_P] * 2 + [_L] * 2 + [_I] * 5
    return L


@pytest.fixture
def lib_option():
    """Set library options (csrc/options.h) for one test; restored afterwards."""
    from unflow_amd import _lib
    saved = {}

    def setter(name, value):
        saved.setdefault(name, _lib.get_option(name))
        _lib.set_option(name, value)
    yield setter
    for k, v in saved.items():
        _lib.set_option(k, v)


def dt(a, dev):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def tt(a):
    return torch.tensor(np.ascontiguousarray(a))


def dp(t):
    return ctypes.c_void_p(t.data_ptr())


def host(t):
    return t.detach().cpu().numpy()


def launched(status):
    """Status of a glue call that must have run.  A HIP error (-5: a fault of a reference kernel) ends the whole session: nothing
    more is started on a GPU that has faulted."""
    if status == -5:
        pytest.exit("the HIP runtime reported an error after a reference kernel", returncode=3)
    assert status == 0, status


def nan_like(shape, dev):
    return torch.full(tuple(shape), float("nan"), device=dev)


# ---------------------------------------------------------------- the reference kernels
def ref_corr_shape(reflib, case):
    N, C, H, W, k, md, pad, s1, s2 = case
    s5 = (ctypes.c_int * 5)()
    assert reflib.ref_glue_correlation(None, None, None, None, None, 0, 0, N, C, H, W, k, md, pad, s1, s2, s5) == 0
    return tuple(s5)


def ref_correlation(reflib, dev, in0, in1, dout, case):
    """The reference's Correlation (twice: is it bit-stable?) and CorrelationGrad -> out, grad0, grad1 (numpy NCHW), stable."""
    N, C, H, W, k, md, pad, s1, s2 = case
    oc, oh, ow, ph, pw = ref_corr_shape(reflib, case)
    a, b = dt(in0, dev), dt(in1, dev)
    outs = []
    for _ in range(2):
        out = nan_like((N, oc, oh, ow), dev)
        p0, p1 = nan_like((N, ph, pw, C), dev), nan_like((N, ph, pw, C), dev)
        st = reflib.ref_glue_correlation(dp(a), dp(b), dp(out), dp(p0), dp(p1), out.numel(), p0.numel(), N, C, H, W, k, md, pad,
                                         s1, s2, None)
        launched(st)
        outs.append(host(out))
    res = {"out": outs[0], "stable": bool(np.array_equal(outs[0], outs[1]))}
    if dout is not None:
        d = dt(dout, dev)
        g0, g1 = nan_like(a.shape, dev), nan_like(a.shape, dev)
        st = reflib.ref_glue_correlation_grad(dp(d), dp(p0), dp(p1), dp(g0), dp(g1), d.numel(), p0.numel(), g0.numel(), N, C, H, W,
                                              k, md, pad, s1, s2)
        launched(st)
        res["grad0"], res["grad1"] = host(g0), host(g1)
    return res


_REF = {}


def ref_case(reflib, dev, idx):
    """The reference's outputs of a case, computed once and shared."""
    if idx not in _REF:
        _REF[idx] = ref_correlation(reflib, dev, *R.corr_inputs(idx), R.CORR_CASES[idx])
        for a in _REF[idx].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[idx]


# ---------------------------------------------------------------- the HIP entries
def hip_corr_fp32(dev, in0, in1, dout, case):
    """unflow_correlation_fwd / _bwd (NCHW) with the fp32 part of the workspace alone: the fp32-operand kernels.  None when the
    entry reports UNFLOW_ERR_UNSUPPORTED for the attributes."""
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr, stream
    L = _lib.lib()
    N, C, H, W, k, md, pad, s1, s2 = case
    o3 = (ctypes.c_int * 3)()
    st = L.unflow_correlation_out_shape(H, W, k, md, pad, s1, s2, o3)
    if st == UNSUPPORTED:
        return None
    check(st, "out_shape")
    oc, oh, ow = tuple(o3)
    nbytes = (4 * in0.size + N * oc * oh * ow) * 4
    ws = torch.zeros(nbytes // 4 + 64, device=dev)
    a, b = dt(in0, dev), dt(in1, dev)
    out = nan_like((N, oc, oh, ow), dev)
    st = L.unflow_correlation_fwd(ptr(a), ptr(b), ptr(out), N, C, H, W, k, md, pad, s1, s2, ptr(ws), _lib.csz(nbytes), stream())
    if st == UNSUPPORTED:
        return None
    check(st, "correlation_fwd")
    res = {"out": host(out)}
    if dout is not None:
        g0, g1 = nan_like(a.shape, dev), nan_like(a.shape, dev)
        check(L.unflow_correlation_bwd(ptr(dt(dout, dev)), ptr(a), ptr(b), ptr(g0), ptr(g1), N, C, H, W, k, md, pad, s1, s2, ptr(ws),
                                       _lib.csz(nbytes), stream()), "correlation_bwd")
        res["grad0"], res["grad1"] = host(g0), host(g1)
    return res


def plane_path_takes(case):
    """unflow_correlation_nhwc_fwd_pl's own condition (include/unflow_hip.h): kernel_size 1, stride_1 1, C % 16 == 0."""
    N, C, H, W, k, md, pad, s1, s2 = case
    return k == 1 and s1 == 1 and C % 16 == 0


def hip_corr_planes(dev, in0, in1, dout, case):
    """unflow_correlation_nhwc_fwd_pl / _bwd_pl on bf16 x 3 operand planes of two independent tensors (pair_shift 0), default
    options -> out, grad0, grad1 as numpy NCHW."""
    from test_planes_gpu import make_pt
    from unflow_amd import _lib
    from unflow_amd._lib import check, ptr, stream
    L = _lib.lib()
    N, C, H, W, k, md, pad, s1, s2 = case
    oc, oh, ow = R.corr_geometry(H, W, k, md, pad, s1, s2)[:3]
    F0 = make_pt(torch.from_numpy(np.ascontiguousarray(in0.transpose(0, 2, 3, 1))), dev, 3)
    F1 = make_pt(torch.from_numpy(np.ascontiguousarray(in1.transpose(0, 2, 3, 1))), dev, 3)
    out = nan_like((N, oh, ow, oc), dev)
    check(L.unflow_correlation_nhwc_fwd_pl(ptr(F0.t), ptr(F1.t), F0.t.stride(2), _lib.planes_of(F0.pl), _lib.planes_of(F1.pl), 0,
                                           ptr(out), oc, N, C, H, W, k, md, pad, s1, s2, stream()), "correlation_fwd_pl")
    res = {"out": host(out).transpose(0, 3, 1, 2)}
    if dout is not None:
        d = dt(dout.transpose(0, 2, 3, 1), dev)
        g0, g1 = nan_like((N, H, W, C), dev), nan_like((N, H, W, C), dev)
        check(L.unflow_correlation_nhwc_bwd_pl(ptr(d), oc, ptr(F0.t), ptr(F1.t), F0.t.stride(2), _lib.planes_of(F0.pl),
                                               _lib.planes_of(F1.pl), 0, ptr(g0), ptr(g1), C, 0, N, C, H, W, k, md, pad, s1, s2,
                                               stream()), "correlation_bwd_pl")
        res["grad0"], res["grad1"] = host(g0).transpose(0, 3, 1, 2), host(g1).transpose(0, 3, 1, 2)
    return res


@functools.lru_cache(maxsize=None)
def plain_fp32(idx):
    """The plain-fp32 side of assert_fp32_class: torch's CPU fp32 evaluation of the same sums (tests/exact_inputs.py, NHWC)."""
    import exact_inputs as E
    N, C, H, W, k, md, pad, s1, s2 = R.CORR_CASES[idx]
    f0, f1, d = (torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))) for x in R.corr_inputs(idx))
    g0, g1 = E.corr_backward_ref(d, f0, f1, md, pad, s2)
    return {"out": E.corr_forward_ref(f0, f1, md, pad, s2).permute(0, 3, 1, 2), "grad0": g0.permute(0, 3, 1, 2),
            "grad1": g1.permute(0, 3, 1, 2)}


def nonzero_sites(a):
    return [tuple(int(i) for i in s) for s in np.argwhere(np.asarray(a) != 0)]


# ---------------------------------------------------------------- the glue refuses what does not fit, before any launch
def test_glue_refuses_wrong_sizes_and_geometry(reflib, dev):
    """Every call here must come back with its status and launch nothing: the buffer stays as it was."""
    t = torch.zeros(1024, device=dev)
    case = (1, 2, 4, 4, 1, 1, 1, 1, 1)                                  # out [1, 9, 4, 4], padded [1, 6, 6, 2]
    assert ref_corr_shape(reflib, case) == (9, 4, 4, 6, 6)
    call = lambda oe, pe, *c: reflib.ref_glue_correlation(dp(t), dp(t), dp(t), dp(t), dp(t), oe, pe, *c, None)      # noqa: E731
    assert call(143, 72, *case) == -3 and call(144, 73, *case) == -3                      # buffer sizes against CorrelationState
    assert call(144, 72, 1, 2, 4, 4, 2, 1, 1, 1, 1) == -2                                  # even kernel
    assert call(144, 72, 0, 2, 4, 4, 1, 1, 1, 1, 1) == -2 and call(144, 72, 1, 2, 4, 4, 1, 1, 1, 0, 1) == -2
    assert call(144, 72, 1, 2, 4, 4, 1, 4, 1, 1, 1) == -2                                  # empty output
    assert reflib.ref_glue_correlation(None, dp(t), dp(t), dp(t), dp(t), 144, 72, *case, None) == -1
    grad = lambda *c: reflib.ref_glue_correlation_grad(dp(t), dp(t), dp(t), dp(t), dp(t), *c)                    # noqa: E731
    # pad < the displacement grid's reach: Backward0 / 1 would read before the padded buffer (forward alone stays inside)
    assert ref_corr_shape(reflib, (1, 1, 8, 8, 1, 2, 1, 1, 1))[:3] == (25, 6, 6)
    assert grad(900, 100, 64, 1, 1, 8, 8, 1, 2, 1, 1, 1) == -4
    assert grad(144, 72, 31, *case) == -3
    assert reflib.ref_glue_backward_warp(dp(t), dp(t), dp(t), 24, 15, 1, 2, 4, 3) == -3
    assert reflib.ref_glue_backward_warp(dp(t), dp(t), dp(t), 24, 16, 1, 2, 0, 3) == -2
    assert reflib.ref_glue_forward_warp(dp(t), dp(t), 16, 9, 1, 2, 4) == -3
    assert reflib.ref_glue_downsample(dp(t), dp(t), 48, 12, 1, 4, 4, 3, 3) == -2           # 4 is not divisible by 3
    assert reflib.ref_glue_downsample(dp(t), dp(t), 48, 11, 1, 4, 4, 3, 2) == -3
    assert torch.all(t == 0).item()


# ---------------------------------------------------------------- (a) oracle against the reference kernels
@pytest.mark.parametrize("idx", range(len(R.CORR_CASES)), ids=R.CORR_IDS)
def test_correlation_oracle_against_reference_kernels(idx, reflib, dev, oracle_lib):
    case, tag = R.CORR_CASES[idx], R.CORR_IDS[idx]
    in0, in1, dout = R.corr_inputs(idx)
    attrs = R.attrs_of(case)
    ex = R.corr_exact(idx)
    ref = ref_case(reflib, dev, idx)
    # the geometry is the reference's own (CorrelationState through the glue)
    assert ref_corr_shape(reflib, case)[:3] == oracle_lib.correlation_out_shape(case[2], case[3], **attrs) == ex["out"][0].shape[1:]
    print("REFPIN reference Correlation %s run twice: %s" % (tag, "bit-stable" if ref["stable"] else "NOT bit-stable"))
    orc = {"out": oracle_lib.correlation(in0, in1, **attrs)}
    orc["grad0"], orc["grad1"] = oracle_lib.correlation_grad(dout, in0, in1, **attrs)
    for what in ("out", "grad0", "grad1"):
        R.assert_within("reference correlation %s %s vs fp64" % (what, tag), ref[what], ex[what])
        R.assert_within("oracle    correlation %s %s vs fp64" % (what, tag), orc[what], ex[what])
        R.assert_within("|reference - oracle| correlation %s %s (bound 2 gamma)" % (what, tag), orc[what], ex[what], 2.0, ref[what])
        print("REFPIN |reference - oracle| / gamma correlation %s %s = %.4f" %
              (what, tag, R.ratio_to_bound(orc[what], ref[what], R.gamma(ex[what][2], ex[what][1]))))


# ---------------------------------------------------------------- (b) HIP ops against the reference kernels
@pytest.mark.parametrize("math", ["default", "corr_math_fp32"])
@pytest.mark.parametrize("idx", range(len(R.CORR_CASES)), ids=R.CORR_IDS)
def test_correlation_hip_fp32_entry_against_reference_kernels(idx, math, reflib, dev, lib_option):
    """unflow_correlation_fwd / unflow_correlation_bwd, fp32-operand kernels.  With the default options the backward of the
    C % 32 == 0 shapes forms its products from a bf16 x 3 split in registers (corr_bwd_b3_kernel): those gradients are held to
    assert_fp32_class; with corr_math_fp32 = 1 every kernel is an fp32 sum and is held to gamma."""
    from test_planes_gpu import assert_fp32_class
    case, tag = R.CORR_CASES[idx], R.CORR_IDS[idx]
    if math == "corr_math_fp32":
        lib_option("corr_math_fp32", 1)
    in0, in1, dout = R.corr_inputs(idx)
    ex = R.corr_exact(idx)
    ref = ref_case(reflib, dev, idx)
    hip = hip_corr_fp32(dev, in0, in1, dout, case)
    assert hip is not None, "UNFLOW_ERR_UNSUPPORTED"          # every attribute set of these cases is accepted today
    N, C, H, W, k, s1 = case[0], case[1], case[2], case[3], case[4], case[7]
    split_bwd = math == "default" and k == 1 and s1 == 1 and C % 32 == 0
    for what in ("out", "grad0", "grad1"):
        assert hip[what].shape == ref[what].shape
        if what != "out" and split_bwd:
            p32 = plain_fp32(idx)
            assert_fp32_class(tt(hip[what]), tt(ex[what][0]), p32[what], "hip fp32-operand entry, bf16 x 3 backward: %s %s" % (what, tag))
            print("REFPIN hip fp32-operand entry, bf16 x 3 backward %s %s: |diff| / gamma = %.4f (not asserted)" %
                  (what, tag, R.ratio_to_bound(hip[what], ex[what][0], R.gamma(ex[what][2], ex[what][1]))))
            continue
        R.assert_within("hip fp32 (%s) correlation %s %s vs fp64" % (math, what, tag), hip[what], ex[what])
        R.assert_within("|hip fp32 (%s) - reference| correlation %s %s (bound 2 gamma)" % (math, what, tag), hip[what], ex[what],
                        2.0, ref[what])


@pytest.mark.parametrize("idx", [i for i, c in enumerate(R.CORR_CASES) if plane_path_takes(c)],
                         ids=[t for t, c in zip(R.CORR_IDS, R.CORR_CASES) if plane_path_takes(c)])
def test_correlation_hip_plane_entry_against_reference_kernels(idx, reflib, dev):
    """unflow_correlation_nhwc_fwd_pl / _bwd_pl, default options, in0 and in1 two independent tensors: rms error against fp64 at
    most FP32_CLASS x that of the plain fp32 evaluation — and, next to it, the reference kernels' own rms error by the same measure
    (they ARE a plain fp32 evaluation)."""
    from test_planes_gpu import assert_fp32_class
    case, tag = R.CORR_CASES[idx], R.CORR_IDS[idx]
    in0, in1, dout = R.corr_inputs(idx)
    ex = R.corr_exact(idx)
    ref = ref_case(reflib, dev, idx)
    p32 = plain_fp32(idx)
    hip = hip_corr_planes(dev, in0, in1, dout, case)
    for what in ("out", "grad0", "grad1"):
        assert hip[what].shape == ref[what].shape and np.all(np.isfinite(hip[what]))
        v = tt(ex[what][0])
        assert_fp32_class(tt(hip[what]), v, p32[what], "hip planes %s %s" % (what, tag))
        assert_fp32_class(tt(ref[what]), v, p32[what], "reference kernels %s %s" % (what, tag))


def test_one_hot_pair_lights_the_same_channel_and_site_everywhere(reflib, dev, oracle_lib):
    """One non-zero pixel per input of the 441-channel case: in0[1, 5, 7, 9] = 2, in1[1, 5, 1, 17] = 3, a displacement of
    (dy, dx) = (-6, +8).  Every implementation must light exactly one output element, the same one, with the value 6 / 96.  The
    reference kernels put it in channel 161 = (dy / 2 + 10) * 21 + (dx / 2 + 10) — the x displacement runs fastest — at site
    (7, 9) of sample 1 (recorded from the reference's own kernel on an MI355X)."""
    case = R.CORR_CASES[R.ONE_HOT_CASE]
    a, b = R.corr_one_hot_inputs()
    ex = R.corr_exact_fwd(a, b, *case[4:])
    sides = {"reference": ref_correlation(reflib, dev, a, b, None, case)["out"],
             "oracle": oracle_lib.correlation(a, b, **R.attrs_of(case)),
             "hip fp32": hip_corr_fp32(dev, a, b, None, case)["out"],
             "hip planes": hip_corr_planes(dev, a, b, None, case)["out"],
             "fp64": ex[0]}
    lit = {name: nonzero_sites(out) for name, out in sides.items()}
    print("REFPIN one-hot 441: %s" % lit)
    for name, sites in lit.items():
        assert len(sites) == 1, (name, sites[:5])
        assert sites == lit["reference"], (name, sites, lit["reference"])
        assert abs(float(sides[name][sites[0]]) - 6.0 / 96.0) <= R.gamma(96, 6.0 / 96.0), (name, sides[name][sites[0]])
    assert lit["reference"] == [(1, 161, 7, 9)]


# ---------------------------------------------------------------- warps and downsample
def ref_warps(reflib, dev, size, C):
    B, H, W = size
    im, flow, dout = (dt(x, dev) for x in R.warp_inputs(size, C))
    res = {}
    out, dfl = nan_like(im.shape, dev), nan_like(flow.shape, dev)
    launched(reflib.ref_glue_backward_warp(dp(im), dp(flow), dp(out), im.numel(), flow.numel(), B, H, W, C))
    launched(reflib.ref_glue_backward_warp_grad(dp(dout), dp(im), dp(flow), dp(dfl), im.numel(), flow.numel(), B, H, W, C))
    res["backward_warp"] = {"out": host(out), "d_flow": host(dfl)}
    if C == 1:
        out, dfl = nan_like((B, H, W, 1), dev), nan_like(flow.shape, dev)
        launched(reflib.ref_glue_forward_warp(dp(flow), dp(out), flow.numel(), out.numel(), B, H, W))
        launched(reflib.ref_glue_forward_warp_grad(dp(dout), dp(flow), dp(dfl), dout.numel(), flow.numel(), B, H, W))
        res["forward_warp"] = {"out": host(out), "d_flow": host(dfl)}
    return res


def oracle_warps(oracle_lib, size, C):
    im, flow, dout = R.warp_inputs(size, C)
    res = {"backward_warp": {"out": oracle_lib.backward_warp(im, flow), "d_flow": oracle_lib.backward_warp_grad(dout, im, flow)}}
    if C == 1:
        res["forward_warp"] = {"out": oracle_lib.forward_warp(flow), "d_flow": oracle_lib.forward_warp_grad(dout, flow)}
    return res


def hip_warps(dev, size, C):
    from unflow_amd import ops
    im, flow, dout = (dt(x, dev) for x in R.warp_inputs(size, C))
    fl = flow.clone().requires_grad_()
    out = ops.backward_warp(im, fl)
    out.backward(dout)
    res = {"backward_warp": {"out": host(out), "d_flow": host(fl.grad)}}
    if C == 1:
        for det in (False, True):
            fl = flow.clone().requires_grad_()
            out = ops.forward_warp(fl, deterministic=det)
            out.backward(dout)
            res["forward_warp_det" if det else "forward_warp"] = {"out": host(out), "d_flow": host(fl.grad)}
    return res


@pytest.mark.parametrize("C", R.WARP_CHANNELS)
@pytest.mark.parametrize("size", R.WARP_SIZES, ids=str)
def test_warps_oracle_and_hip_against_reference_kernels(size, C, reflib, dev, oracle_lib):
    """backward_warp and its flow gradient (C = 1, 3), forward_warp's splat and its gradient (with C = 1): reference kernels,
    oracle and HIP ops each within gamma of fp64, pairwise within 2 gamma.  forward_warp adds with float atomics in the reference
    and in the HIP op's non-deterministic mode: never compared bitwise.  The HIP op's deterministic mode sums its terms as
    integers of 2^-31 (each term rounded to that grid once): its bound is gamma + n 2^-31."""
    ex = R.warp_exact(size, C)
    ref, orc, hip = ref_warps(reflib, dev, size, C), oracle_warps(oracle_lib, size, C), hip_warps(dev, size, C)
    for op in ref:
        for what in ("out", "d_flow"):
            tag = "%s %s %s C%d" % (op, what, size, C)
            e = ex[op][what]
            R.assert_within("reference %s vs fp64" % tag, ref[op][what], e)
            R.assert_within("oracle    %s vs fp64" % tag, orc[op][what], e)
            R.assert_within("hip       %s vs fp64" % tag, hip[op][what], e)
            R.assert_within("|reference - oracle| %s (bound 2 gamma)" % tag, orc[op][what], e, 2.0, ref[op][what])
            R.assert_within("|reference - hip|    %s (bound 2 gamma)" % tag, hip[op][what], e, 2.0, ref[op][what])
            print("REFPIN |reference - oracle| / gamma %s = %.4f" % (tag, R.ratio_to_bound(orc[op][what], ref[op][what], R.gamma(e[2], e[1]))))
    if C == 1:
        v, S, n = ex["forward_warp"]["out"]
        got = hip["forward_warp_det"]["out"]
        ratio = R.ratio_to_bound(got, v, R.gamma(n, S) + n * 2.0 ** -31)
        print("REFPIN hip forward_warp deterministic out %s: worst |diff| / (gamma + n 2^-31) = %.4f" % (size, ratio))
        assert ratio <= 1.0
        # the gradient kernel does not depend on the mode
        assert np.array_equal(hip["forward_warp_det"]["d_flow"], hip["forward_warp"]["d_flow"])


@pytest.mark.parametrize("scale", R.DOWNSAMPLE_SCALES)
def test_downsample_oracle_and_hip_against_reference_kernels(scale, reflib, dev, oracle_lib):
    from unflow_amd import ops
    for shape in R.DOWNSAMPLE_SHAPES:
        B, H, W, C = shape
        im = R.ds_inputs(shape)
        e = R.ds_exact(im, scale)
        tim = dt(im, dev)
        out = nan_like((B, H // scale, W // scale, C), dev)
        launched(reflib.ref_glue_downsample(dp(tim), dp(out), tim.numel(), out.numel(), B, H, W, C, scale))
        ref, orc, hip = host(out), oracle_lib.downsample(im, scale), host(ops.downsample(tim, scale))
        tag = "downsample %s / %d" % (shape, scale)
        for name, got in (("reference", ref), ("oracle", orc), ("hip", hip)):
            R.assert_within("%-9s %s vs fp64" % (name, tag), got, e)
        R.assert_within("|reference - oracle| %s (bound 2 gamma)" % tag, orc, e, 2.0, ref)
        R.assert_within("|reference - hip|    %s (bound 2 gamma)" % tag, hip, e, 2.0, ref)
        print("REFPIN |reference - oracle| / gamma %s = %.4f" % (tag, R.ratio_to_bound(orc, ref, R.gamma(e[2], e[1]))))
