"""The exact-input regimes of tests/exact_inputs.py have teeth — proven without a GPU on a torch emulation of the kernels' arithmetic
(three bf16 planes, six product terms, fp32 accumulation per term and per K tile of 32): with every term in place the emulation
equals the fp64 reference bit for bit in every regime; with any single term removed it differs on more than half of the non-zero
outputs of the regime built for that term; with one tap or one K tile removed the dense regime differs.  Guards the generators
against later edits: a regime that stopped exposing its terms would fail here, not silently pass on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E

# a small layer with an M tail, a K tail (9 * 20 = 180 = 5.6 K tiles) and the three conv forms
CONV = (2, 9, 11, 20, 24, 3, 1)
CONV_S2 = (1, 12, 14, 12, 16, 5, 2)
DECONV = (1, 5, 6, 24, 16, 4, 2)


def _im2col(x, w, stride):
    """The GEMM of a SAME conv: a [sites, taps * Cin] (tap-major), b [taps * Cin, Cout]."""
    from oracle import model_ref as M
    B, H, W, Cin = x.shape
    k = w.shape[0]
    pt, pb = M.same_pads(H, k, stride)
    pl, pr = M.same_pads(W, k, stride)
    cols = F.unfold(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), k, stride=stride)          # [B, Cin * k * k, L]
    a = cols.reshape(B, Cin, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * Cin)
    return a, w.reshape(k * k * Cin, -1)


def _mismatch(got, ref):
    nz = ref != 0
    return ((got.double() != ref) & nz).sum().item() / max(nz.sum().item(), 1)


@pytest.mark.parametrize("regime", E.REGIMES3)
@pytest.mark.parametrize("case", [CONV, CONV_S2])
def test_emulated_six_terms_equal_fp64_and_every_lost_term_shows(case, regime):
    x, w, b, ref = E.conv_forward_problem(regime, *case)
    a, bm = _im2col(x, w, case[6])
    ref2 = ref.reshape(-1, case[4]) - b
    assert torch.equal(a @ bm, ref2)                                          # the GEMM view is the same problem
    assert torch.equal(E.emulated_gemm(a, bm).double(), ref2)
    assert _mismatch(E.emulated_gemm(a, bm, drop=((0, 0),)), ref2) > 0.5      # hi * hi: visible in every regime
    for term in E.EXPOSES.get(regime, ()):
        frac = _mismatch(E.emulated_gemm(a, bm, drop=(term,)), ref2)
        print(case, regime, "term", term, "dropped: mismatch on %.0f %% of the non-zero outputs" % (100 * frac))
        assert frac > 0.5, (regime, term, frac)
    if regime != 'dense':      # the terms over planes a regime leaves empty are exactly zero in it; every other one shows
        pa, pb = E.kinds(regime)[2:]
        empty = tuple(t for t in E.TERMS if t[0] >= pa or t[1] >= pb)
        assert torch.equal(E.emulated_gemm(a, bm, drop=empty).double(), ref2)
        for term in set(E.TERMS) - set(empty):
            assert _mismatch(E.emulated_gemm(a, bm, drop=(term,)), ref2) > 0.5, (regime, term)


def test_every_term_is_exposed_by_some_regime():
    seen = {(0, 0)}
    for r in E.EXPOSES.values():
        seen.update(r)
    assert seen == set(E.TERMS)


@pytest.mark.parametrize("case", [CONV, CONV_S2])
def test_dense_regime_sees_a_lost_tap_and_a_lost_k_tile(case):
    x, w, b, ref = E.conv_forward_problem('dense', *case)
    a, bm = _im2col(x, w, case[6])
    ref2 = ref.reshape(-1, case[4]) - b
    Cin, k = case[3], case[5]
    for tap in (0, k * k // 2, k * k - 1):
        rows = torch.arange(tap * Cin, (tap + 1) * Cin)
        assert _mismatch(E.emulated_gemm(a, bm, drop_rows=rows), ref2) > 0.5, tap
    K = a.shape[1]
    for k0 in (0, 32, K // 32 * 32):                                         # first, second and the partial last K tile
        rows = torch.arange(k0, min(k0 + 32, K))
        assert _mismatch(E.emulated_gemm(a, bm, drop_rows=rows), ref2) > 0.5, k0
    assert _mismatch(E.emulated_gemm(a, bm, drop_rows=torch.tensor([K - 1])), ref2) > 0.25   # one channel of the last tap


@pytest.mark.parametrize("regime", E.REGIMES1)
def test_fp16_regimes_are_exact_and_see_a_lost_k_tile(regime):
    x, w, b, ref = E.conv_forward_problem(regime, *CONV)
    a, bm = _im2col(x, w, 1)
    ref2 = ref.reshape(-1, CONV[4]) - b
    assert torch.equal(E.emulated_gemm(a, bm, n_planes=1).double(), ref2)
    assert _mismatch(E.emulated_gemm(a, bm, n_planes=1, drop_rows=torch.arange(32, 64)), ref2) > 0.5
    if regime == 'f16':        # the 11th bit matters: operands rounded to 10 bits give another result
        a10 = (a * 512).round() / 512
        assert _mismatch(a10 @ bm, ref2) > 0.5


@pytest.mark.parametrize("regime", E.REGIMES3)
def test_three_plane_values_have_the_planes_they_promise(regime):
    g = E.gen('planes', regime)
    ka, kb, pa, pb = E.kinds(regime)
    a, b = ka((4096,), g), kb((4096,), g)
    if pa is None:
        assert a.abs().max() == 2 and b.abs().max() == 1 and (a == 0).any()
        return
    assert torch.all(E.nonzero_planes(a) == pa) and torch.all(E.nonzero_planes(b) == pb)
    hi, mid, lo = E.split3(a if pa >= pb else b)
    assert torch.all(mid.abs() == 2.0 ** -9)
    if max(pa, pb) == 3:
        assert torch.all(lo.abs() == 2.0 ** -18) and torch.all(hi.abs() >= 1 - 2.0 ** -8) and torch.all(hi.abs() <= 1.75)


@pytest.mark.parametrize("regime", E.REGIMES3 + ('f16',))
@pytest.mark.parametrize("op", ["dgrad", "wgrad", "deconv_fwd", "deconv_dgrad", "deconv_wgrad"])
def test_gradient_and_deconv_problems_meet_the_condition(op, regime):
    """The generators assert the condition themselves (assert_condition); here: they do so for every op form, the sparse operand
    reaches the edges, and the result is not trivially sparse."""
    case, dec = (DECONV, True) if op.startswith("deconv") else (CONV_S2, False)
    kind = op.split("_")[-1]
    if kind == "fwd":
        a, b, _, ref = E.conv_forward_problem(regime, *case, deconv=dec)
    elif kind == "dgrad":
        a, b, ref = E.conv_dgrad_problem(regime, *case, deconv=dec)
    else:
        a, b, ref = E.conv_wgrad_problem(regime, *case, deconv=dec)
    assert (ref != 0).double().mean() > 0.4
    sparse = a if regime == 'B3' and kind != "wgrad" else b
    if sparse.dim() == 4 and sparse.shape[0] == sparse.shape[1]:              # weights: first and last tap
        assert (sparse[0, 0] != 0).any() and (sparse[-1, -1] != 0).any()
    else:                                                                     # sites: last row, last column, last channel
        assert (sparse[:, -1] != 0).any() and (sparse[:, :, -1] != 0).any() and (sparse[..., -1] != 0).any()


@pytest.mark.parametrize("regime", E.REGIMES3)
def test_correlation_problems_and_their_references(regime, oracle_lib):
    """The fp64 cost volume and its adjoint used by the GPU tests agree with the scalar C oracle — bit for bit, since on these
    inputs the oracle's fp32 sums are exact too — and with autograd."""
    import numpy as np
    N, C, H, W, md, pad, s2 = 2, 32, 7, 12, 4, 5, 2
    attrs = dict(kernel_size=1, max_displacement=md, pad=pad, stride_1=1, stride_2=s2)
    f0, f1, ref = E.corr_forward_problem(regime, N, C, H, W, md, pad, s2)
    nchw = lambda t: np.ascontiguousarray(t.permute(0, 3, 1, 2).numpy().astype(np.float32))      # noqa: E731
    assert np.array_equal(oracle_lib.correlation(nchw(f0), nchw(f1), **attrs).astype(np.float64), nchw(ref).astype(np.float64))
    dout, f, refs = E.corr_backward_problem(regime, N, C, H, W, md, pad, s2)
    g0, g1 = oracle_lib.correlation_grad(nchw(dout), nchw(f), nchw(torch.roll(f, -1, 0)), **attrs)
    for q, r in zip((g0, np.roll(g1, 1, axis=0)), refs):
        assert np.array_equal(q.astype(np.float64), nchw(r).astype(np.float64)) and (q != 0).any()
    fa, fb = f0.clone().requires_grad_(), f1.clone().requires_grad_()
    d = torch.randn(ref.shape, dtype=torch.float64, generator=E.gen('d'))
    E.corr_forward_ref(fa, fb, md, pad, s2).backward(d)
    ga, gb = E.corr_backward_ref(d, f0, f1, md, pad, s2)
    assert torch.allclose(ga, fa.grad, rtol=1e-12, atol=1e-12) and torch.allclose(gb, fb.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case,dec", [(CONV, False), (CONV_S2, False), (DECONV, True), ((1, 7, 9, 6, 5, 4, 2), False)])
def test_filter_gradient_reference_is_autograd(case, dec):
    """wgrad_ref (one GEMM per tap) against autograd through the model's conv / conv_transpose."""
    B, H, W, Cin, Cout, k, stride = case
    g = E.gen('wgrad_ref', case)
    Ho, Wo = (2 * H, 2 * W) if dec else (-(-H // stride), -(-W // stride))
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    dz = torch.randn(B, Ho, Wo, Cout, generator=g, dtype=torch.float64)
    w0 = torch.zeros((4, 4, Cout, Cin) if dec else (k, k, Cin, Cout), dtype=torch.float64, requires_grad=True)
    want = torch.autograd.grad(E._conv_ref(x, w0, None, stride, dec), w0, dz)[0]
    assert torch.allclose(E.wgrad_ref(x, dz, k, stride, dec), want, rtol=1e-12, atol=1e-12)
