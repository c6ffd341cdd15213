"""The comparators and inputs of tests/test_loss_kernels_gpu.py proven without a GPU (tests/loss_parity.py): the fp32 torch-CPU
evaluation of the oracle's functions stands in for the kernels and must pass every assertion the GPU tests make against the
fp64 reference; one wrong border pixel or one wrong mask bit must fail them; the input margins hold."""
import pytest
import torch

import loss_parity as P

F32, F64 = torch.float32, torch.float64


def _pair(fn, *a):
    return fn(*a, F32), fn(*a, F64)


def _check_term(r32, r64, keys, exclude=None):
    P.check_loss(r32['loss'], r64['loss'])
    for k in keys:
        bound, own = P.grad_bound(r32[k], r64[k], exclude)
        assert bound < 1e-3, (k, bound)            # the sensitivity the suite promises (test_one_wrong_border_pixel_fails)
        assert P.check_grad(r32[k], r64[k], bound, exclude) == own


@pytest.mark.parametrize("name,kind", P.SMOOTH_CASES)
@pytest.mark.parametrize("term", ['second_order', 'smooth_1st'])
def test_smoothness_terms_fp32_oracle_passes(term, name, kind):
    _check_term(*_pair(P.ref_smooth, term, name, kind), ['d_flow'])


@pytest.mark.parametrize("name,kind", P.WARP_CASES)
def test_photometric_and_sobel_fp32_oracle_passes(name, kind):
    for n_mask in (1, P.SHAPES[name][0]):
        r32, r64 = _pair(P.ref_photometric, name, kind, n_mask)
        _check_term(r32, r64, ['d_flow'], r64['kink'])
        _check_term(*_pair(P.ref_gradient, name, kind, n_mask), ['d_im2w'])
        _check_term(*_pair(P.ref_gradient_chain, name, kind, n_mask), ['d_flow'])


@pytest.mark.parametrize("name,kind", P.GRAY_CASES)
def test_warped_gray_fp32_oracle_passes(name, kind):
    r32, r64 = _pair(P.ref_warp_gray, name, kind)
    for k in ('gray1', 'gray2w'):
        bound, _ = P.grad_bound(r32[k], r64[k], floor=1e-6)
        P.check_grad(r32[k], r64[k], bound)


@pytest.mark.parametrize("name,kind,D,n_mask", [c for c in P.CENSUS_CASES if c[:3] != ('BIG', 'm4.0', 4)])
def test_census_fp32_oracle_passes(name, kind, D, n_mask):
    """(BIG at D = 4 is left to the GPU run: its bound comes from the oracle there as well, and the fp64 patch tensors take GBs.)"""
    r32, r64 = _pair(P.ref_census, name, kind, D, P.n_of(n_mask, name))
    _check_term(r32, r64, ['d_dist', 'd_gray2w'])
    if D == 0:
        assert r64['d_gray2w'].abs().max().item() == 0.0 and r64['d_dist'].abs().max().item() == 0.0


@pytest.mark.parametrize("name,kind,mode,n_base", P.MASK_CASES)
def test_mask_terms_fp32_oracle_passes(name, kind, mode, n_base):
    for w in P.MASK_WEIGHTS:
        r32, r64 = _pair(P.ref_mask_terms, name, kind, mode, P.n_of(n_base, name), w)
        P.check_mask(r32['mask'], r64['mask'])            # exact: the margins keep every threshold away from fp32 rounding
        _check_term(r32, r64, ['d_flow', 'd_warped'] if w[0] else [])
    m = r64['mask']
    assert name == 'TINY' or 0.02 < (m != 0).float().mean().item() < 0.995      # both mask values occur


# ------------------------------------------------------------------------------------------------ sensitivity
def _border_pixels(t):
    """(n, y, x) of a corner, an edge pixel of the last row and one of the last column of the last sample."""
    N, H, W = t.shape[:3]
    return [(0, 0, 0), (N - 1, H - 1, W // 2), (N - 1, H // 2, W - 1)]


@pytest.mark.parametrize("name", ['RAGGED', 'BIG'])
def test_one_wrong_border_pixel_fails(name):
    """One element off by 1e-3 of the tensor's max — far below what a scalar loss or a share-of-pixels check sees."""
    kind = 'm1.5'
    refs = [(P.ref_smooth('second_order', name, kind, F64)['d_flow'], None),
            (P.ref_census(name, kind, 1, 1, F64)['d_gray2w'], None),
            (P.ref_photometric(name, kind, 1, F64)['d_flow'], P.ref_photometric(name, kind, 1, F64)['kink'])]
    for ref, exclude in refs:
        for px in _border_pixels(ref):
            if exclude is not None and exclude[px]:
                continue
            bad = ref.clone()
            bad[px] += 1e-3 * ref.abs().max()
            with pytest.raises(AssertionError):
                P.check_grad(bad.float(), ref, P.GRAD_TOL, exclude)
        bad = ref.clone().float()
        bad[0, 0, 0] = float('nan')                      # an element the kernel never wrote
        with pytest.raises(AssertionError):
            P.check_grad(bad, ref, P.GRAD_TOL, exclude)


@pytest.mark.parametrize("name", ['RAGGED', 'BIG'])
def test_one_wrong_mask_bit_fails(name):
    ref = P.ref_mask_terms(name, 'm1.5', 1, 0, P.MASK_WEIGHTS[3], F64)['mask']
    for px in _border_pixels(ref):
        bad = ref.clone()
        bad[px] = 1.0 - bad[px]
        with pytest.raises(AssertionError):
            P.check_mask(bad, ref)
    P.check_mask(ref.clone(), ref)


def test_loss_comparator_and_exclusion_cap():
    P.check_loss(1.0 + 5e-6, 1.0)
    with pytest.raises(AssertionError):
        P.check_loss(1.0 + 2e-5, 1.0)
    with pytest.raises(AssertionError):
        P.check_loss(float('nan'), 1.0)
    ref = torch.ones(1, 40, 50, 2, dtype=F64)
    got = ref.clone()
    got[0, 3, 4] = 5.0
    ex = torch.zeros(1, 40, 50, dtype=torch.bool)
    ex[0, 3, 4] = True                                   # 1 of 2000 pixels = 5e-4: allowed, and it hides the wrong pixel
    assert P.check_grad(got, ref, 1e-6, ex) == 0.0
    ex[0, 0, 0] = True                                   # 2 of 2000: over the cap
    with pytest.raises(AssertionError):
        P.check_grad(got, ref, 1e-6, ex)
    with pytest.raises(AssertionError):
        P.check_grad(got, ref, 1e-6)
    zero = torch.zeros(2, 3, 4)
    assert P.check_grad(zero, zero.double(), 0.0) == 0.0     # an all-zero reference demands exact zeros
    with pytest.raises(AssertionError):
        P.check_grad(zero + 1e-30, zero.double(), 1.0)


# ------------------------------------------------------------------------------------------------ inputs
@pytest.mark.parametrize("name,kind", P.WARP_CASES)
def test_input_margins_and_kink_share(name, kind):
    inp = P.make_inputs(name, kind)
    N, H, W = P.SHAPES[name]
    assert inp['flow'].dtype == F32 and inp['im'].dtype == F32 and tuple(inp['flow'].shape) == (N, H, W, 2)
    assert P.frac_margin(inp['flow'], inp['fs']).min().item() >= P.FRAC_MARGIN
    if kind == 'far':
        far = (inp['flow'].abs() > 40).any(3).float().mean().item()
        assert 0.1 < far < 0.3, far
    for n_mask in (1, N):
        assert P.ref_photometric(name, kind, n_mask, F64)['kink'].float().mean().item() <= P.KINK_SHARE_CAP


@pytest.mark.parametrize("name,kind", sorted({c[:2] for c in P.MASK_CASES}))
def test_mask_input_margins(name, kind):
    inp = P.make_mask_inputs(name, kind)
    assert P.frac_margin(inp['flow'], inp['fs']).min().item() >= P.FRAC_MARGIN
    for m in P.mask_margins(inp['flow'], inp['warped'], inp['fwarp'], inp['fs']):
        assert m.min().item() >= P.THRESH_MARGIN


def test_second_pass_shapes():
    """BIG is past every cap (2048 blocks of 256 threads, 2048 census tiles, 2048 warp tiles), XCD leaves a remainder."""
    N, H, W = P.SHAPES['BIG']
    cdiv = lambda a, b: -(-a // b)
    assert N * H * W > 2048 * 256 and N * cdiv(H, 8) * cdiv(W, 32) == 2100 and N * cdiv(H, 4) * cdiv(W, 64) == 2184
    N, H, W = P.SHAPES['XCD']
    assert cdiv(N * H * W, 256) == 41 and N * cdiv(H, 8) * cdiv(W, 32) == 60
